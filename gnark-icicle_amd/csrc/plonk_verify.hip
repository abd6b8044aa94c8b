// Batched KZG and PLONK verification, host side: the verifying keys, dispatch by
// curve id and the chunking of the streamed entries.  The kernels are
// plonk_verify_impl.hpp, instantiated per curve; the pairing is pairing_impl.hpp's.
#include "plonk_verify.hpp"

#include <vector>

#include "curves.hpp"
#include "ntt.hpp"
#include "points_check.hpp"

namespace gm {

namespace {

constexpr size_t FAN = 16;  // PR_FAN of pairing_impl.hpp

const char* class_name(uint32_t cls) {
  switch (cls) {
    case GM_POINT_NOT_REDUCED: return "a coordinate is not below p";
    case GM_POINT_OFF_CURVE: return "not on the curve";
    case GM_POINT_OFF_SUBGROUP: return "not in the subgroup";
  }
  return "ok";
}

// np products of two pairs each: Miller lanes, one reduce launch, the final exponentiation
struct PairWs {
  DevBuf a, b, ok;
  int alloc(Arena& arena, int curve, size_t np) {
    const size_t gt = pairing_gt_bytes(curve);
    if (int rc = a.alloc(arena, 2 * np * gt)) return rc;
    if (int rc = b.alloc(arena, np * gt)) return rc;
    return ok.alloc(arena, std::max<size_t>(np, 16));
  }
};
int pairs_queue(gm_ctx* ctx, int curve, const void* g1, const void* g2, size_t np, const PairWs& ws) {
  int rc;
  if ((rc = GM_CURVE(curve, pairing_miller_launch<C>(ctx, g1, g2, 2 * np, ws.a.p)))) return rc;
  if ((rc = GM_CURVE(curve, pairing_reduce_launch<C>(ctx, ws.a.p, np, 2, 1, ws.b.p)))) return rc;
  return GM_CURVE(curve, pairing_final_launch<C>(ctx, ws.b.p, np, ws.ok.as<uint8_t>()));
}

// uploads nothing: checks n points already on the device and names the first bad one
int check_members(gm_ctx* ctx, int curve, const char* entry, bool g2, const void* dev, size_t n,
                  const std::vector<std::string>& names) {
  gm_points_report rep;
  if (int rc = points_check_device(ctx, curve, g2, dev, n, nullptr, &rep)) return rc;
  if (rep.first_bad != rep.n) {
    set_error(std::string(entry) + ": " + names[rep.first_bad] +
              " fails the point check: " + class_name(rep.first_class));
    return GM_ERR_INVALID;
  }
  return GM_OK;
}

// the two G2 members to g2_dev, checked, the second negated
int upload_g2(gm_ctx* ctx, int curve, const char* entry, const void* g2_0, const void* g2_1, void* g2_dev,
              const char* n0, const char* n1) {
  const size_t b2 = 4 * fp_bytes(curve);
  GM_HIP(hipMemcpyAsync(g2_dev, g2_0, b2, hipMemcpyHostToDevice, ctx->stream));
  GM_HIP(hipMemcpyAsync((char*)g2_dev + b2, g2_1, b2, hipMemcpyHostToDevice, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  if (int rc = check_members(ctx, curve, entry, true, g2_dev, 2, {n0, n1})) return rc;
  if (int rc = GM_CURVE(curve, points_negate_launch<C, true>(ctx, (char*)g2_dev + b2, 1))) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

}  // namespace

// ---- KZG ---------------------------------------------------------------------------------
void kzg_vk_release(gm_kzg_vk* vk) {
  if (vk->g1) hipFree(vk->g1);
  if (vk->g2) hipFree(vk->g2);
  delete vk;
}

int kzg_vk_upload(gm_ctx* ctx, int curve, const gm_kzg_vk_host* in, gm_kzg_vk** out) {
  const char* me = "gm_kzg_vk_upload";
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const size_t b1 = 2 * fp_bytes(curve), b2 = 4 * fp_bytes(curve);
  gm_kzg_vk* vk = new gm_kzg_vk;
  vk->ctx = ctx;
  vk->curve = curve;
  auto fail = [&](int rc) {
    kzg_vk_release(vk);
    return rc;
  };
  if (hipMalloc(&vk->g1, b1) != hipSuccess || hipMalloc(&vk->g2, 2 * b2) != hipSuccess) {
    set_error(std::string(me) + ": device allocation failed");
    return fail(GM_ERR_OOM);
  }
  hipError_t e = hipMemcpyAsync(vk->g1, in->g1, b1, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    set_error(std::string(me) + ": copy: " + hipGetErrorString(e));
    return fail(GM_ERR_DEVICE);
  }
  if (int rc = check_members(ctx, curve, me, false, vk->g1, 1, {"g1"})) return fail(rc);
  if (int rc = upload_g2(ctx, curve, me, in->g2_0, in->g2_1, vk->g2, "g2_0", "g2_1")) return fail(rc);
  *out = vk;
  return GM_OK;
}

size_t kzg_verify_chunk(size_t m, bool fold) {
  // two Miller lanes per opening (per opening), and the ladder lanes
  return std::max<size_t>(std::min(m, std::min(PAIRING_CHUNK_PAIRS / 2, PV_CHUNK_LADDERS / (fold ? 4 : 2))), 1);
}

int kzg_verify_batch(gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* in, size_t m, size_t per, bool fold,
                     uint8_t* status_out, size_t* nb_ok) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  const int curve = vk->curve;
  const size_t fb = fp_bytes(curve), b1 = 2 * fb, b2 = 4 * fb, xb = 4 * fb, L = fold ? 4 : 2;
  per = std::min(std::max<size_t>(per, 1), m);
  const size_t np = fold ? 1 : per;
  DevBuf dc, dh, dz, dy, dl, stc, sth, bad, terms, pre, p1, p2, status, res, part, sum_a, sum_b;
  PairWs ws;
  int rc;
  if ((rc = dc.alloc(arena, per * b1)) || (rc = dh.alloc(arena, per * b1)) || (rc = dz.alloc(arena, per * 32)) ||
      (rc = dy.alloc(arena, per * 32)) || (rc = dl.alloc(arena, fold ? per * 32 : 16)) || (rc = stc.alloc(arena, per)) ||
      (rc = sth.alloc(arena, per)) || (rc = bad.alloc(arena, per)) || (rc = terms.alloc(arena, per * L * xb)) ||
      (rc = pre.alloc(arena, per)) || (rc = p1.alloc(arena, 2 * np * b1)) || (rc = p2.alloc(arena, 2 * np * b2)) ||
      (rc = status.alloc(arena, std::max<size_t>(np, 16))) ||
      (rc = res.alloc(arena, PC_RES_WORDS * sizeof(unsigned long long))) || (rc = ws.alloc(arena, curve, np)))
    return rc;
  if (fold) {
    const size_t lvl = (per + 1 + FAN - 1) / FAN;
    if ((rc = part.alloc(arena, (per + 1) * 2 * xb)) || (rc = sum_a.alloc(arena, lvl * 2 * xb)) ||
        (rc = sum_b.alloc(arena, ((lvl + FAN - 1) / FAN) * 2 * xb)))
      return rc;
    GM_HIP(hipMemsetAsync(part.p, 0, 2 * xb, ctx->stream));  // the carry: two infinities
  }
  std::vector<uint8_t> pre_host(fold ? per : 0);
  bool any_point = false, any_input = false;
  size_t accepted = 0;
  for (size_t i0 = 0; i0 < m; i0 += per) {
    const size_t cnt = std::min(per, m - i0);
    GM_HIP(hipMemcpyAsync(dc.p, (const char*)in->digests + i0 * b1, cnt * b1, hipMemcpyHostToDevice, ctx->stream));
    GM_HIP(hipMemcpyAsync(dh.p, (const char*)in->proofs + i0 * b1, cnt * b1, hipMemcpyHostToDevice, ctx->stream));
    GM_HIP(hipMemcpyAsync(dz.p, (const char*)in->points + i0 * 32, cnt * 32, hipMemcpyHostToDevice, ctx->stream));
    GM_HIP(hipMemcpyAsync(dy.p, (const char*)in->values + i0 * 32, cnt * 32, hipMemcpyHostToDevice, ctx->stream));
    if (fold)
      GM_HIP(hipMemcpyAsync(dl.p, (const char*)in->lambda + i0 * 32, cnt * 32, hipMemcpyHostToDevice, ctx->stream));
    GM_HIP(hipMemsetAsync(bad.p, 0, cnt, ctx->stream));
    KzgvDev d;
    d.digests = dc.p, d.proofs = dh.p, d.z = dz.p, d.y = dy.p, d.lambda = dl.p;
    d.key_g1 = vk->g1, d.key_g2 = vk->g2;
    d.m = cnt;
    d.first = i0 == 0;
    d.st_c = stc.as<uint8_t>(), d.st_h = sth.as<uint8_t>(), d.bad_input = bad.as<uint8_t>();
    d.terms = terms.p, d.pre = pre.as<uint8_t>(), d.pair_g1 = p1.p, d.pair_g2 = p2.p, d.part = part.p;
    unsigned long long* r = res.as<unsigned long long>();
    if ((rc = points_check_reset(ctx, r)) ||
        (rc = points_check_queue(ctx, curve, false, dc.p, cnt, 0, stc.as<uint8_t>(), r)) ||
        (rc = points_check_queue(ctx, curve, false, dh.p, cnt, 0, sth.as<uint8_t>(), r)) ||
        (rc = GM_CURVE(curve, kzgv_terms_launch<C>(ctx, d, fold))) ||
        (rc = GM_CURVE(curve, kzgv_assemble_launch<C>(ctx, d, fold))))
      return rc;
    if (!fold) {
      if ((rc = pairs_queue(ctx, curve, p1.p, p2.p, cnt, ws)) ||
          (rc = GM_CURVE(curve, g16_verify_status_launch<C>(ctx, d.pre, ws.ok.as<uint8_t>(), cnt, status.as<uint8_t>()))))
        return rc;
      GM_HIP(hipMemcpyAsync(status_out + i0, status.p, cnt, hipMemcpyDeviceToHost, ctx->stream));
      GM_HIP(hipStreamSynchronize(ctx->stream));  // the chunk's buffers are reused; no host pointer is retained
      for (size_t i = 0; i < cnt; i++) accepted += status_out[i0 + i] == GM_KZG_VERIFY_OK;
      continue;
    }
    // the chunk's partial sums and the carry, 16 per lane and launch, back into the carry
    const void* cur = part.p;
    void* bufs[2] = {sum_a.p, sum_b.p};
    int which = 0;
    for (size_t c = cnt + 1; c > 1;) {
      const size_t nc = (c + FAN - 1) / FAN;
      if ((rc = GM_CURVE(curve, kzgv_sum_launch<C>(ctx, cur, c, nc, bufs[which])))) return rc;
      cur = bufs[which];
      which ^= 1;
      c = nc;
    }
    GM_HIP(hipMemcpyAsync(part.p, cur, 2 * xb, hipMemcpyDeviceToDevice, ctx->stream));
    GM_HIP(hipMemcpyAsync(pre_host.data(), pre.p, cnt, hipMemcpyDeviceToHost, ctx->stream));
    GM_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < cnt; i++) {
      any_point = any_point || pre_host[i] == GM_KZG_VERIFY_BAD_POINT;
      any_input = any_input || pre_host[i] == GM_KZG_VERIFY_BAD_INPUT;
    }
    // a bad point decides the batch; a bad input does unless a later chunk holds a bad point
    if (any_point) break;
  }
  if (fold) {
    if (any_point || any_input) {
      status_out[0] = any_point ? GM_KZG_VERIFY_BAD_POINT : GM_KZG_VERIFY_BAD_INPUT;
    } else {
      uint8_t ok = 0;
      if ((rc = GM_CURVE(curve, kzgv_fold_pairs_launch<C>(ctx, part.p, vk->g2, p1.p, p2.p))) ||
          (rc = pairs_queue(ctx, curve, p1.p, p2.p, 1, ws)))
        return rc;
      GM_HIP(hipMemcpyAsync(&ok, ws.ok.p, 1, hipMemcpyDeviceToHost, ctx->stream));
      GM_HIP(hipStreamSynchronize(ctx->stream));
      status_out[0] = ok ? GM_KZG_VERIFY_OK : GM_KZG_VERIFY_MISMATCH;
    }
    accepted = status_out[0] == GM_KZG_VERIFY_OK;
  }
  if (nb_ok) *nb_ok = accepted;
  if (ctx->profiling) prof_collect(ctx);
  return GM_OK;
}

// ---- PLONK -------------------------------------------------------------------------------
void plonk_vk_release(gm_plonk_vk* vk) {
  if (vk->g1) hipFree(vk->g1);
  if (vk->g2) hipFree(vk->g2);
  if (vk->fr) hipFree(vk->fr);
  delete vk;
}

namespace {

template <class C>
int plonk_vk_fr(const gm_plonk_vk_host* in, uint32_t logn, std::vector<uint8_t>& out) {
  using HFr = typename C::HFr;
  using HF = host::F<HFr>;
  HF w;
  if (int rc = ntt_root<C>((int)logn, w.v)) return rc;
  std::vector<HF> v(PV_KEY_FR + in->nb_bsb);
  v[0] = host::finv(host::from_u64<HFr>(in->n));
  v[1] = w;
  v[2] = host::finv(w);
  v[3] = host::from_u64<HFr>(C::COSET_GEN);
  for (size_t j = 0; j < in->nb_bsb; j++) {
    const uint64_t e = in->commitment_row[j];
    v[PV_KEY_FR + j] = host::fpow(w, &e, 1);
  }
  static_assert(sizeof(HF) == 32, "one gnark fr.Element");
  out.resize(v.size() * sizeof(HF));
  memcpy(out.data(), v.data(), out.size());
  return GM_OK;
}

}  // namespace

int plonk_vk_upload(gm_ctx* ctx, int curve, const gm_plonk_vk_host* in, gm_plonk_vk** out) {
  const char* me = "gm_plonk_vk_upload";
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const size_t b1 = 2 * fp_bytes(curve), b2 = 4 * fp_bytes(curve), nb = in->nb_bsb;
  uint32_t logn = 0;
  while ((size_t(1) << logn) < in->n) logn++;
  std::vector<uint8_t> fr;
  if (int rc = GM_CURVE(curve, plonk_vk_fr<C>(in, logn, fr))) return rc;
  // G, Ql, Qr, Qm, Qo, S3, S1, S2, Qcp[j], Qk
  const void* single[PV_KEY_LADDERS] = {in->kzg_g1, in->ql, in->qr, in->qm, in->qo, in->s3, in->s1, in->s2};
  std::vector<std::string> names = {"kzg_g1", "ql", "qr", "qm", "qo", "s3", "s1", "s2"};
  const size_t npts = PV_KEY_LADDERS + nb + 1;
  std::vector<uint8_t> pts(npts * b1);
  for (size_t k = 0; k < PV_KEY_LADDERS; k++) memcpy(pts.data() + k * b1, single[k], b1);
  if (nb) memcpy(pts.data() + PV_KEY_LADDERS * b1, in->qcp, nb * b1);
  for (size_t j = 0; j < nb; j++) names.push_back("qcp[" + std::to_string(j) + "]");
  memcpy(pts.data() + (PV_KEY_LADDERS + nb) * b1, in->qk, b1);
  names.push_back("qk");

  gm_plonk_vk* vk = new gm_plonk_vk;
  vk->ctx = ctx;
  vk->curve = curve;
  vk->n = in->n, vk->nb_public = in->nb_public, vk->nb_bsb = nb, vk->logn = logn;
  auto fail = [&](int rc) {
    plonk_vk_release(vk);
    return rc;
  };
  if (hipMalloc(&vk->g1, pts.size()) != hipSuccess || hipMalloc(&vk->g2, 2 * b2) != hipSuccess ||
      hipMalloc(&vk->fr, fr.size()) != hipSuccess) {
    set_error(std::string(me) + ": device allocation failed");
    return fail(GM_ERR_OOM);
  }
  hipError_t e = hipMemcpyAsync(vk->g1, pts.data(), pts.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(vk->fr, fr.data(), fr.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // pts and fr are this call's
  if (e != hipSuccess) {
    set_error(std::string(me) + ": copy: " + hipGetErrorString(e));
    return fail(GM_ERR_DEVICE);
  }
  if (int rc = check_members(ctx, curve, me, false, vk->g1, npts, names)) return fail(rc);
  if (int rc = upload_g2(ctx, curve, me, in->kzg_g2_0, in->kzg_g2_1, vk->g2, "kzg_g2_0", "kzg_g2_1")) return fail(rc);
  *out = vk;
  return GM_OK;
}

size_t pv_prefix_bytes(int curve) {
  return with_curve(
      curve,
      [](auto tag_) {
        using C = typename decltype(tag_)::type;
        return sizeof(Fe<typename C::Fr>);
      },
      (size_t)0);
}

size_t plonk_verify_chunk(const gm_plonk_vk* vk, size_t m) {
  size_t per = std::min(m, PAIRING_CHUNK_PAIRS / 2);
  per = std::min(per, std::max<size_t>(PV_CHUNK_LADDERS / pv_terms(vk->nb_bsb), 1));
  per = std::min(per, std::max<size_t>(PV_CHUNK_PREFIX / (vk->nb_public + vk->nb_bsb + 1), 1));
  return std::max<size_t>(per, 1);
}

int plonk_verify_run(gm_ctx* ctx, const gm_plonk_vk* vk, const gm_plonk_proofs_host* in, size_t m, size_t per,
                     uint8_t* status_out, size_t* nb_ok) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  const int curve = vk->curve;
  const size_t fb = fp_bytes(curve), b1 = 2 * fb, b2 = 4 * fb, xb = 4 * fb;
  const size_t nb = vk->nb_bsb, nbp = vk->nb_public, NP = pv_proof_points(nb), NV = pv_values(nb), T = pv_terms(nb);
  const size_t K = nbp + nb + 1;
  per = std::min(std::max<size_t>(per, 1), m);
  DevBuf pts, vals, pubs, hashed, chal, st, prefix, scal, aux, pre, terms, p1, p2, status, res;
  PairWs ws;
  int rc;
  if ((rc = pts.alloc(arena, per * NP * b1)) || (rc = vals.alloc(arena, per * NV * 32)) ||
      (rc = pubs.alloc(arena, std::max<size_t>(per * nbp * 32, 16))) ||
      (rc = hashed.alloc(arena, std::max<size_t>(per * nb * 32, 16))) || (rc = chal.alloc(arena, per * 6 * 32)) ||
      (rc = st.alloc(arena, per * NP)) || (rc = prefix.alloc(arena, per * K * pv_prefix_bytes(curve))) ||
      (rc = scal.alloc(arena, per * T * 32)) || (rc = aux.alloc(arena, per * 2 * 32)) || (rc = pre.alloc(arena, per)) ||
      (rc = terms.alloc(arena, per * T * xb)) || (rc = p1.alloc(arena, 2 * per * b1)) ||
      (rc = p2.alloc(arena, 2 * per * b2)) || (rc = status.alloc(arena, per)) ||
      (rc = res.alloc(arena, PC_RES_WORDS * sizeof(unsigned long long))) || (rc = ws.alloc(arena, curve, per)))
    return rc;
  size_t accepted = 0;
  for (size_t i0 = 0; i0 < m; i0 += per) {
    const size_t cnt = std::min(per, m - i0);
    auto up = [&](const DevBuf& dst, const void* src, size_t each) {
      return each == 0 ? hipSuccess
                       : hipMemcpyAsync(dst.p, (const char*)src + i0 * each, cnt * each, hipMemcpyHostToDevice,
                                        ctx->stream);
    };
    GM_HIP(up(pts, in->points, NP * b1));
    GM_HIP(up(vals, in->values, NV * 32));
    GM_HIP(up(pubs, in->publics, nbp * 32));
    GM_HIP(up(hashed, in->hashed_cmt, nb * 32));
    GM_HIP(up(chal, in->challenges, 6 * 32));
    PvDev d;
    d.points = pts.p, d.values = vals.p, d.publics = pubs.p, d.hashed = hashed.p, d.chal = chal.p;
    d.key_g1 = vk->g1, d.key_g2 = vk->g2, d.key_fr = vk->fr;
    d.m = cnt, d.nb_public = nbp, d.nb_bsb = nb, d.logn = vk->logn;
    d.st_g1 = st.as<uint8_t>();
    d.prefix = prefix.p, d.scal = scal.p, d.aux = aux.p, d.pre = pre.as<uint8_t>(), d.terms = terms.p;
    d.pair_g1 = p1.p, d.pair_g2 = p2.p;
    unsigned long long* r = res.as<unsigned long long>();
    // the proof's points arrive as one array: the point check takes it as it is
    if ((rc = points_check_reset(ctx, r)) ||
        (rc = points_check_queue(ctx, curve, false, pts.p, cnt * NP, 0, st.as<uint8_t>(), r)) ||
        (rc = GM_CURVE(curve, pv_scalars_launch<C>(ctx, d))) || (rc = GM_CURVE(curve, pv_terms_launch<C>(ctx, d))) ||
        (rc = GM_CURVE(curve, pv_assemble_launch<C>(ctx, d))) || (rc = pairs_queue(ctx, curve, p1.p, p2.p, cnt, ws)) ||
        (rc = GM_CURVE(curve, g16_verify_status_launch<C>(ctx, d.pre, ws.ok.as<uint8_t>(), cnt, status.as<uint8_t>()))))
      return rc;
    GM_HIP(hipMemcpyAsync(status_out + i0, status.p, cnt, hipMemcpyDeviceToHost, ctx->stream));
    GM_HIP(hipStreamSynchronize(ctx->stream));  // the chunk's buffers are reused; no host pointer is retained
    for (size_t i = 0; i < cnt; i++) accepted += status_out[i0 + i] == GM_PLONK_VERIFY_OK;
  }
  if (nb_ok) *nb_ok = accepted;
  if (ctx->profiling) prof_collect(ctx);
  return GM_OK;
}

}  // namespace gm
