// Pairing-product checks and batched Groth16 verification, host side: dispatch by
// curve id, the chunking of the streamed entries and the verifying key.  The
// kernels are pairing_impl.hpp, instantiated per curve.
#include "pairing.hpp"

#include "curves.hpp"
#include "points_check.hpp"

namespace gm {

size_t pairing_gt_bytes(int curve) { return 12 * fp_bytes(curve); }

namespace {

constexpr size_t FAN = 16;  // PR_FAN of pairing_impl.hpp: values one lane multiplies per launch

int miller_queue(gm_ctx* ctx, int curve, const void* g1, const void* g2, size_t n, void* f) {
  return GM_CURVE(curve, pairing_miller_launch<C>(ctx, g1, g2, n, f));
}
int reduce_queue(gm_ctx* ctx, int curve, const void* in, size_t np, size_t cnt, size_t newcnt, void* out) {
  return GM_CURVE(curve, pairing_reduce_launch<C>(ctx, in, np, cnt, newcnt, out));
}
int final_queue(gm_ctx* ctx, int curve, const void* f, size_t n, uint8_t* ok) {
  return GM_CURVE(curve, pairing_final_launch<C>(ctx, f, n, ok));
}

// Workspace of the products of one chunk: the Miller values and the buffer the
// reduce launches alternate with.
struct ProductWs {
  DevBuf a, b, ok;
  int alloc(Arena& arena, int curve, size_t np, size_t k) {
    const size_t gt = pairing_gt_bytes(curve);
    if (int rc = a.alloc(arena, np * k * gt)) return rc;
    if (int rc = b.alloc(arena, np * ((k + FAN - 1) / FAN) * gt)) return rc;
    return ok.alloc(arena, np);
  }
};

// Queues Miller loops, the ceil(log16 k) reduce launches and the final
// exponentiation of np products of k pairs; ws.ok receives the np bytes.
int products_queue(gm_ctx* ctx, int curve, const void* g1_dev, const void* g2_dev, size_t np, size_t k,
                   const ProductWs& ws) {
  if (int rc = miller_queue(ctx, curve, g1_dev, g2_dev, np * k, ws.a.p)) return rc;
  void* cur = ws.a.p;
  void* other = ws.b.p;
  for (size_t cnt = k; cnt > 1;) {
    const size_t newcnt = (cnt + FAN - 1) / FAN;
    if (int rc = reduce_queue(ctx, curve, cur, np, cnt, newcnt, other)) return rc;
    std::swap(cur, other);
    cnt = newcnt;
  }
  return final_queue(ctx, curve, cur, np, ws.ok.as<uint8_t>());
}

// products per chunk: whole products, about PAIRING_CHUNK_PAIRS Miller lanes
size_t chunk_products(size_t n_products, size_t k) {
  return std::min(n_products, std::max<size_t>(PAIRING_CHUNK_PAIRS / k, 1));
}

}  // namespace

int pairing_check_device(gm_ctx* ctx, int curve, const void* g1_dev, const void* g2_dev, size_t n_products,
                         size_t k, uint8_t* ok_host) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  const size_t per = chunk_products(n_products, k);
  const size_t b1 = 2 * fp_bytes(curve), b2 = 4 * fp_bytes(curve);
  ProductWs ws;
  if (int rc = ws.alloc(arena, curve, per, k)) return rc;
  for (size_t j0 = 0; j0 < n_products; j0 += per) {
    const size_t np = std::min(per, n_products - j0);
    if (int rc = products_queue(ctx, curve, (const char*)g1_dev + j0 * k * b1, (const char*)g2_dev + j0 * k * b2, np,
                                k, ws))
      return rc;
    GM_HIP(hipMemcpyAsync(ok_host + j0, ws.ok.p, np, hipMemcpyDeviceToHost, ctx->stream));
    GM_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is reused by the next chunk
  }
  if (ctx->profiling) prof_collect(ctx);
  return GM_OK;
}

int pairing_check_host(gm_ctx* ctx, int curve, const void* g1_host, const void* g2_host, size_t n_products,
                       size_t k, uint8_t* ok_host) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  const size_t per = chunk_products(n_products, k);
  const size_t b1 = 2 * fp_bytes(curve), b2 = 4 * fp_bytes(curve);
  ProductWs ws;
  DevBuf d1, d2;
  if (int rc = d1.alloc(arena, per * k * b1)) return rc;
  if (int rc = d2.alloc(arena, per * k * b2)) return rc;
  if (int rc = ws.alloc(arena, curve, per, k)) return rc;
  for (size_t j0 = 0; j0 < n_products; j0 += per) {
    const size_t np = std::min(per, n_products - j0);
    GM_HIP(hipMemcpyAsync(d1.p, (const char*)g1_host + j0 * k * b1, np * k * b1, hipMemcpyHostToDevice, ctx->stream));
    GM_HIP(hipMemcpyAsync(d2.p, (const char*)g2_host + j0 * k * b2, np * k * b2, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = products_queue(ctx, curve, d1.p, d2.p, np, k, ws)) return rc;
    GM_HIP(hipMemcpyAsync(ok_host + j0, ws.ok.p, np, hipMemcpyDeviceToHost, ctx->stream));
    GM_HIP(hipStreamSynchronize(ctx->stream));  // the chunk's buffers are reused; the host arrays are not retained
  }
  if (ctx->profiling) prof_collect(ctx);
  return GM_OK;
}

// ---- Groth16 verifying key ------------------------------------------------------------
namespace {

const char* class_name(uint32_t cls) {
  switch (cls) {
    case GM_POINT_NOT_REDUCED: return "a coordinate is not below p";
    case GM_POINT_OFF_CURVE: return "not on the curve";
    case GM_POINT_OFF_SUBGROUP: return "not in the subgroup";
  }
  return "ok";
}

void vk_release(gm_g16_vk* vk) {
  if (vk->g1) hipFree(vk->g1);
  if (vk->g2) hipFree(vk->g2);
  delete vk;
}

}  // namespace

int g16_vk_upload(gm_ctx* ctx, int curve, const gm_g16_vk_host* in, gm_g16_vk** out) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const size_t b1 = 2 * fp_bytes(curve), b2 = 4 * fp_bytes(curve);
  if (in->nb_k > (~size_t(0)) / b1 - 1) {
    set_error("gm_g16_vk_upload: nb_k points do not fit the address space");
    return GM_ERR_INVALID;
  }
  gm_g16_vk* vk = new gm_g16_vk;
  vk->ctx = ctx;
  vk->curve = curve;
  vk->nb_k = in->nb_k;
  auto fail = [&](int rc) {
    vk_release(vk);
    return rc;
  };
  if (hipMalloc(&vk->g1, (1 + in->nb_k) * b1) != hipSuccess || hipMalloc(&vk->g2, 3 * b2) != hipSuccess) {
    set_error("gm_g16_vk_upload: device allocation failed");
    return fail(GM_ERR_OOM);
  }
  char* g1 = (char*)vk->g1;
  char* g2 = (char*)vk->g2;
  hipError_t e = hipMemcpyAsync(g1, in->alpha_g1, b1, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(g1 + b1, in->k_g1, in->nb_k * b1, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(g2, in->beta_g2, b2, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(g2 + b2, in->gamma_g2, b2, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(g2 + 2 * b2, in->delta_g2, b2, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    set_error(std::string("gm_g16_vk_upload: copy: ") + hipGetErrorString(e));
    return fail(GM_ERR_DEVICE);
  }
  struct Member {
    const char* name;
    bool g2;
    const void* dev;
    size_t n;
  };
  const Member members[5] = {{"alpha_g1", false, g1, 1},
                             {"beta_g2", true, g2, 1},
                             {"gamma_g2", true, g2 + b2, 1},
                             {"delta_g2", true, g2 + 2 * b2, 1},
                             {"k_g1", false, g1 + b1, in->nb_k}};
  for (const Member& mb : members) {
    gm_points_report rep;
    if (int rc = points_check_device(ctx, curve, mb.g2, mb.dev, mb.n, nullptr, &rep)) return fail(rc);
    if (rep.first_bad != rep.n) {
      set_error(std::string("gm_g16_vk_upload: ") + mb.name + "[" + std::to_string(rep.first_bad) +
                "] fails the point check: " + class_name(rep.first_class));
      return fail(GM_ERR_INVALID);
    }
  }
  // alpha, gamma and delta are kept negated
  int rc = GM_CURVE(curve, points_negate_launch<C, false>(ctx, g1, 1));
  if (!rc) rc = GM_CURVE(curve, points_negate_launch<C, true>(ctx, g2 + b2, 2));
  if (rc) return fail(rc);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_error("gm_g16_vk_upload: device error");
    return fail(GM_ERR_DEVICE);
  }
  *out = vk;
  return GM_OK;
}

// ---- batched verification ---------------------------------------------------------------
int g16_verify_batch(gm_ctx* ctx, const gm_g16_vk* vk, const void* proofs_host, const void* publics_host, size_t m,
                     uint8_t* status_out, size_t* nb_ok) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  const int curve = vk->curve;
  const size_t fb = fp_bytes(curve), b1 = 2 * fb, b2 = 4 * fb, rec = 2 * b1 + b2;
  const size_t nb_in = vk->nb_k - 1, in_bytes = nb_in * 32, term_bytes = 4 * fb;
  // proofs per chunk: four Miller lanes each, and at most about 2^20 ladder lanes
  size_t per = std::min(m, PAIRING_CHUNK_PAIRS / 4);
  if (nb_in) per = std::min(per, std::max<size_t>((size_t(1) << 20) / nb_in, 1));
  if (nb_in && per > (~size_t(0)) / (nb_in * term_bytes)) {
    set_error("gm_g16_verify_batch: the key's inputs do not fit the address space");
    return GM_ERR_INVALID;
  }
  DevBuf proofs, publics, chk1, chk2, st1, st2, terms, bad, p1, p2, pre, status, res;
  ProductWs ws;
  int rc;
  if ((rc = proofs.alloc(arena, per * rec)) || (rc = publics.alloc(arena, per * in_bytes)) ||
      (rc = chk1.alloc(arena, 2 * per * b1)) || (rc = chk2.alloc(arena, per * b2)) ||
      (rc = st1.alloc(arena, 2 * per)) || (rc = st2.alloc(arena, per)) ||
      (rc = terms.alloc(arena, per * nb_in * term_bytes)) || (rc = bad.alloc(arena, per)) ||
      (rc = p1.alloc(arena, 4 * per * b1)) || (rc = p2.alloc(arena, 4 * per * b2)) || (rc = pre.alloc(arena, per)) ||
      (rc = status.alloc(arena, per)) || (rc = res.alloc(arena, PC_RES_WORDS * sizeof(unsigned long long))) ||
      (rc = ws.alloc(arena, curve, per, 4)))
    return rc;
  size_t accepted = 0;
  for (size_t i0 = 0; i0 < m; i0 += per) {
    const size_t cnt = std::min(per, m - i0);
    GM_HIP(hipMemcpyAsync(proofs.p, (const char*)proofs_host + i0 * rec, cnt * rec, hipMemcpyHostToDevice,
                          ctx->stream));
    if (nb_in)
      GM_HIP(hipMemcpyAsync(publics.p, (const char*)publics_host + i0 * in_bytes, cnt * in_bytes,
                            hipMemcpyHostToDevice, ctx->stream));
    GM_HIP(hipMemsetAsync(bad.p, 0, cnt, ctx->stream));
    G16VerifyDev d;
    d.proofs = proofs.p;
    d.publics = publics.p;
    d.vk_g1 = vk->g1;
    d.vk_g2 = vk->g2;
    d.m = cnt;
    d.nb_in = nb_in;
    d.chk_g1 = chk1.p;
    d.chk_g2 = chk2.p;
    d.st_g1 = st1.as<uint8_t>();
    d.st_g2 = st2.as<uint8_t>();
    d.terms = terms.p;
    d.bad_input = bad.as<uint8_t>();
    d.pair_g1 = p1.p;
    d.pair_g2 = p2.p;
    d.pre = pre.as<uint8_t>();
    unsigned long long* r = res.as<unsigned long long>();
    if ((rc = GM_CURVE(curve, g16_verify_split_launch<C>(ctx, d))) || (rc = points_check_reset(ctx, r)) ||
        (rc = points_check_queue(ctx, curve, false, d.chk_g1, 2 * cnt, 0, d.st_g1, r)) ||
        (rc = points_check_queue(ctx, curve, true, d.chk_g2, cnt, 0, d.st_g2, r)) ||
        (rc = GM_CURVE(curve, g16_verify_terms_launch<C>(ctx, d))) ||
        (rc = GM_CURVE(curve, g16_verify_assemble_launch<C>(ctx, d))) ||
        (rc = products_queue(ctx, curve, d.pair_g1, d.pair_g2, cnt, 4, ws)) ||
        (rc = GM_CURVE(curve, g16_verify_status_launch<C>(ctx, d.pre, ws.ok.as<uint8_t>(), cnt, status.as<uint8_t>()))))
      return rc;
    GM_HIP(hipMemcpyAsync(status_out + i0, status.p, cnt, hipMemcpyDeviceToHost, ctx->stream));
    GM_HIP(hipStreamSynchronize(ctx->stream));  // the chunk's buffers are reused; no host pointer is retained
    for (size_t i = 0; i < cnt; i++) accepted += status_out[i0 + i] == GM_G16_VERIFY_OK;
  }
  if (nb_ok) *nb_ok = accepted;
  if (ctx->profiling) prof_collect(ctx);
  return GM_OK;
}

}  // namespace gm
