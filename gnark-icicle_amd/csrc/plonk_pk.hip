// A PLONK proving key resident on the device -- what gnark's plonk.ProvingKey
// (backend/plonk/bls12-377/setup.go) holds for the prover, uploaded once:
//   * both KZG SRSs in the MSM's internal layout (gm_points_upload's form);
//   * the fixed polynomials in canonical form (quotient, linearization, batch
//     opening), by the reversal plus inverse transform gm_plonk_perm_z uses for Z;
//     s1, s2, s3 and the incomplete Qk also as the Lagrange values they arrive in
//     (gm_plonk_perm_z takes the former that way; the session completes the latter);
//   * unless GM_PLONK_PK_NO_COSET_CACHE, the values of ql, qr, qm, qo, s1, s2, s3,
//     L1 and every qcp_j on the four cosets of the 4n domain, as the quotient's
//     transforms leave them (plonk_coset_cache_build, plonk.hip): 32 of the 52
//     transforms of a quotient at nb_bsb = 0 are then done once per key.
// No host pointer is kept.
#include <cstring>

#include "curves.hpp"
#include "msm.hpp"
#include "ntt.hpp"
#include "plonk_pk.hpp"
#include "runtime.hpp"

namespace gm {

void plonk_spare_release(gm_plonk_pk* pk) {
  if (pk->ctx) {
    auto& v = pk->ctx->plonk_spare_keys;
    v.erase(std::remove(v.begin(), v.end(), pk), v.end());
  }
  if (pk->spare_buf) hipFree(pk->spare_buf);
  pk->spare_buf = nullptr;
  pk->spare_bytes = 0;
}

void plonk_pk_release(gm_plonk_pk* pk) {
  if (!pk) return;
  if (pk->ctx) hipSetDevice(pk->ctx->device);
  plonk_spare_release(pk);
  for (void* p : {pk->srs_canonical, pk->srs_lagrange, pk->polys, pk->cache})
    if (p) hipFree(p);
  delete pk;
}

namespace {

int alloc_dev(void** out, size_t bytes, const char* what) {
  const hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) {
    *out = nullptr;
    set_error(std::string("plonk pk: hipMalloc of the ") + what + " (" + std::to_string(bytes) +
              " bytes): " + hipGetErrorString(e));
    return GM_ERR_OOM;
  }
  return GM_OK;
}

// the affine form of an MSM's result, as the session's digests take it
template <class C>
int commit_affine(gm_ctx* ctx, const void* scalars, const void* srs, size_t m, void* out) {
  using HP = typename GroupSel<C, false>::HF;
  HP j[3];
  if (int rc = msm_device<C, false>(ctx, scalars, srs, m, j, true)) return rc;
  const host::Aff<HP> a = host::to_aff(host::Jac<HP>{j[0], j[1], j[2]});
  memcpy(out, &a, sizeof(a));
  return GM_OK;
}

template <class C>
int finish_t(gm_ctx* ctx, const PlonkPkFixed& f, unsigned flags, gm_plonk_pk* pk, void* vk_digests) {
  const size_t n = f.n, nb = f.nb_bsb;
  int rc;
  const size_t pb = 2 * fp_bytes(pk->curve);
  Arena arena(ctx);
  DevBuf tmp;
  if ((rc = tmp.alloc(arena, 32 * n))) return rc;
  // selector column `which` (GM_SCS_QL .. GM_SCS_QCP0 + j) at dst: the host
  // vector, or what the key's generator makes of it on the device
  auto column = [&](unsigned which, const void* host, void* dst) -> int {
    if (f.gen) return f.gen->fill(ctx, f.gen->self, which, dst);
    GM_HIP(hipMemcpyAsync(dst, host, 32 * n, hipMemcpyHostToDevice, ctx->stream));
    return GM_OK;
  };
  // Lagrange regular (at `lag`, or column `which` through tmp; which < 0: it lies
  // at `lag` already) -> canonical regular at dst; its digest while it is there
  auto canonical = [&](int which, const void* host, void* lag, void* dst, size_t digest) -> int {
    void* src = lag ? lag : tmp.p;
    if (which >= 0)
      if (int r = column((unsigned)which, host, src)) return r;
    if (int r = bitrev_copy_device<C>(ctx, dst, src, n)) return r;
    if (int r = ntt_device<C>(ctx, dst, n, true, true, false)) return r;
    if (!vk_digests) return GM_OK;
    return commit_affine<C>(ctx, src, pk->srs_lagrange, n, (char*)vk_digests + pb * digest);
  };
  auto can = [&](size_t k) { return const_cast<void*>(pk->canonical(k)); };
  auto lag = [&](size_t k) { return const_cast<void*>(pk->lagrange(k)); };
  // the verifying key's order: S1 S2 S3 Ql Qr Qm Qo Qk Qcp_j
  const void* sel[4] = {f.ql, f.qr, f.qm, f.qo};
  static_assert(GM_SCS_QL == 0 && GM_SCS_QO == 3 && GM_SCS_QK == 4 && GM_SCS_QCP0 == 5, "the columns' numbering");
  for (int k = 0; k < 4; k++)
    if ((rc = canonical(GM_SCS_QL + k, sel[k], nullptr, can(gm_plonk_pk::QL + k), 3 + k))) return rc;
  for (int k = 0; k < 3; k++)
    if ((rc = canonical(-1, nullptr, lag(gm_plonk_pk::LAG_S1 + k), can(gm_plonk_pk::S1 + k), k))) return rc;
  for (size_t j = 0; j < nb; j++)
    if ((rc = canonical((int)(GM_SCS_QCP0 + j), f.gen ? nullptr : f.qcp[j], nullptr, can(gm_plonk_pk::NCANON + j),
                        8 + j)))
      return rc;
  if ((rc = column(GM_SCS_QK, f.qk, lag(gm_plonk_pk::LAG_QK)))) return rc;
  if (vk_digests)
    if ((rc = commit_affine<C>(ctx, lag(gm_plonk_pk::LAG_QK), pk->srs_lagrange, n, (char*)vk_digests + pb * 7)))
      return rc;
  const size_t poly_bytes = 32 * n * (gm_plonk_pk::NCANON + nb + 4);
  pk->resident_bytes = poly_bytes + msm_internal_point_bytes<C, false>() * (f.srs_canonical_len + n);

  pk->lin_key_qk = (flags & GM_PLONK_PK_LIN_KEY_QK) != 0;
  if (!(flags & GM_PLONK_PK_NO_COSET_CACHE)) {
    const size_t cb = 4 * (PC_FIXED + nb) * n * 32;
    if ((rc = alloc_dev(&pk->cache, cb, "coset cache"))) return rc;
    std::vector<const void*> fixed;
    for (size_t k = 0; k < gm_plonk_pk::NCANON + nb; k++) fixed.push_back(pk->canonical(k));
    if ((rc = plonk_coset_cache_build<C>(ctx, n, fixed.data(), nb, pk->cache))) return rc;
    pk->cache_bytes = cb;
    pk->resident_bytes += cb;
  }
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

}  // namespace

int plonk_pk_check(int curve, const PlonkPkFixed& f, unsigned flags, bool other_null) {
  const size_t n = f.n, nb = f.nb_bsb;
  int logn = 0;
  while (((size_t)1 << logn) < n && logn < 62) logn++;
  const int adicity = curve == GM_BN254 ? CurveBN254::TWO_ADICITY : CurveBLS12377::TWO_ADICITY;
  if (((size_t)1 << logn) != n || n < 8 || logn + 2 > adicity || logn + 2 > 30) {
    set_error("plonk pk: n must be a power of two >= 8 with 4n within the 2-adicity");
    return GM_ERR_INVALID;
  }
  if (flags & ~(GM_PLONK_PK_NO_COSET_CACHE | GM_PLONK_PK_LIN_KEY_QK)) {
    set_error("plonk pk: unknown flag");
    return GM_ERR_INVALID;
  }
  if (!f.srs_canonical) other_null = true;
  if (!f.gen)
    for (const void* p : {f.ql, f.qr, f.qm, f.qo, f.qk})
      if (!p) other_null = true;
  if (other_null) {
    set_error("plonk pk: the polynomials and both SRSs must be non-null");
    return GM_ERR_INVALID;
  }
  if (f.srs_canonical_len < n + 3) {
    set_error("plonk pk: the canonical SRS needs at least n + 3 points");
    return GM_ERR_INVALID;
  }
  if (f.nb_public > n) {
    set_error("plonk pk: more public inputs than rows");
    return GM_ERR_INVALID;
  }
  if (nb > 1024 || (nb && ((!f.gen && !f.qcp) || !f.commitment_row))) {
    set_error("plonk pk: nb_bsb > 0 needs the qcp table and the commitment rows (at most 1024 gates)");
    return GM_ERR_INVALID;
  }
  for (size_t j = 0; j < nb; j++) {
    if (!f.gen && !f.qcp[j]) {
      set_error("plonk pk: a qcp entry is null");
      return GM_ERR_INVALID;
    }
    if (f.commitment_row[j] >= n) {
      set_error("plonk pk: a commitment row lies outside the domain");
      return GM_ERR_INVALID;
    }
  }
  return GM_OK;
}

int plonk_pk_begin(gm_ctx* ctx, int curve, const PlonkPkFixed& f, gm_plonk_pk** out) {
  const size_t n = f.n, nb = f.nb_bsb;
  gm_plonk_pk* pk = new gm_plonk_pk;
  *out = pk;
  pk->ctx = ctx;
  pk->curve = curve;
  pk->n = n;
  pk->nb_public = f.nb_public;
  pk->nb_bsb = nb;
  if (nb) pk->commitment_row.assign(f.commitment_row, f.commitment_row + nb);
  pk->srs_canonical_len = f.srs_canonical_len;
  if (int rc = gm_points_upload(ctx, curve, 0, f.srs_canonical, f.srs_canonical_len, &pk->srs_canonical)) return rc;
  const size_t pb = 2 * fp_bytes(curve);
  pk->edge.resize(6 * pb);
  for (int k = 0; k < 3; k++) {
    memcpy(&pk->edge[k * pb], (const char*)f.srs_canonical + k * pb, pb);
    memcpy(&pk->edge[(3 + k) * pb], (const char*)f.srs_canonical + (n + k) * pb, pb);
  }
  return alloc_dev(&pk->polys, 32 * n * (gm_plonk_pk::NCANON + nb + 4), "polynomials");
}

int plonk_pk_finish(gm_ctx* ctx, const PlonkPkFixed& f, unsigned flags, gm_plonk_pk* pk, void* vk_digests) {
  return pk->curve == GM_BN254 ? finish_t<CurveBN254>(ctx, f, flags, pk, vk_digests)
                               : finish_t<CurveBLS12377>(ctx, f, flags, pk, vk_digests);
}

int plonk_pk_upload(gm_ctx* ctx, int curve, const gm_plonk_pk_host* h, unsigned flags, gm_plonk_pk** out) {
  const PlonkPkFixed f = {h->n,      h->nb_public, h->ql,  h->qr,  h->qm, h->qo, h->qk,
                          h->nb_bsb, h->qcp,       h->commitment_row, h->srs_canonical, h->srs_canonical_len};
  if (int rc = plonk_pk_check(curve, f, flags, !h->s1 || !h->s2 || !h->s3 || !h->srs_lagrange)) return rc;
  const size_t n = h->n;
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  gm_plonk_pk* pk = nullptr;
  int rc = plonk_pk_begin(ctx, curve, f, &pk);
  if (!rc) rc = gm_points_upload(ctx, curve, 0, h->srs_lagrange, n, &pk->srs_lagrange);
  if (!rc) {
    // s1, s2, s3 into their Lagrange slots, where gm_plonk_perm_z reads them
    const void* perm[3] = {h->s1, h->s2, h->s3};
    for (int k = 0; k < 3 && !rc; k++)
      if (hipMemcpyAsync(const_cast<void*>(pk->lagrange(gm_plonk_pk::LAG_S1 + k)), perm[k], 32 * n,
                         hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        set_error("plonk pk: upload of s1, s2, s3 failed");
        rc = GM_ERR_DEVICE;
      }
  }
  if (!rc) rc = plonk_pk_finish(ctx, f, flags, pk, nullptr);
  if (rc) {
    hipStreamSynchronize(ctx->stream);  // nothing queued may outlive the buffers
    plonk_pk_release(pk);
    return rc;
  }
  *out = pk;
  return GM_OK;
}

}  // namespace gm
