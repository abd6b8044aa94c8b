// Test hooks of PLONK verification (include/gnark_mi355x_testhooks.h): the scalars
// kernel alone, and the batch entry with a given chunk.  Not in the product library.
#include "curves.hpp"
#include "plonk_verify.hpp"
#include "../../include/gnark_mi355x_testhooks.h"

using namespace gm;

extern "C" int gm_test_plonk_verify_scalars(gm_ctx* ctx, const gm_plonk_vk* vk, const gm_plonk_proofs_host* in,
                                            size_t m, void* scalars_out, void* aux_out, uint8_t* class_out) {
  if (!ctx || !vk || vk->ctx != ctx || !in || !in->values || !in->challenges || !scalars_out || !aux_out || !class_out ||
      (vk->nb_public && !in->publics) || (vk->nb_bsb && !in->hashed_cmt) || m == 0 || m > 4096)
    return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  const size_t nb = vk->nb_bsb, nbp = vk->nb_public, NV = pv_values(nb), T = pv_terms(nb), K = nbp + nb + 1;
  DevBuf vals, pubs, hashed, chal, prefix, scal, aux, pre;
  int rc;
  if ((rc = vals.alloc(arena, m * NV * 32)) || (rc = pubs.alloc(arena, std::max<size_t>(m * nbp * 32, 16))) ||
      (rc = hashed.alloc(arena, std::max<size_t>(m * nb * 32, 16))) || (rc = chal.alloc(arena, m * 6 * 32)) ||
      (rc = prefix.alloc(arena, m * K * pv_prefix_bytes(vk->curve))) || (rc = scal.alloc(arena, m * T * 32)) ||
      (rc = aux.alloc(arena, m * 2 * 32)) || (rc = pre.alloc(arena, m)))
    return rc;
  GM_HIP(hipMemcpyAsync(vals.p, in->values, m * NV * 32, hipMemcpyHostToDevice, ctx->stream));
  if (nbp) GM_HIP(hipMemcpyAsync(pubs.p, in->publics, m * nbp * 32, hipMemcpyHostToDevice, ctx->stream));
  if (nb) GM_HIP(hipMemcpyAsync(hashed.p, in->hashed_cmt, m * nb * 32, hipMemcpyHostToDevice, ctx->stream));
  GM_HIP(hipMemcpyAsync(chal.p, in->challenges, m * 6 * 32, hipMemcpyHostToDevice, ctx->stream));
  PvDev d = {};
  d.values = vals.p, d.publics = pubs.p, d.hashed = hashed.p, d.chal = chal.p;
  d.key_g1 = vk->g1, d.key_g2 = vk->g2, d.key_fr = vk->fr;
  d.m = m, d.nb_public = nbp, d.nb_bsb = nb, d.logn = vk->logn;
  d.st_g1 = nullptr;
  d.prefix = prefix.p, d.scal = scal.p, d.aux = aux.p, d.pre = pre.as<uint8_t>();
  if ((rc = GM_CURVE(vk->curve, pv_scalars_launch<C>(ctx, d)))) return rc;
  GM_HIP(hipMemcpyAsync(scalars_out, scal.p, m * T * 32, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipMemcpyAsync(aux_out, aux.p, m * 2 * 32, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipMemcpyAsync(class_out, pre.p, m, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

extern "C" int gm_test_plonk_verify_chunked(gm_ctx* ctx, const gm_plonk_vk* vk, const gm_plonk_proofs_host* in,
                                            size_t m, size_t per_chunk, uint8_t* status_out, size_t* nb_ok) {
  if (!ctx || !vk || vk->ctx != ctx || !in || !in->points || !in->values || !in->challenges || !status_out ||
      (vk->nb_public && !in->publics) || (vk->nb_bsb && !in->hashed_cmt) || m == 0 || per_chunk == 0)
    return GM_ERR_INVALID;
  return plonk_verify_run(ctx, vk, in, m, per_chunk, status_out, nb_ok);
}

extern "C" int gm_test_kzg_verify_chunked(gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* in, size_t m,
                                          size_t per_chunk, int fold, uint8_t* status_out, size_t* nb_ok) {
  if (!ctx || !vk || vk->ctx != ctx || !in || !in->digests || !in->proofs || !in->points || !in->values ||
      (fold && !in->lambda) || !status_out || m == 0 || per_chunk == 0)
    return GM_ERR_INVALID;
  return kzg_verify_batch(ctx, vk, in, m, per_chunk, fold != 0, status_out, nb_ok);
}
