// A PLONK proving key resident on the device (see plonk_pk.hip): both SRSs in the
// MSM's layout, the fixed polynomials in the bases the prover stages take them
// in, and (optionally) their values on the four cosets of the 4n domain.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/gnark_mi355x.h"
#include "plonk.hpp"

struct gm_plonk_pk {
  gm_ctx* ctx = nullptr;
  int curve = 0;
  size_t n = 0, nb_public = 0, nb_bsb = 0;
  std::vector<size_t> commitment_row;
  void* srs_canonical = nullptr;  // prepared (gm_points_upload), srs_canonical_len points
  size_t srs_canonical_len = 0;
  void* srs_lagrange = nullptr;  // prepared, n points
  // One allocation of (11 + nb_bsb) polynomials of n elements, regular order:
  // canonical ql qr qm qo s1 s2 s3 qcp_0 .., then Lagrange qk s1 s2 s3.
  void* polys = nullptr;
  void* cache = nullptr;  // PlonkCosetCache::base, or nullptr (GM_PLONK_PK_NO_COSET_CACHE)
  bool lin_key_qk = false;  // GM_PLONK_PK_LIN_KEY_QK: round 4 linearises with the key's Qk, as gnark does
  size_t resident_bytes = 0, cache_bytes = 0;
  // The canonical SRS points G_0 G_1 G_2 G_n G_n+1 G_n+2 (gnark affine), copied at
  // upload: the blinding of a commitment, sum_k b_k (G_n+k - G_k), and the
  // StatisticalZK edits of the quotient shards (G_0, G_n+2) are a few host
  // scalar multiplications on them.
  std::vector<uint8_t> edge;
  // The buffer of the last freed session (plonk_session.hip), kept for the next
  // gm_plonk_session_begin on this key: a prover loop allocates once, not per
  // proof.  Host bookkeeping only: no proof reads what an earlier one left in
  // it.  Released by gm_trim, gm_destroy and gm_plonk_pk_free; not counted in
  // resident_bytes.
  void* spare_buf = nullptr;
  size_t spare_bytes = 0;

  enum { QL, QR, QM, QO, S1, S2, S3, NCANON };
  const void* canonical(size_t k) const { return (const char*)polys + 32 * n * k; }
  const void* qcp(size_t j) const { return canonical(NCANON + j); }
  enum { LAG_QK, LAG_S1, LAG_S2, LAG_S3 };
  const void* lagrange(size_t k) const { return canonical(NCANON + nb_bsb + k); }
  gm::PlonkCosetCache coset_cache() const { return {cache, n, nb_bsb}; }
};

namespace gm {
// What both ways of making a key are given (gm_plonk_pk_host and
// gm_plonk_setup_host share these members): the key's fixed part.
// A selector column that is made on the device instead of copied from the
// host: fill queues column `which` (GM_SCS_QL .. GM_SCS_QCP0 + j), n elements,
// Lagrange regular, at out_dev on ctx->stream.
struct PlonkColumnGen {
  int (*fill)(gm_ctx* ctx, const void* self, unsigned which, void* out_dev);
  const void* self;
};
struct PlonkPkFixed {
  size_t n, nb_public;
  const void *ql, *qr, *qm, *qo, *qk;
  size_t nb_bsb;
  const void* const* qcp;
  const size_t* commitment_row;
  const void* srs_canonical;
  size_t srs_canonical_len;
  // the columns' source: nullptr = the host vectors above; otherwise those (and
  // qcp) are not read
  const PlonkColumnGen* gen = nullptr;
};
// Every argument is checked on the host before the first device call.
int plonk_pk_upload(gm_ctx* ctx, int curve, const gm_plonk_pk_host* host, unsigned flags, gm_plonk_pk** out);
// The three steps of plonk_pk_upload, shared with plonk_pk_setup (plonk_setup.hip):
//  * the refusals (other_null: a pointer of the caller's own part is NULL);
//  * a new key with the canonical SRS prepared, the six edge points copied and the
//    polynomials allocated (the caller holds the context's lock);
//  * the tail, once pk->srs_lagrange is prepared and s1, s2, s3 lie in their
//    Lagrange slots: every polynomial in the bases the prover takes it in, the
//    coset cache.  vk_digests (host, 8 + nb_bsb gnark G1Affine, or NULL) receives
//    the commits of S1 S2 S3 Ql Qr Qm Qo Qk Qcp_j over the Lagrange SRS, taken
//    while each polynomial's Lagrange values are on the device.
// After a failure of the second or third the caller drains the stream and
// releases the key.
int plonk_pk_check(int curve, const PlonkPkFixed& f, unsigned flags, bool other_null);
int plonk_pk_begin(gm_ctx* ctx, int curve, const PlonkPkFixed& f, gm_plonk_pk** out);
int plonk_pk_finish(gm_ctx* ctx, const PlonkPkFixed& f, unsigned flags, gm_plonk_pk* pk, void* vk_digests);
void plonk_pk_release(gm_plonk_pk* pk);
// frees the key's parked session buffer and takes the key off its context's list
void plonk_spare_release(gm_plonk_pk* pk);
}  // namespace gm
