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
// Every argument is checked on the host before the first device call.
int plonk_pk_upload(gm_ctx* ctx, int curve, const gm_plonk_pk_host* host, unsigned flags, gm_plonk_pk** out);
void plonk_pk_release(gm_plonk_pk* pk);
// frees the key's parked session buffer and takes the key off its context's list
void plonk_spare_release(gm_plonk_pk* pk);
}  // namespace gm
