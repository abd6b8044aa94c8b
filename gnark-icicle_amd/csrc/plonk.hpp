// PLONK quotient on the device (see plonk.hip): resident polynomials in, h out.
#pragma once
#include <cstddef>
#include "../../include/gnark_mi355x.h"
#include "curves.hpp"

namespace gm {
// Slots of one coset's block of a key's cache of coset evaluations (plonk_pk.hip):
// the polynomials of the quotient that never change for a key, Qcp_j at
// PC_FIXED + j.  Qk is not among them: its completed form differs per proof.
enum { PC_QL, PC_QR, PC_QM, PC_QO, PC_S1, PC_S2, PC_S3, PC_L1, PC_FIXED };
// base: 4 blocks (coset i = g w1^i <w0>) of PC_FIXED + nb_bsb slots of n elements
// each, position order and number form as coset4_ntt_device leaves them.
struct PlonkCosetCache {
  const void* base;
  size_t n, nb_bsb;
};
// fixed: device pointers to the canonical ql, qr, qm, qo, s1, s2, s3, qcp_0 ..
// (7 + nb_bsb polynomials of n elements); cache: 4 (PC_FIXED + nb_bsb) n elements.
// Queues on ctx->stream.
template <class C>
int plonk_coset_cache_build(gm_ctx* ctx, size_t n, const void* const* fixed, size_t nb_bsb, void* cache);

// h_dev[0..4n) = the polynomial of degree < 4n that is T / Z_H on g <w_4n>
// (include/gnark_mi355x.h, gm_plonk_quotient).  With a cache the fixed
// polynomials of `in` are not read (their pointers are still checked): their
// coset values come from the cache, and only qk, l, r, o, z and the pi2_j are
// transformed.  Queues on ctx->stream; the caller synchronises.
template <class C>
int plonk_quotient_device(gm_ctx* ctx, const gm_plonk_quotient_in* in, void* h_dev,
                          const PlonkCosetCache* cache = nullptr);
}  // namespace gm
