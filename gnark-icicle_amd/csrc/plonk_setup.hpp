// PLONK setup on the device (see plonk_setup.hip): the Lagrange-form SRS by an
// EC-FFT, S1, S2, S3 from the permutation, and the proving key built from what
// gnark's Setup holds.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/gnark_mi355x.h"

namespace gm {
// largest log2 n of the EC-FFT: the 2-adicity, and 30 as for every transform here
template <class C>
constexpr int ecfft_max_logn() {
  return C::TWO_ADICITY < 30 ? C::TWO_ADICITY : 30;
}
// out[i] = (1/n) sum_j w^(-ij) in[j] on n gnark G1Affine points (out == in allowed,
// no other overlap: the caller checks).  Scratch from the workspace; returns
// with the stream drained.
template <class C>
int kzg_srs_lagrange_device(gm_ctx* ctx, const void* srs_dev, size_t n, void* lagrange_dev);
// first entry of perm[0, 3n) outside [0, 3n), named in the error; host only
int plonk_perm_check(size_t n, const int64_t* perm);
// s_k[i] = g^(S / n) w^(S mod n), S = perm[kn + i] (checked by the caller).
// Returns with the stream drained.
template <class C>
int plonk_sigma_device(gm_ctx* ctx, size_t n, const int64_t* perm_host, void* s1, void* s2, void* s3);
// the same from the resident wire tables: the permutation is derived on the
// device (plonk_wires_perm.hip) and read as 32-bit positions
template <class C>
int plonk_sigma_wires_device(gm_ctx* ctx, const gm_plonk_wires* w, void* s1, void* s2, void* s3);
int plonk_pk_setup(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, unsigned flags, gm_plonk_pk** out,
                   void* vk_digests, void* srs_lagrange_out);
// plonk_pk_setup with the permutation taken from w (in->permutation is NULL)
int plonk_pk_setup_wires(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, const gm_plonk_wires* w,
                         unsigned flags, gm_plonk_pk** out, void* vk_digests, void* srs_lagrange_out);
// plonk_pk_setup_wires from a resident circuit (plonk_scs.hip): its tables, its
// sizes and commitment rows, its selectors generated on the device
int plonk_pk_setup_scs(gm_ctx* ctx, const gm_plonk_scs* s, const void* srs_canonical, size_t srs_canonical_len,
                       unsigned flags, gm_plonk_pk** out, void* vk_digests, void* srs_lagrange_out);
}  // namespace gm
