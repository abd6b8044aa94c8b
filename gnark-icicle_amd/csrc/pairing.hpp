// Pairing-product checks and batched Groth16 verification on the device
// (include/gnark_mi355x.h "pairing-product checks").
#pragma once
#include "runtime.hpp"

namespace gm {

// pairs (Miller lanes) of one chunk of the streamed entries: a device-filling
// round of one wave per SIMD is 256 CUs x 4 x 64 = 2^16 lanes
constexpr size_t PAIRING_CHUNK_PAIRS = size_t(1) << 16;

// Queue on ctx->stream; instantiated per curve in pairing_<curve>.hip.
// f_dev[i] = the Miller value of (g1_dev[i], g2_dev[i]): n Fp12 values, twelve Fp
// each in gnark Montgomery form, gnark-crypto's E12 memory order.
template <class C>
int pairing_miller_launch(gm_ctx* ctx, const void* g1_dev, const void* g2_dev, size_t n, void* f_dev);
// out[j][t] = prod in[j][16 t .. min(cnt, 16 t + 16)), newcnt = ceil(cnt / 16) values per product
template <class C>
int pairing_reduce_launch(gm_ctx* ctx, const void* in_dev, size_t n_products, size_t cnt, size_t newcnt,
                          void* out_dev);
// ok_dev[j] = (f_dev[j]^(s (p^12 - 1) / r) == 1)
template <class C>
int pairing_final_launch(gm_ctx* ctx, const void* f_dev, size_t n, uint8_t* ok_dev);

// The Groth16 verification kernels (pairing_impl.hpp has their contracts).
struct G16VerifyDev {
  const void* proofs;   // m records {Ar, Bs, Krs}
  const void* publics;  // m x nb_in fr.Elements
  const void* vk_g1;    // -alpha, K[0..nb_k)
  const void* vk_g2;    // beta, -gamma, -delta
  size_t m, nb_in;
  void* chk_g1;         // 2m: Ar, Krs
  void* chk_g2;         // m: Bs
  uint8_t* st_g1;       // 2m classes
  uint8_t* st_g2;       // m classes
  void* terms;          // m x nb_in XYZZ, packed internal
  uint8_t* bad_input;   // m
  void* pair_g1;        // 4m
  void* pair_g2;        // 4m
  uint8_t* pre;         // m: 0, BAD_POINT or BAD_INPUT
};
template <class C>
int g16_verify_split_launch(gm_ctx* ctx, const G16VerifyDev& d);
template <class C>
int g16_verify_terms_launch(gm_ctx* ctx, const G16VerifyDev& d);
template <class C>
int g16_verify_assemble_launch(gm_ctx* ctx, const G16VerifyDev& d);
template <class C>
int g16_verify_status_launch(gm_ctx* ctx, const uint8_t* pre_dev, const uint8_t* ok_dev, size_t m,
                             uint8_t* status_dev);
// y <- -y of n gnark affine points, in place
template <class C, bool G2>
int points_negate_launch(gm_ctx* ctx, void* pts_dev, size_t n);

// bytes of one Fp12 value (0 for an unknown id)
size_t pairing_gt_bytes(int curve);

// The entries behind their refusals.
int pairing_check_device(gm_ctx* ctx, int curve, const void* g1_dev, const void* g2_dev, size_t n_products,
                         size_t k, uint8_t* ok_host);
int pairing_check_host(gm_ctx* ctx, int curve, const void* g1_host, const void* g2_host, size_t n_products,
                       size_t k, uint8_t* ok_host);

}  // namespace gm

struct gm_g16_vk {
  gm_ctx* ctx = nullptr;
  int curve = 0;
  size_t nb_k = 0;
  void* g1 = nullptr;  // -alpha, K[0..nb_k)
  void* g2 = nullptr;  // beta, -gamma, -delta
};

namespace gm {
int g16_vk_upload(gm_ctx* ctx, int curve, const gm_g16_vk_host* vk, gm_g16_vk** out);
int g16_verify_batch(gm_ctx* ctx, const gm_g16_vk* vk, const void* proofs_host, const void* publics_host, size_t m,
                     uint8_t* status_out, size_t* nb_ok);
}  // namespace gm
