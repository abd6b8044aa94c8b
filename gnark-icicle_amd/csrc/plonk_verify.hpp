// Batched KZG and PLONK verification on the device (DESIGN.md section 3.12;
// include/gnark_mi355x.h "KZG and PLONK verification").  The pairing itself is
// pairing.hpp's: these units add the verifier's Fr arithmetic, the linear
// combination of G1 points per proof and the fold into a product of two pairs.
#pragma once
#include "pairing.hpp"

namespace gm {

// ladder lanes of one chunk of the streamed entries (as gm_g16_verify_batch)
constexpr size_t PV_CHUNK_LADDERS = size_t(1) << 20;
// elements of the batch inversion's prefix products of one chunk (36 or 40 bytes each)
constexpr size_t PV_CHUNK_PREFIX = size_t(1) << 22;

// Points of one proof, in the order of the entry: L, R, O, Z, H0, H1, H2, Hb, Hz, Bsb22[j].
constexpr size_t PV_PROOF_POINTS = 9;
constexpr size_t PV_HZ = 8;
// The key's G1 array: G, Ql, Qr, Qm, Qo, S3, S1, S2, Qcp[j], then Qk (scalar 1, no ladder).
constexpr size_t PV_KEY_LADDERS = 8;
// The key's Fr array (gnark form): 1 / n, w, 1 / w, the coset shift, then w^row[j].
constexpr size_t PV_KEY_FR = 4;

constexpr size_t pv_proof_points(size_t nb_bsb) { return PV_PROOF_POINTS + nb_bsb; }
constexpr size_t pv_values(size_t nb_bsb) { return 7 + nb_bsb; }
// ladders of one proof: the key's, the proof's, and [u] Hz of the second pair
constexpr size_t pv_terms(size_t nb_bsb) { return PV_KEY_LADDERS + nb_bsb + PV_PROOF_POINTS + nb_bsb + 1; }

// The device arrays of one chunk of m proofs (plonk_verify_impl.hpp has the kernels' contracts).
struct PvDev {
  const void* points;    // m x (9 + nb_bsb) gnark G1Affine
  const void* values;    // m x (7 + nb_bsb) Fr
  const void* publics;   // m x nb_public Fr
  const void* hashed;    // m x nb_bsb Fr
  const void* chal;      // m x 6 Fr: gamma, beta, alpha, zeta, v, u
  const void* key_g1;    // 9 + nb_bsb points
  const void* key_g2;    // G2[0], -G2[1]
  const void* key_fr;    // 4 + nb_bsb Fr
  size_t m, nb_public, nb_bsb;
  uint32_t logn;
  const uint8_t* st_g1;  // m x (9 + nb_bsb) point classes, or NULL (the scalars alone)
  void* prefix;          // (nb_public + nb_bsb + 1) x m Fr, internal limbs
  void* scal;            // m x pv_terms Fr, gnark form
  void* aux;             // m x 2 Fr, gnark form: PI(zeta), constLin
  uint8_t* pre;          // m: 0, BAD_POINT, BAD_INPUT or ALGEBRAIC
  void* terms;           // m x pv_terms XYZZ, packed internal
  void* pair_g1;         // 2m: A, B
  void* pair_g2;         // 2m: G2[0], -G2[1]
};
template <class C>
int pv_scalars_launch(gm_ctx* ctx, const PvDev& d);
template <class C>
int pv_terms_launch(gm_ctx* ctx, const PvDev& d);
template <class C>
int pv_assemble_launch(gm_ctx* ctx, const PvDev& d);

// One chunk of m KZG openings.  Per opening: two ladders and the pairs
// (C - [y] G + [z] H, G2[0]) (H, -G2[1]).  Folded: four ladders per opening with the
// caller's lambda, the partial sums (A_i, B_i) as XYZZ in part[1 + i], then the sum
// over the chunk and the carry of the chunks before (part[0]).
struct KzgvDev {
  const void* digests;   // m gnark G1Affine
  const void* proofs;    // m
  const void* z;         // m Fr
  const void* y;         // m Fr
  const void* lambda;    // m Fr (folded)
  const void* key_g1;    // G
  const void* key_g2;    // G2[0], -G2[1]
  size_t m;
  int first;             // folded: opening 0 of this chunk is the batch's opening 0 (lambda = 1)
  const uint8_t* st_c;   // m point classes
  const uint8_t* st_h;   // m
  uint8_t* bad_input;    // m, zeroed by the host
  void* terms;           // m x 2 (or 4) XYZZ
  uint8_t* pre;          // m
  void* pair_g1;         // 2m (folded: 2)
  void* pair_g2;         // 2m (folded: 2)
  void* part;            // folded: (1 + m) x 2 XYZZ
};
template <class C>
int kzgv_terms_launch(gm_ctx* ctx, const KzgvDev& d, bool fold);
template <class C>
int kzgv_assemble_launch(gm_ctx* ctx, const KzgvDev& d, bool fold);
// out[t] = sum in[16 t .. min(cnt, 16 t + 16)): pairs of XYZZ, both halves summed
template <class C>
int kzgv_sum_launch(gm_ctx* ctx, const void* in_dev, size_t cnt, size_t newcnt, void* out_dev);
// the folded sums (A, B) to the two pairs of the product
template <class C>
int kzgv_fold_pairs_launch(gm_ctx* ctx, const void* sum_dev, const void* key_g2, void* pair_g1, void* pair_g2);

}  // namespace gm

struct gm_kzg_vk {
  gm_ctx* ctx = nullptr;
  int curve = 0;
  void* g1 = nullptr;  // G
  void* g2 = nullptr;  // G2[0], -G2[1]
};

struct gm_plonk_vk {
  gm_ctx* ctx = nullptr;
  int curve = 0;
  size_t n = 0, nb_public = 0, nb_bsb = 0;
  uint32_t logn = 0;
  void* g1 = nullptr;  // G, Ql, Qr, Qm, Qo, S3, S1, S2, Qcp[j], Qk
  void* g2 = nullptr;  // G2[0], -G2[1]
  void* fr = nullptr;  // 1 / n, w, 1 / w, g, w^row[j]
};

namespace gm {
int kzg_vk_upload(gm_ctx* ctx, int curve, const gm_kzg_vk_host* in, gm_kzg_vk** out);
void kzg_vk_release(gm_kzg_vk* vk);
// openings per chunk of the KZG entries for this m
size_t kzg_verify_chunk(size_t m, bool fold);
// the chunk loop: `per` whole openings per chunk (the entries pass kzg_verify_chunk's)
int kzg_verify_batch(gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* in, size_t m, size_t per, bool fold,
                     uint8_t* status_out, size_t* nb_ok);
int plonk_vk_upload(gm_ctx* ctx, int curve, const gm_plonk_vk_host* in, gm_plonk_vk** out);
void plonk_vk_release(gm_plonk_vk* vk);
// proofs per chunk of gm_plonk_verify_batch for this key and m
size_t plonk_verify_chunk(const gm_plonk_vk* vk, size_t m);
// the chunk loop: `per` whole proofs per chunk (the entry passes plonk_verify_chunk's)
int plonk_verify_run(gm_ctx* ctx, const gm_plonk_vk* vk, const gm_plonk_proofs_host* in, size_t m, size_t per,
                     uint8_t* status_out, size_t* nb_ok);
// the workspace and uploads of one chunk up to the scalars kernel (the entry and the test hook)
size_t pv_prefix_bytes(int curve);
}  // namespace gm
