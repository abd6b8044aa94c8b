#pragma once
// Pippenger bucket MSM on gfx950 -- replaces iciclegnark MsmOnDevice /
// MsmG2OnDevice (backend/groth16/bn254/icicle/icicle.go:302,315,332,355,382).
//
// Pipeline (one HIP stream, all state in HBM; msm_plan + msm_run below):
//   1. k_msm_digits / k_msm_s1_scatter   Montgomery -> canonical scalar, signed
//                       c-bit digits of all W windows; non-zero digits are
//                       partitioned into coarse bins (bucket >> F) -- pass 1 of a
//                       hand-written two-level counting sort (no library sort).
//   2. k_msm_s2_*       (msm_sort.hip) each coarse bin -> its buckets: sorted
//                       values (point index | sign << 31), the bucket start
//                       offsets and -- for plans a G2 kernel reads -- the sorted
//                       bucket keys, written directly.
//   3. k_msm_accum_seg  G1: one lane per piece of the plan's piece plan (buckets
//                       cut into ceil(len / T) pieces of nearly equal length,
//                       sorted by length; k_msm_pp_* in msm_sort.hip): lazily
//                       reduced XYZZ mixed adds of the gathered points (sign
//                       applied on load), one store; the parts of a cut bucket lie
//                       in contiguous slots and are merged by k_msm_fixup
//                       (k_msm_fix_tree + k_msm_fixup_long above FIX_SERIAL adds).
//                       G2: slices of K sorted entries per lane pair, buckets cut
//                       by slice edges in part_first / part_last (pair_fp2.hpp).
//                       Buckets and parts are stored as the lazy add leaves them,
//                       each once ("Storage contract" at LazyAcc): at the 2^20
//                       bench shape 51,930 VALU instructions per wave against
//                       55,793 with a canonical emit inside the loop, 146 MB
//                       written against 205 (profiles/raw_bucket_emit_pmc.txt).
//   4. k_msm_seg        bucket reduction level 1: running sums over segments of
//                       L buckets;  k_msm_bitsum: LDS bit-sum trees up to one node
//                       per window;  k_msm_export: nodes -> gnark words.
//   5. host: Horner over the window / bit-position nodes, XYZZ -> Jacobian.
// With a precomputed point set (MsmPrecomp) every window shares one bucket set
// and steps 4-5 run once.
//
// Exact group arithmetic: the result is independent of summation order.
#include "curves.hpp"
#include "msm.hpp"
#include "pair_fp2.hpp"
#include "runtime.hpp"

#include <hip/hip_ext.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace gm {

// ---------------------------------------------------------------------------
// scalar digits
// ---------------------------------------------------------------------------
template <class Fr>
GM_DEV uint32_t window_bits(const FeG<Fr>& k, uint32_t bit, uint32_t mask) {
  const uint32_t idx = bit >> 5, sh = bit & 31;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < Fr::NG; i++) {
    lo = (idx == (uint32_t)i) ? k.w[i] : lo;
    hi = (idx + 1 == (uint32_t)i) ? k.w[i] : hi;
  }
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  return (uint32_t)(v >> sh) & mask;
}

// gnark Montgomery fr.Element -> canonical integer as packed u32 words
template <class Fr>
GM_DEV FeG<Fr> load_scalar_canonical(const uint32_t* __restrict__ s, uint32_t i) {
  return fe_pack(fe_gnark_to_canonical(fe_load_g<Fr>(s, i)));
}

// Plain layout: bucket b = w*nb + |d|-1 (window-major), entry value = point
// index | sign << 31.  Precomputed (shared-bucket) layout: b = |d|-1 for every
// window, value = w*stride + i (the shifted copy) | sign << 31.
// Windows 0..wn-1 are c bits wide, windows wn..W-1 (the `narrow` windows) c - 1
// bits, with c W - narrow = bits + 1: no window is left with only the few top
// bits of the scalar (precomputed layouts, msm.hpp MsmPrecomp, and plain
// non-GLV layouts; a plain 2^24 BN254 MSM at c = 20 has 8 windows of 20 bits
// and 5 of 19 instead of a 15-bit top window whose 2^14 buckets hold ~1024
// points each -- spans of 16 slices that need the tree fixup).
struct DigitGeom {
  uint32_t n, c, W, nb, shared_stride, F;  // F: pass-1 bin = b >> F
  uint32_t wn;
};
// bit offset and width of window w
GM_HD void window_geom(uint32_t c, uint32_t wn, uint32_t w, uint32_t& off, uint32_t& cw) {
  off = w * c - (w > wn ? w - wn : 0u);
  cw = w >= wn ? c - 1 : c;
}

// ---------------------------------------------------------------------------
// Bucket sort of the digits: a two-level counting sort written for this job.
// Order inside a bucket is irrelevant (group addition is exact), so no pass has
// to be stable, and zero digits are dropped at the source.
//   k_msm_digits     (here, per scalar field) one thread per point: the W
//                    signed digits, stored window-major (coalesced) as
//                    dig[w*n + i] = (|d|-1) | sign << 31 (~0: zero digit), and
//                    the coarse histogram (bin H = bucket >> F; LDS, then one
//                    global atomic per bin per block)
//   msm_sort.hip     k_msm_s1_scan: coarse bases; k_msm_s1_scatter: one block
//                    per (window, 8K points) partitions those digits into the
//                    coarse bins (a plain-layout block only touches its own
//                    window's bins, so its write runs are long); pass 2 sorts
//                    every coarse bin into its 2^F buckets and writes the
//                    sorted values, the bucket offsets and (G2 plans) the keys
//                    directly.  Between the passes an entry is one 32-bit word
//                    (low key bits, index, sign) when that fits, else 8 bytes
//                    (SortGeom::compact, msm.hpp).
// ---------------------------------------------------------------------------
constexpr uint32_t DG_THREADS = 1024, DG_PPT = 4;

template <class Fr>
__global__ void __launch_bounds__(1024) k_msm_digits(const uint32_t* __restrict__ scalars, DigitGeom g,
                                                     uint32_t NC, uint32_t* __restrict__ dig,
                                                     uint32_t* __restrict__ ccount) {
  extern __shared__ uint32_t dg_lds[];
  const uint32_t t = threadIdx.x;
  for (uint32_t q = t; q < NC; q += DG_THREADS) dg_lds[q] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * DG_THREADS * DG_PPT;
  for (uint32_t r = 0; r < DG_PPT; r++) {
    const uint32_t i = base + r * DG_THREADS + t;
    if (i >= g.n) break;
    const FeG<Fr> k = load_scalar_canonical<Fr>(scalars, i);
    uint32_t carry = 0;
    for (uint32_t w = 0; w < g.W; w++) {
      uint32_t off, cw;
      window_geom(g.c, g.wn, w, off, cw);
      const uint32_t raw = window_bits(k, off, (1u << cw) - 1) + carry;
      uint32_t d, neg;
      if (raw > (1u << (cw - 1))) {
        d = (1u << cw) - raw;
        carry = 1;
        neg = 1;
      } else {
        d = raw;
        carry = 0;
        neg = 0;
      }
      dig[(size_t)w * g.n + i] = d ? (d - 1) | (neg << 31) : 0xffffffffu;
      if (d) atomicAdd(&dg_lds[(g.shared_stride ? d - 1 : w * g.nb + d - 1) >> g.F], 1u);
    }
  }
  __syncthreads();
  for (uint32_t q = t; q < NC; q += DG_THREADS)
    if (dg_lds[q]) atomicAdd(&ccount[q], dg_lds[q]);
}

// ---------------------------------------------------------------------------
// GLV split for BN254 G1: phi(x, y) = (beta x, y) = [lambda] P with beta, lambda
// primitive cube roots of unity (p resp. r).  Short lattice basis of
// {(a, b) : a + b lambda = 0 mod r}: v1 = (a1, b1), v2 = (a2, b2) with
// a1 = b2 - |b1| ~ 2^126.8, b1 = -a2, a2 ~ 2^63.1.  c1 = floor(k g1 / 2^384),
// c2 = floor(k g2 / 2^384) with g1 = floor(2^384 b2 / r), g2 = floor(2^384 |b1| / r)
// undershoot b2 k / r and |b1| k / r by e1, e2 in [0, 1 + 2^-130), so
// k1 = k - c1 a1 - c2 a2 = e1 a1 + e2 a2 lies in [0, 2^127) and
// k2 = c1 |b1| - c2 b2 = -(e1 |b1|) + e2 b2 in (-2^127, 2^127): both are exact
// in 128-bit wrap-around arithmetic.  Constants derived by
// tools/glv_constants.py (checked there against the oracle's group law).
// ---------------------------------------------------------------------------
struct GlvBn254 {
  GM_HD static constexpr uint64_t g1(int i) {
    constexpr uint64_t a[5] = {0x163b4843cb4b9a5eull, 0x149d540fd5e495ccull, 0x5398fd0300ff6565ull,
                               0x4ccef014a773d2d2ull, 0x0000000000000002ull};
    return a[i];
  }
  GM_HD static constexpr uint64_t g2(int i) {
    constexpr uint64_t a[4] = {0x8fa7d32d2fafba64ull, 0x6eb9c714773a6ef2ull, 0xd91d232ec7e0b3d7ull,
                               0x0000000000000002ull};
    return a[i];
  }
  static constexpr uint64_t A1_LO = 0x8211bbeb7d4f1128ull, A1_HI = 0x6f4d8248eeb859fcull;
  static constexpr uint64_t A2 = 0x89d3256894d213e3ull;  // = |b1|
  static constexpr uint64_t B2_LO = 0x0be4e1541221250bull, B2_HI = 0x6f4d8248eeb859fdull;
  // beta in the internal radix-2^29 Montgomery form (beta * 2^261 mod p)
  GM_HD static constexpr uint32_t beta29(int i) {
    constexpr uint32_t a[9] = {0x18ccb791u, 0x175b1c3au, 0x0b83d6e2u, 0x0e8ed071u, 0x1282bee2u,
                               0x04220e84u, 0x1fe4017fu, 0x15084d4au, 0x00169119u};
    return a[i];
  }
  // G2 (the twist y^2 = x^3 + b' over Fp2): (x, y) -> (beta^2 x, y) is [lambda] on
  // the r-torsion (the other cube root of unity of Fp; tools/glv_constants.py)
  GM_HD static constexpr uint32_t beta29_g2(int i) {
    constexpr uint32_t a[9] = {0x0a337995u, 0x158d1d23u, 0x189c9b98u, 0x12fa4e45u, 0x185faadcu,
                               0x0176f16du, 0x0eed93bau, 0x14291140u, 0x000c0afeu};
    return a[i];
  }
};

// ---------------------------------------------------------------------------
// GLV split for BLS12-377: lambda = x^2 - 1 (x = 0x8508c00000000001, the curve
// seed) is a cube root of unity mod r with lambda^2 < r < (lambda + 1)^2, so
// k = k1 + k2 lambda with k2 = floor(k / lambda), k1 = k mod lambda -- both in
// [0, 2^127), no signs.  q = floor(k g / 2^384), g = floor(2^384 / lambda),
// undershoots k / lambda by less than one: one conditional correction.
// phi(x, y) = (beta x, y) on G1, (beta^2 x, y) on the G2 twist (tools/glv_constants.py
// checks both against the oracle's group law).
// ---------------------------------------------------------------------------
struct GlvBls377 {
  GM_HD static constexpr uint64_t g(int i) {
    constexpr uint64_t a[5] = {0x5cc5a03b7b820d29ull, 0x3366fc876f25c6b5ull, 0x7f72ed32af90182cull,
                               0xb3f7aa969fd37160ull, 0x0000000000000003ull};
    return a[i];
  }
  static constexpr uint64_t LAM_LO = 0x0a11800000000000ull, LAM_HI = 0x452217cc90000001ull;
  GM_HD static constexpr uint32_t beta29(int i) {
    constexpr uint32_t a[14] = {0x1c8a7893u, 0x0b7d08f2u, 0x06b88506u, 0x162aa2edu, 0x1c5fdf80u,
                                0x11b95a22u, 0x03b86dd7u, 0x1191f770u, 0x10701220u, 0x1501c11fu,
                                0x1cee88bbu, 0x118d05ecu, 0x06f2fa26u, 0x00000000u};
    return a[i];
  }
  GM_HD static constexpr uint32_t beta29_g2(int i) {
    constexpr uint32_t a[14] = {0x098a903fu, 0x0deef70eu, 0x0bd62e43u, 0x12fc3bfau, 0x0de940feu,
                                0x047b8e82u, 0x17ec1b27u, 0x1a776815u, 0x120a67b5u, 0x0a70d0c4u,
                                0x0271dc9au, 0x182f7308u, 0x19602487u, 0x00000000u};
    return a[i];
  }
};

// ---------------------------------------------------------------------------
// GLV split for BLS12-381: lambda = x^2 - 1 (x = -0xd201000000010000, the curve
// seed) is a cube root of unity mod r = lambda^2 + lambda + 1, but lambda ~
// 2^127.43: the halves of BLS12-377's unsigned division split (up to lambda) do
// not fit the GLV_HALF_BITS = 127 bits the digit geometry covers.  The split is
// signed and balanced instead: k > (r - 1) / 2 becomes r - k with both halves
// negated; then k2 = round(k / lambda), k1 = k - k2 lambda, so |k1| <=
// (lambda - 1) / 2 and 0 <= k2 <= (lambda + 1) / 2 + 1, both below 2^126.44, and
// the window count at c = 16 stays 8.  q = floor(k g / 2^384), g = floor(2^384 /
// lambda), is floor(k / lambda), or one less when lambda divides k, so
// r0 = k - q lambda lies in [0, lambda]: exact mod 2^128.
// phi(x, y) = (beta x, y) on G1, (beta^2 x, y) on the G2 twist.  Constants and
// the split's model (200,000 scalars and the special ones): tools/glv_constants.py.
// ---------------------------------------------------------------------------
struct GlvBls381 {
  GM_HD static constexpr uint64_t g(int i) {
    constexpr uint64_t a[5] = {0xda5e4f8d896c72ddull, 0x389f49a7268bf7a3ull, 0x63f6e522f6cfee30ull,
                               0x7c6becf1e01faaddull, 0x0000000000000001ull};
    return a[i];
  }
  static constexpr uint64_t LAM_LO = 0x00000000ffffffffull, LAM_HI = 0xac45a4010001a402ull;
  GM_HD static constexpr uint64_t r(int i) {
    constexpr uint64_t a[4] = GM_BLS12381_FR_P64;
    return a[i];
  }
  // (r - 1) / 2: scalars above it are split as r - k
  GM_HD static constexpr uint64_t half(int i) {
    constexpr uint64_t a[4] = {0x7fffffff80000000ull, 0xa9ded2017fff2dffull, 0x199cec0404d0ec02ull,
                               0x39f6d3a994cebea4ull};
    return a[i];
  }
  // largest half: k2 <= (lambda + 1) / 2 + 1 (|k1| <= (lambda - 1) / 2 is smaller)
  static constexpr unsigned __int128 MAX_HALF =
      ((((unsigned __int128)LAM_HI << 64) | LAM_LO) + 1) / 2 + 1;
  static_assert(MAX_HALF < ((unsigned __int128)1 << GLV_HALF_BITS),
                "the halves of the balanced split must fit the digits of a GLV plan");
  GM_HD static constexpr uint32_t beta29(int i) {
    constexpr uint32_t a[14] = {0x1195dfebu, 0x1b04e484u, 0x06026044u, 0x086070a2u, 0x1fd68858u,
                                0x137e9670u, 0x06871e67u, 0x1e736664u, 0x083b24f6u, 0x08a70373u,
                                0x02a012fdu, 0x0112f94bu, 0x18a2733cu, 0x00000003u};
    return a[i];
  }
  GM_HD static constexpr uint32_t beta29_g2(int i) {
    constexpr uint32_t a[14] = {0x0abf79e7u, 0x194b14ebu, 0x1ceb16a6u, 0x1845cd5du, 0x0c814568u,
                                0x199ca109u, 0x13ee6ee1u, 0x05d123e5u, 0x0dfbdce2u, 0x010ecb54u,
                                0x0d9337edu, 0x1daaf4b0u, 0x146806fbu, 0x0000000cu};
    return a[i];
  }
};

// beta of phi per base field: g1 for G1 points, g2 (= beta^2) for the G2 twist
template <class P>
struct GlvBeta;
template <>
struct GlvBeta<Bn254Fp> {
  GM_HD static constexpr uint32_t g1(int i) { return GlvBn254::beta29(i); }
  GM_HD static constexpr uint32_t g2(int i) { return GlvBn254::beta29_g2(i); }
};
template <>
struct GlvBeta<Bls377Fp> {
  GM_HD static constexpr uint32_t g1(int i) { return GlvBls377::beta29(i); }
  GM_HD static constexpr uint32_t g2(int i) { return GlvBls377::beta29_g2(i); }
};
template <>
struct GlvBeta<Bls381Fp> {
  GM_HD static constexpr uint32_t g1(int i) { return GlvBls381::beta29(i); }
  GM_HD static constexpr uint32_t g2(int i) { return GlvBls381::beta29_g2(i); }
};

// x -> beta x of the GLV endomorphism, G1 (Fp) and G2 (Fp2, beta in Fp)
template <class P>
GM_DEV Fe<P> glv_phi_x(const Fe<P>& x) {
  Fe<P> b;
#pragma unroll
  for (int j = 0; j < P::N; j++) b.v[j] = GlvBeta<P>::g1(j);
  return fe_mul(x, b);
}
template <class P, int B>
GM_DEV Fe2<P, B> glv_phi_x(const Fe2<P, B>& x) {
  Fe<P> b;
#pragma unroll
  for (int j = 0; j < P::N; j++) b.v[j] = GlvBeta<P>::g2(j);
  return {fe_mul(x.a0, b), fe_mul(x.a1, b)};
}

// floor(k * G / 2^384) for a 256-bit k and a G of NG 64-bit limbs (< 2^128 here)
template <int NG, class GF>
GM_DEV unsigned __int128 glv_mulshift(const uint64_t (&k)[4], GF g) {
  uint64_t t[4 + NG] = {};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < NG; j++) {
      const unsigned __int128 v = (unsigned __int128)k[i] * g(j) + t[i + j] + carry;
      t[i + j] = (uint64_t)v;
      carry = (uint64_t)(v >> 64);
    }
    t[i + NG] = carry;
  }
  return ((unsigned __int128)t[7] << 64) | t[6];
}

// one scalar's signed digits, written at dig[w * g.n + i]; flip: negate them
template <class Fr>
GM_DEV void emit_digits(const FeG<Fr>& k, uint32_t flip, uint32_t i, const DigitGeom& g, uint32_t* __restrict__ dig,
                        uint32_t* lds) {
  const uint32_t mask = (1u << g.c) - 1;
  uint32_t carry = 0;
  for (uint32_t w = 0; w < g.W; w++) {
    const uint32_t raw = window_bits(k, w * g.c, mask) + carry;
    uint32_t d, neg;
    if (raw > g.nb) {
      d = (1u << g.c) - raw;
      carry = 1;
      neg = 1;
    } else {
      d = raw;
      carry = 0;
      neg = 0;
    }
    dig[(size_t)w * g.n + i] = d ? (d - 1) | ((neg ^ flip) << 31) : 0xffffffffu;
    if (d) atomicAdd(&lds[(w * g.nb + d - 1) >> g.F], 1u);
  }
}

// Scalar split k = k1 + k2 lambda per curve: k1 in [0, 2^127), |k2| < 2^127,
// neg2 = sign of k2 (BLS12-377: always 0).  signed_k1 (BLS12-381): k1 carries a
// sign too, |k1| < 2^127, and split takes neg1.  2^127 is 2^GLV_HALF_BITS (msm.hpp).
template <class C>
struct Glv {
  static constexpr bool ok = false;
  static constexpr bool signed_k1 = false;
};
template <>
struct Glv<CurveBN254> {
  static constexpr bool ok = true;
  static constexpr bool signed_k1 = false;
  using U = unsigned __int128;
  GM_DEV static void split(const uint64_t (&k64)[4], U& k1, U& k2, uint32_t& neg2) {
    const U c1 = glv_mulshift<5>(k64, GlvBn254::g1);
    const U c2 = glv_mulshift<4>(k64, GlvBn254::g2);
    const U a1 = ((U)GlvBn254::A1_HI << 64) | GlvBn254::A1_LO;
    const U b2 = ((U)GlvBn254::B2_HI << 64) | GlvBn254::B2_LO;
    const U klo = ((U)k64[1] << 64) | k64[0];
    k1 = klo - c1 * a1 - c2 * (U)GlvBn254::A2;  // in [0, 2^127)
    k2 = c1 * (U)GlvBn254::A2 - c2 * b2;        // signed, |k2| < 2^127
    neg2 = (uint32_t)(k2 >> 127);
    if (neg2) k2 = (U)0 - k2;
  }
};
template <>
struct Glv<CurveBLS12377> {
  static constexpr bool ok = true;
  static constexpr bool signed_k1 = false;
  using U = unsigned __int128;
  GM_DEV static void split(const uint64_t (&k64)[4], U& k1, U& k2, uint32_t& neg2) {
    U q = glv_mulshift<5>(k64, GlvBls377::g);  // floor(k / lambda) or one less
    const U lam = ((U)GlvBls377::LAM_HI << 64) | GlvBls377::LAM_LO;
    const U klo = ((U)k64[1] << 64) | k64[0];
    U r = klo - q * lam;  // true value in [0, 2 lambda): exact mod 2^128
    if (r >= lam) {
      r -= lam;
      q += 1;
    }
    k1 = r;
    k2 = q;
    neg2 = 0;
  }
};

template <>
struct Glv<CurveBLS12381> {
  static constexpr bool ok = true;
  static constexpr bool signed_k1 = true;
  using U = unsigned __int128;
  GM_DEV static void split(const uint64_t (&k64)[4], U& k1, uint32_t& neg1, U& k2, uint32_t& neg2) {
    // flip = k > (r - 1) / 2: the borrow of (r - 1) / 2 - k; then kk = r - k
    uint64_t kk[4], borrow = 0, b2 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const U d = (U)GlvBls381::half(i) - k64[i] - borrow;
      borrow = (uint64_t)(d >> 127) & 1;
      const U e = (U)GlvBls381::r(i) - k64[i] - b2;
      b2 = (uint64_t)(e >> 127) & 1;
      kk[i] = (uint64_t)e;
    }
    const uint32_t flip = (uint32_t)borrow;
#pragma unroll
    for (int i = 0; i < 4; i++) kk[i] = flip ? kk[i] : k64[i];
    U q = glv_mulshift<5>(kk, GlvBls381::g);  // floor(kk / lambda), or one less when lambda | kk
    const U lam = ((U)GlvBls381::LAM_HI << 64) | GlvBls381::LAM_LO;
    const U klo = ((U)kk[1] << 64) | kk[0];
    U r0 = klo - q * lam;  // true value in [0, lambda]: exact mod 2^128
    neg1 = 0;
    if (r0 > (lam >> 1)) {  // round to nearest: k1 = r0 - lambda
      r0 = lam - r0;
      q += 1;
      neg1 = 1;
    }
    k1 = r0;
    k2 = q;
    neg1 ^= flip;
    neg2 = flip;
  }
};

// k_msm_digits for the GLV split (plain layout): thread i writes the digits of
// k1 at virtual point i and of k2 at virtual point n0 + i (g.n = 2 n0).
template <class C>
__global__ void __launch_bounds__(1024) k_msm_digits_glv(const uint32_t* __restrict__ scalars, DigitGeom g,
                                                         uint32_t n0, uint32_t NC, uint32_t* __restrict__ dig,
                                                         uint32_t* __restrict__ ccount) {
  using Fr = typename C::Fr;
  extern __shared__ uint32_t dg_lds[];
  const uint32_t t = threadIdx.x;
  for (uint32_t q = t; q < NC; q += DG_THREADS) dg_lds[q] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * DG_THREADS * DG_PPT;
  for (uint32_t r = 0; r < DG_PPT; r++) {
    const uint32_t i = base + r * DG_THREADS + t;
    if (i >= n0) break;
    const FeG<Fr> k = load_scalar_canonical<Fr>(scalars, i);
    uint64_t k64[4];
#pragma unroll
    for (int j = 0; j < 4; j++) k64[j] = (uint64_t)k.w[2 * j] | ((uint64_t)k.w[2 * j + 1] << 32);
    unsigned __int128 k1, k2;
    uint32_t neg1 = 0, neg2;
    if constexpr (Glv<C>::signed_k1) Glv<C>::split(k64, k1, neg1, k2, neg2);
    else Glv<C>::split(k64, k1, k2, neg2);
    FeG<Fr> m1, m2;
#pragma unroll
    for (int j = 0; j < Fr::NG; j++) {
      m1.w[j] = j < 4 ? (uint32_t)(k1 >> (32 * j)) : 0u;
      m2.w[j] = j < 4 ? (uint32_t)(k2 >> (32 * j)) : 0u;
    }
    emit_digits<Fr>(m1, neg1, i, g, dig, dg_lds);
    emit_digits<Fr>(m2, neg2, n0 + i, g, dig, dg_lds);
  }
  __syncthreads();
  for (uint32_t q = t; q < NC; q += DG_THREADS)
    if (dg_lds[q]) atomicAdd(&ccount[q], dg_lds[q]);
}

// gnark-layout points -> internal layout (GLV: plus phi(P_i) = (beta x, y) at
// n + i; G2: beta^2 on the twist), with coalesced HBM traffic: a block stages its 256 points
// through LDS (16-B lane loads / stores over contiguous bytes) and converts
// from there, instead of each lane reading and writing 64 B at a 64-B lane
// stride.  GLV: the phi copy goes out through the same LDS tile.  LDS rows are
// padded by 16 B (point stride Q + 1 uint4) against bank conflicts.
template <class F, bool GLV>
__global__ void __launch_bounds__(256) k_msm_convert_points_lds(const uint32_t* __restrict__ src, size_t n,
                                                                uint32_t* __restrict__ dst) {
  constexpr int PW = 2 * Coord<F>::WORDS;
  constexpr uint32_t Q = PW / 4;  // uint4 per point
  static_assert(PW % 4 == 0, "points are whole uint4s");
  __shared__ uint4 tile[256 * (Q + 1)];
  const size_t b0 = (size_t)blockIdx.x * 256;
  const uint32_t np = (uint32_t)min((size_t)256, n - b0);
  const uint32_t t = threadIdx.x;
  const uint4* s = reinterpret_cast<const uint4*>(src) + b0 * Q;
  for (uint32_t q = t; q < np * Q; q += 256) tile[(q / Q) * (Q + 1) + q % Q] = s[q];
  __syncthreads();
  uint32_t* mine = reinterpret_cast<uint32_t*>(tile + t * (Q + 1));
  Affine<F> a;
  if (t < np) {
    a = load_affine_gnark<F>(mine);
    store_affine_packed<F>(mine, a);
  }
  __syncthreads();
  uint4* d = reinterpret_cast<uint4*>(dst) + b0 * Q;
  for (uint32_t q = t; q < np * Q; q += 256) d[q] = tile[(q / Q) * (Q + 1) + q % Q];
  if constexpr (GLV) {
    __syncthreads();
    if (t < np) {
      a.x = glv_phi_x(a.x);
      store_affine_packed<F>(mine, a);
    }
    __syncthreads();
    uint4* d2 = reinterpret_cast<uint4*>(dst) + (n + b0) * Q;
    for (uint32_t q = t; q < np * Q; q += 256) d2[q] = tile[(q / Q) * (Q + 1) + q % Q];
  }
}

// ---------------------------------------------------------------------------
// points: gnark layout -> internal layout (once per MSM, into workspace)
// ---------------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(256) k_msm_convert_points(const uint32_t* __restrict__ src, size_t n,
                                                            uint32_t* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int PW = 2 * Coord<F>::WORDS;
  store_affine_packed<F>(dst + i * PW, load_affine_gnark<F>(src + i * PW));
}

// Fixed-base copies: pts[w*stride + i] = [2^off(w)] pts[i] for w = 1..W-1
// (copy 0 already converted; off(w) = window_geom's offset, windows >= wn one
// bit narrower).  width(w-1) doublings per copy in XYZZ, then one Fermat
// inversion back to affine; one-time setup cost, like the pk upload itself.
template <class F>
__global__ void __launch_bounds__(128) k_msm_precompute(uint32_t* __restrict__ pts, size_t n, size_t stride,
                                                        uint32_t c, uint32_t W, uint32_t wn) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int PW = 2 * Coord<F>::WORDS;
  const Affine<F> P = load_affine_packed<F>(pts + i * PW);
  Affine<F> zero;
  zero.x = FOps<F>::zero();
  zero.y = FOps<F>::zero();
  if (aff_is_inf(P)) {
    for (uint32_t w = 1; w < W; w++) store_affine_packed<F>(pts + (w * stride + i) * PW, zero);
    return;
  }
  XYZZ<F> acc;
  acc.x = P.x;
  acc.y = P.y;
  acc.zz = FOps<F>::one();
  acc.zzz = FOps<F>::one();
  for (uint32_t w = 1; w < W; w++) {
    const uint32_t cw = (w - 1 >= wn) ? c - 1 : c;
    for (uint32_t k = 0; k < cw; k++) acc = xyzz_dbl(acc);
    Affine<F> r = zero;
    if (!xyzz_is_inf(acc)) {
      const F t = fe_inv(fe_mul(acc.zz, acc.zzz));
      r.x = fe_mul(acc.x, fe_mul(t, acc.zzz));  // X / ZZ
      r.y = fe_mul(acc.y, fe_mul(t, acc.zz));   // Y / ZZZ
    }
    store_affine_packed<F>(pts + (w * stride + i) * PW, r);
  }
}

// raw words of one packed point (vector loads; unpacked just before use)
template <int PW>
struct PackedPt {
  uint32_t w[PW];
};
template <int PW>
GM_DEV PackedPt<PW> load_packed_pt(const uint32_t* __restrict__ src) {
  static_assert(PW % 4 == 0, "packed points are whole 16-byte chunks");
  PackedPt<PW> r;
#pragma unroll
  for (int q = 0; q < PW / 4; q++) {
    const uint4 v = reinterpret_cast<const uint4*>(src)[q];
    r.w[4 * q] = v.x;
    r.w[4 * q + 1] = v.y;
    r.w[4 * q + 2] = v.z;
    r.w[4 * q + 3] = v.w;
  }
  return r;
}

// Accumulation over the plan's pieces (MsmPlan, msm.hpp): lane t owns piece t,
// at most T consecutive sorted entries of ONE bucket.  A bucket that is a single
// piece is written straight to `buckets`; the pieces of a cut bucket go to its
// contiguous part slots and are merged by k_msm_fixup.  Every piece is at most T
// entries whatever the bucket, so skewed scalar distributions (one huge bucket)
// cost the same as uniform ones in this phase, and the pieces are sorted by
// length, so the lanes of a wave run the same number of adds.
//
// Storage contract of `buckets` and `parts` (G1, Fe<P>): the lazily reduced
// accumulator is stored as it stands, with no canonical pass --
//   x < 8p,  y < 2p,  zz < 2p,  zzz < 2p,  limbs normalised (the top limb keeps
//   the excess), infinity as xyzz_inf() (zz = 0 exactly).
// The fixup kernels store their sums under the same contract; xyzz_add_lz takes
// such operands (curve.hpp), and k_msm_seg makes its running sums canonical
// (xyzz_canon_raw) when it stores the nodes -- the first canonical pass of a
// bucket's life.  Every non-empty bucket is written exactly once by the
// accumulation (one piece) or by the fixup (cut buckets); empty buckets are
// never written and never read (k_msm_seg).
// G2 buckets (lane pairs, pair_fp2.hpp) stay on the slice grid -- thread t owns
// entries [t*K, t*K+K), buckets cut by slice edges go to part_first / part_last
// -- and are stored canonical: the raw emit there measured within noise
// (3.78-3.80 -> 3.77-3.80 ms at 2^20) and put the BN254 pair kernel, at its
// 168-VGPR cap, into scratch (profiles/raw_bucket_emit_ab.txt).
template <class F>
struct LazyAcc {
  static constexpr bool on = false;
  template <bool CH = false>
  GM_DEV static void add(XYZZ<F>& a, Affine<F> p, bool neg) {
    if (neg) p.y = fe_neg(p.y);
    xyzz_add_aff(a, p);
  }
};
template <class P>
struct LazyAcc<Fe<P>> {
  static constexpr bool on = true;
  template <bool CH = false>
  GM_DEV static void add(XYZZ<Fe<P>>& a, const Affine<Fe<P>>& p, bool neg) {
    // CH: strict mad chains (level 2) -- isolated 2^20 accumulation ~1 % faster than
    // per-column chains, bench line +1.7 % (profiles/r05an_strict_chain_ab.txt)
    xyzz_add_aff_lz<P, CH ? 2 : 0>(a, p, neg);
  }
};

// Profiled launches (ProfScope::wave_stamp): lane 0 of a wave stamps the wall
// clock on entry (atomicMin) and after the body, where the wave's lanes have
// reconverged (atomicMax): first wave start .. last wave end of the launch.  Blocks
// are dispatched in index order, so the entry stamps of the first 64 blocks hold the
// first wave; every wave stamps its end.  The pair is the block's (index mod 64,
// 256 B apart): one shared pair took every wave's atomics on one L2 channel, and
// the entry stamps of all waves arrive as one burst (bench -2 %, r06ae).
GM_DEV void wave_stamp_begin(unsigned long long* stamp) {
  if (stamp && blockIdx.x < 64 && (threadIdx.x & 63) == 0)
    atomicMin(stamp + blockIdx.x * 32, (unsigned long long)wall_clock64());
}
GM_DEV void wave_stamp_end(unsigned long long* stamp) {
  if (stamp && (threadIdx.x & 63) == 0)
    atomicMax(stamp + (blockIdx.x & 63) * 32 + 1, (unsigned long long)wall_clock64());
}

// Four consecutive entry values in one 16-byte load.  A piece starts at any
// entry, so the address is only 4-byte aligned; gfx950 takes a global dwordx4
// load at that alignment.
struct __attribute__((packed, aligned(4))) EntryQuad {
  uint32_t x, y, z, w;
};
GM_DEV uint4 load_entry_quad(const uint32_t* __restrict__ p) {
  const EntryQuad q = *reinterpret_cast<const EntryQuad*>(p);
  return make_uint4(q.x, q.y, q.z, q.w);
}

// Entry q -> q + 1 of a piece: shifts the value group, loads the next group at a
// group boundary (its latency overlaps entry q's add), bounds-checks entry
// q + 1 and, with PREFETCH, loads its point.  false: bad point index (err = 2).
template <int PW, bool PREFETCH>
GM_DEV bool accum_next(const uint32_t* __restrict__ points, uint32_t n, const uint32_t* __restrict__ vp,
                       uint32_t len, uint32_t q, uint4& vg, uint32_t& vn, PackedPt<PW>& Pn,
                       uint32_t* __restrict__ err) {
  if ((q & 3) == 3) {
    if (q + 1 < len) vg = load_entry_quad(vp + q + 1);
  } else {
    vg = make_uint4(vg.y, vg.z, vg.w, vg.w);
  }
  vn = vg.x;  // entry q + 1 (when q + 1 < len)
  if (q + 1 < len) {
    if ((vn & 0x7fffffffu) >= n) {
      atomicOr(err, 2u);
      return false;
    }
    if (PREFETCH) Pn = load_packed_pt<PW>(points + (size_t)(vn & 0x7fffffffu) * PW);
  }
  return true;
}

// G1 accumulation body: len lazy adds into an accumulator that starts at
// infinity, then ONE raw store.  Every lane of a wave is at the first entry of
// its piece in the same step, q = 0, so the copy branch of xyzz_add_aff_lz
// (fe_pminus for a negated entry; an infinity point leaves infinity) is taken by
// the whole wave there and the add is skipped (s_cbranch_execz); it stays
// inside the loop because hoisted in front of it the BN254 kernel needs 128
// VGPRs and 28 bytes of scratch against 120 and none.  No keys are read: the
// bucket is the descriptor's, which is read again for the store rather than
// held in a register.  Values arrive four entries per 16-byte load (r05: 4-byte
// loads touched one cache line per lane per entry).  Reads past the piece's last
// entry stay inside `vals`, which is allocated 16 bytes longer than its entries
// (msm_plan).  A wave whose lanes hold two length classes loops to its longest
// piece.
template <class F, bool CH, bool PREFETCH = false>
GM_DEV void accum_piece_body(const uint32_t* __restrict__ points, uint32_t n, const uint32_t* __restrict__ vals,
                             const uint4* __restrict__ pieces, const uint32_t* __restrict__ pcount,
                             XYZZ<F>* __restrict__ buckets, XYZZ<F>* __restrict__ parts,
                             uint32_t* __restrict__ err) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pcount[0]) return;
  const uint32_t* vp = vals + pieces[t].x;  // {first entry, length >= 1, destination, -}
  const uint32_t len = pieces[t].y;
  uint4 vg = load_entry_quad(vp);
  uint32_t v = vg.x;
  if ((v & 0x7fffffffu) >= n) {
    atomicOr(err, 2u);
    return;
  }
  constexpr int PW = 2 * Coord<F>::WORDS;  // u32 words per packed point
  PackedPt<PW> P, Pn;
  if (PREFETCH) P = load_packed_pt<PW>(points + (size_t)(v & 0x7fffffffu) * PW);
  XYZZ<F> acc = xyzz_inf<F>();
  for (uint32_t q = 0; q < len; q++) {
    uint32_t vn;
    if (!accum_next<PW, PREFETCH>(points, n, vp, len, q, vg, vn, Pn, err)) return;
    if (!PREFETCH) P = load_packed_pt<PW>(points + (size_t)(v & 0x7fffffffu) * PW);
    LazyAcc<F>::template add<CH>(acc, load_affine_packed<F>(P.w), (v >> 31) != 0);
    v = vn;
    if (PREFETCH) P = Pn;
  }
  const uint32_t dst = pieces[t].z;
  *((dst & PIECE_PART) ? parts + (dst & ~PIECE_PART) : buckets + dst) = acc;
}

// BN254 G1: one strict mad chain per product inside the add (r05; the split-
// column schedule measured slower, profiles/r05e_acc_chain_ab.txt,
// r05an_strict_chain_ab.txt), four waves per SIMD, no prefetch: the other waves
// hide the point loads (profiles/r03e_ab.txt).  Applied to every MSM kernel the
// chains slowed the one-to-two-wave reduction kernels (r04h, r05ax).
template <class F>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(4)))
k_msm_accum_seg_ch(const uint32_t* __restrict__ points, uint32_t n, const uint32_t* __restrict__ vals,
                   const uint4* __restrict__ pieces, const uint32_t* __restrict__ pcount,
                   XYZZ<F>* __restrict__ buckets, XYZZ<F>* __restrict__ parts, uint32_t* __restrict__ err,
                   unsigned long long* __restrict__ stamp) {
  wave_stamp_begin(stamp);
  accum_piece_body<F, true>(points, n, vals, pieces, pcount, buckets, parts, err);
  wave_stamp_end(stamp);
}
// Four waves fit the 9-limb fields only: BLS12-377's 14-limb add spills 216
// VGPRs under the cap and takes the prefetching kernel (two waves, no spill).
template <class F>
struct AccumW4 {
  static constexpr bool ok = false;
};
template <class P>
struct AccumW4<Fe<P>> {
  static constexpr bool ok = P::N <= 9;
};
// The next point prefetched into registers while the current add runs
// (BLS12-377 G1: two waves per SIMD).
template <class F>
__global__ void __launch_bounds__(128) k_msm_accum_seg_pf4(const uint32_t* __restrict__ points, uint32_t n,
                                                           const uint32_t* __restrict__ vals,
                                                           const uint4* __restrict__ pieces,
                                                           const uint32_t* __restrict__ pcount,
                                                           XYZZ<F>* __restrict__ buckets,
                                                           XYZZ<F>* __restrict__ parts,
                                                           uint32_t* __restrict__ err,
                                                           unsigned long long* __restrict__ stamp) {
  wave_stamp_begin(stamp);
  accum_piece_body<F, false, true>(points, n, vals, pieces, pcount, buckets, parts, err);
  wave_stamp_end(stamp);
}
// G1 accumulation kernel of a field
template <class F>
constexpr auto g1_accum_kernel() {
  if constexpr (AccumW4<F>::ok) return k_msm_accum_seg_ch<F>;
  else return k_msm_accum_seg_pf4<F>;
}

// G2: Fp2 components split across lane pairs (pair_fp2.hpp), keys / values in
// groups of four as in the G1 accumulation.
template <class F>
struct PairSel {
  static constexpr bool ok = false;
};
template <class P, int B>
struct PairSel<Fe2<P, B>> {
  static constexpr bool ok = true;
  // BN254: one mad chain per product in the pair add, no prefetch, three waves
  // per SIMD (168 VGPRs, no spill; the prefetching kernel needs 200 and runs
  // two): G2 2^20 accumulation 3.91-3.92 -> 3.86-3.89 ms, Groth16 2^24
  // 148.0-149.3 -> 146.8-147.8 ms (profiles/r05aj_pair_chain_ab.txt).
  // BLS12-377: no prefetch (its pair kernel spills at three waves with the
  // prefetch registers: 2^22 accumulation 46.1 -> 44.2 ms, profiles/r03i_ab.txt),
  // two waves (r04e_g2_ab.txt).
  static constexpr auto kernel() {
    if constexpr (P::N <= 9) return k_msm_accum_seg_pair<P, B, false, 3, true, true>;
    else return k_msm_accum_seg_pair<P, B, false, GM_PAIR_WPE, true>;
  }
  static constexpr auto fixup() { return k_msm_fixup_pair<P, B>; }
  static constexpr auto fixup_edge() { return k_msm_fixup_edge_pair<P, B>; }
  static constexpr auto fix_tree() { return k_msm_fix_tree_pair<P, B>; }
  static constexpr auto fixup_long() { return k_msm_fixup_long_pair<P, B>; }
  static constexpr auto seg() { return k_msm_seg_pair<P, B>; }
  static constexpr auto bitsum() { return k_msm_bitsum_pair<P, B>; }
};
// one-lane kernels are instantiated for G1 fields; G2 runs on lane pairs
template <class F>
constexpr bool kOneLane = !PairSel<F>::ok;

// Full adds of the fixup / reduction kernels: lazily reduced for G1
// (xyzz_add_lz), canonical xyzz_add otherwise.  A G1 sum is < 2p in every
// coordinate, or one of the operands unchanged when the other is infinity.  So:
//   the fixup kernels store sums of raw buckets / parts as they are (the
//     storage contract of the accumulation above holds for them);
//   canon   a sum whose operands may be raw (k_msm_seg: a segment with a single
//     non-empty bucket hands that bucket through): x < 8p;
//   canon2  a sum of canonical operands (k_msm_bitsum's nodes): < 2p.
template <class F>
struct FullAdd {
  GM_DEV static XYZZ<F> add(const XYZZ<F>& a, const XYZZ<F>& b) { return xyzz_add(a, b); }
  GM_DEV static XYZZ<F> canon(const XYZZ<F>& a) { return a; }
  GM_DEV static XYZZ<F> canon2(const XYZZ<F>& a) { return a; }
};
template <class P>
struct FullAdd<Fe<P>> {
  GM_DEV static XYZZ<Fe<P>> add(const XYZZ<Fe<P>>& a, const XYZZ<Fe<P>>& b) { return xyzz_add_lz(a, b); }
  GM_DEV static XYZZ<Fe<P>> canon(const XYZZ<Fe<P>>& a) { return xyzz_canon_raw(a); }
  GM_DEV static XYZZ<Fe<P>> canon2(const XYZZ<Fe<P>>& a) { return xyzz_canon2(a); }
};

// Merge the parts of the cut buckets (G1; the lane-pair kernels of G2 merge
// slice parts, pair_fp2.hpp).  Bucket b of len > T entries has p = ceil(len / T)
// parts in the contiguous slots parts[pbase[b] .. pbase[b] + p), and its sum is
// their sum in slot order.  Up to FIX_SERIAL adds (p - 1) are done by one thread;
// buckets with more parts (a huge bucket: skewed witness values, or the nearly
// empty top window of a scalar field much narrower than W*c bits) report
// p - 1 through `maxspan` and are tree-reduced in place over their slots by
// k_msm_fix_tree levels -- depth log2(p) adds instead of p serial ones.
constexpr uint32_t FIX_SERIAL = 8;

template <class F>
__global__ void __launch_bounds__(128) k_msm_fixup(const uint32_t* __restrict__ offsets, uint32_t total,
                                                   uint32_t T, XYZZ<F>* __restrict__ buckets,
                                                   const XYZZ<F>* __restrict__ parts,
                                                   const uint32_t* __restrict__ pbase,
                                                   uint32_t* __restrict__ maxspan) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= total) return;
  const uint32_t len = offsets[b + 1] - offsets[b];
  if (len <= T) return;  // empty, or written whole by the accumulation
  const uint32_t p = (len + T - 1) / T;
  if (p - 1 > FIX_SERIAL) {
    atomicMax(maxspan, p - 1);
    return;
  }
  const XYZZ<F>* q = parts + pbase[b];
  XYZZ<F> acc = q[0];
  for (uint32_t i = 1; i < p; i++) acc = FullAdd<F>::add(acc, q[i]);
  buckets[b] = acc;
}

// One level d of the pairwise tree over the part slots of every long bucket:
// one thread per slot (partb: the slot's bucket).
template <class F>
__global__ void __launch_bounds__(128) k_msm_fix_tree(const uint32_t* __restrict__ offsets, uint32_t T,
                                                      const uint32_t* __restrict__ pcount,
                                                      const uint32_t* __restrict__ pbase,
                                                      const uint32_t* __restrict__ partb, uint32_t d,
                                                      XYZZ<F>* __restrict__ parts) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= pcount[1]) return;
  const uint32_t b = partb[s];
  const uint32_t p = (offsets[b + 1] - offsets[b] + T - 1) / T;
  if (p - 1 <= FIX_SERIAL) return;
  const uint32_t rel = s - pbase[b], step = 1u << d;
  if ((rel & ((step << 1) - 1)) == 0 && rel + step < p) parts[s] = FullAdd<F>::add(parts[s], parts[s + step]);
}

// after the tree levels the first slot of a long bucket holds its sum
template <class F>
__global__ void __launch_bounds__(128) k_msm_fixup_long(const uint32_t* __restrict__ offsets, uint32_t total,
                                                        uint32_t T, XYZZ<F>* __restrict__ buckets,
                                                        const XYZZ<F>* __restrict__ parts,
                                                        const uint32_t* __restrict__ pbase) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= total) return;
  const uint32_t len = offsets[b + 1] - offsets[b];
  if (len <= T || (len + T - 1) / T - 1 <= FIX_SERIAL) return;
  buckets[b] = parts[pbase[b]];
}

// ---------------------------------------------------------------------------
// Bucket reduction: window sum P_w = sum_j (j+1) B_j over the nb buckets of a
// window.  A single EC add costs ~15-20 us of latency in one wave, so the
// reduction is organised to keep every serial chain short and all 1024 SIMDs
// busy, and to leave the inherently serial Horner tail (~W*c doublings) to the
// host, where one group op is ~50x cheaper in latency:
//
//   level 1 (k_msm_seg): segments of L buckets, running sums
//        S_s = sum_l B_{sL+l},  T_s = sum_l (l+1) B_{sL+l}
//     so P_w = sum_s T_s + L * sum_s s*S_s.
//   levels 2.. (k_msm_bitsum): LDS trees over the segments that never multiply
//     by the index: a node carries [G, U, Y_0..Y_{K-1}] with G = sum S, U = sum T
//     and Y_b = sum of S over the node's segments whose local index has bit b
//     set.  Merging two sibling nodes of 2^d segments is (K+3) independent adds
//     (Y_d of the parent is G of the right child), one per thread, so a tree
//     over NT segments has depth log2(NT) adds and ~3 adds of work per segment.
//   host: P_w = U + sum_b 2^(b + log2 L) Y_b, merged into the window Horner.
// ---------------------------------------------------------------------------
// node layout: per window, m nodes of Q = 2 + K XYZZ points [G, U, Y_0..Y_{K-1}]
// (tree levels and the BS_THREADS block: msm_tree_geom, msm.hpp)
// A bucket with no entries (offsets[b] == offsets[b + 1]) was never written by
// the accumulation or the fixup: it reads as infinity here, so the buckets need no
// clearing before the accumulation (a 1 GB memset per plain 2^24 MSM).
// Non-empty buckets arrive under the storage contract of the accumulation (raw,
// x < 8p); the running sums are made canonical when they are stored as nodes.
template <class F>
__global__ void __launch_bounds__(128) k_msm_seg(const XYZZ<F>* __restrict__ buckets,
                                                 const uint32_t* __restrict__ offsets, uint32_t nb, uint32_t L,
                                                 uint32_t nseg, uint32_t W, XYZZ<F>* __restrict__ nodes) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W * nseg) return;
  const uint32_t w = t / nseg, s = t % nseg;
  const size_t b0 = (size_t)w * nb + (size_t)s * L;
  const XYZZ<F>* B = buckets + b0;
  const uint32_t* O = offsets + b0;
  uint32_t o_hi = O[L];
  uint32_t o_lo = O[L - 1];
  XYZZ<F> S = o_lo == o_hi ? xyzz_inf<F>() : B[L - 1], T = S;
  for (int j = (int)L - 2; j >= 0; j--) {
    o_hi = o_lo;
    o_lo = O[j];
    S = FullAdd<F>::add(S, o_lo == o_hi ? xyzz_inf<F>() : B[j]);
    T = FullAdd<F>::add(T, S);
  }
  nodes[2 * (size_t)t] = FullAdd<F>::canon(S);
  nodes[2 * (size_t)t + 1] = FullAdd<F>::canon(T);
}

// One tree level group: block (w, j) merges nodes [j*NT, (j+1)*NT) of window w
// (Qin points each) into one node of Qin + log2(NT) points.
template <class F>
__global__ void __launch_bounds__(BS_THREADS) k_msm_bitsum(const XYZZ<F>* __restrict__ in, uint32_t m,
                                                    uint32_t Qin, uint32_t NT, uint32_t lgNT,
                                                    XYZZ<F>* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  XYZZ<F>* X = reinterpret_cast<XYZZ<F>*>(smem_raw);
  const uint32_t groups = m / NT;
  const uint32_t w = blockIdx.x / groups, j = blockIdx.x % groups;
  const XYZZ<F>* src = in + ((size_t)w * m + (size_t)j * NT) * Qin;
  for (uint32_t q = threadIdx.x; q < NT * Qin; q += blockDim.x) X[q] = src[q];
  __syncthreads();
  for (uint32_t d = 0; d < lgNT; d++) {
    const uint32_t qc = Qin + d + 1;           // quantities of a parent node
    const uint32_t tasks = (NT >> (d + 1)) * qc;
    const uint32_t child = (Qin << d);          // slots spanned by one child
    XYZZ<F> r0, r1;
    uint32_t s0 = 0xffffffffu, s1 = 0xffffffffu;
    {
      const uint32_t t = threadIdx.x;
      if (t < tasks) {
        const uint32_t p = t / qc, q = t % qc, base = p * 2 * child;
        r0 = (q + 1 < qc) ? FullAdd<F>::canon2(FullAdd<F>::add(X[base + q], X[base + child + q])) : X[base + child];
        s0 = base + q;
      }
    }
    {
      const uint32_t t = threadIdx.x + blockDim.x;
      if (t < tasks) {
        const uint32_t p = t / qc, q = t % qc, base = p * 2 * child;
        r1 = (q + 1 < qc) ? FullAdd<F>::canon2(FullAdd<F>::add(X[base + q], X[base + child + q])) : X[base + child];
        s1 = base + q;
      }
    }
    __syncthreads();
    if (s0 != 0xffffffffu) X[s0] = r0;
    if (s1 != 0xffffffffu) X[s1] = r1;
    __syncthreads();
  }
  const uint32_t Qout = Qin + lgNT;
  XYZZ<F>* dst = out + ((size_t)w * groups + j) * Qout;
  for (uint32_t q = threadIdx.x; q < Qout; q += blockDim.x) dst[q] = X[q];
}

// internal XYZZ -> gnark-layout (X, Y, ZZ, ZZZ) words for the host finish
template <class F>
__global__ void __launch_bounds__(128) k_msm_export(const XYZZ<F>* __restrict__ nodes, uint32_t count,
                                                    uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  uint32_t* o = out + (size_t)t * 4 * Coord<F>::WORDS;
  const XYZZ<F> r = nodes[t];
  Coord<F>::store_gnark(o, r.x);
  Coord<F>::store_gnark(o + Coord<F>::WORDS, r.y);
  Coord<F>::store_gnark(o + 2 * Coord<F>::WORDS, r.zz);
  Coord<F>::store_gnark(o + 3 * Coord<F>::WORDS, r.zzz);
}

// ---------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------
// (window choice and the plan's derived sizes: choose_window, msm_plan_geom, msm.hpp)
// Keys, sort and bucket offsets for one scalar vector (see MsmPlan).
template <class C>
int msm_plan(gm_ctx* ctx, Arena& arena, const void* scalars_dev, size_t n, const MsmPrecomp* pre,
             MsmPlan& plan, bool glv, bool pieces, bool keys) {
  hipStream_t st = ctx->stream;
  plan = MsmPlan();
  plan.n = n;
  plan.bits = C::FR_BITS;
  if (n == 0) return GM_OK;
  if (glv && (!Glv<C>::ok || (pre && pre->c))) {
    set_error("msm: the GLV split needs a plain (not precomputed) layout");
    return GM_ERR_INVALID;
  }
  const size_t n0 = n;  // scalars
  MsmPlanGeom pg;
  const char* refusal = msm_plan_geom(n0, C::FR_BITS, glv, pre, ctx->msm_c_override, pg);
  n = pg.n;  // GLV: the virtual points P_i and phi(P_i)
  plan.n = pg.n;
  plan.bits = pg.bits;
  plan.c = pg.c;
  plan.W = pg.W;
  plan.nb = pg.nb;
  plan.Wred = pg.Wred;
  plan.total = pg.total;
  plan.npts = pg.npts;
  plan.M = pg.M;
  if (refusal) {
    set_error(refusal);
    return GM_ERR_INVALID;
  }
  const bool shared = pre && pre->c;
  const uint32_t c = pg.c, W = pg.W;
  const size_t M = pg.M;
  const SortGeom& sg = pg.sg;
  int rc;
  DevBuf dig, keys_out, vals_out, offsets, scount;
  if ((rc = dig.alloc(arena, sizeof(uint32_t) * M)) || (keys && (rc = keys_out.alloc(arena, sizeof(uint32_t) * M))) ||
      (rc = vals_out.alloc(arena, sizeof(uint32_t) * M + 16)) ||  // + 16: accum_piece_body's group loads
      (rc = offsets.alloc(arena, sizeof(uint32_t) * ((size_t)plan.total + 1))) ||
      (rc = scount.alloc(arena, sizeof(uint32_t) * sg.NS)))
    return rc;
  DigitGeom g;
  g.n = (uint32_t)n;
  g.c = c;
  g.W = W;
  g.nb = plan.nb;
  g.shared_stride = shared ? (uint32_t)pre->stride : 0u;
  g.wn = pg.wn;
  plan.wn = g.wn;
  g.F = sg.F + sg.G;  // the digits kernel counts pass-1 bins
  {
    ProfScope ps(ctx, "msm_digits");
    GM_HIP(hipMemsetAsync(scount.p, 0, sizeof(uint32_t) * sg.NS, st));
    if constexpr (Glv<C>::ok) {
      if (glv)
        hipLaunchKernelGGL(k_msm_digits_glv<C>, dim3(blocks_for(n0, DG_THREADS * DG_PPT)), dim3(DG_THREADS),
                         sizeof(uint32_t) * sg.NS, st, reinterpret_cast<const uint32_t*>(scalars_dev), g,
                           (uint32_t)n0, sg.NS, dig.as<uint32_t>(), scount.as<uint32_t>());
    }
    if (!glv)
      hipLaunchKernelGGL(k_msm_digits<typename C::Fr>, dim3(blocks_for(n, DG_THREADS * DG_PPT)), dim3(DG_THREADS),
                         sizeof(uint32_t) * sg.NS, st, reinterpret_cast<const uint32_t*>(scalars_dev), g, sg.NS,
                         dig.as<uint32_t>(), scount.as<uint32_t>());
    GM_HIP(hipGetLastError());
  }
  {
    ProfScope ps(ctx, "msm_sort");
    // the entry width taken, as a counted name (no events of its own)
    if (ctx->profiling) ctx->stats[sg.compact ? "msm_sort_compact" : "msm_sort_wide"].count += 1;
    if ((rc = msm_sort_digits(ctx, arena, sg, n, W, plan.nb, g.shared_stride, dig.as<uint32_t>(),
                              scount.as<uint32_t>(), keys_out.as<uint32_t>(), vals_out.as<uint32_t>(),
                              offsets.as<uint32_t>())))
      return rc;
  }
  plan.keys = keys_out.as<uint32_t>();
  plan.vals = vals_out.as<uint32_t>();
  plan.offsets = offsets.as<uint32_t>();
  if (pieces) {
    ProfScope ps(ctx, "msm_piece_plan");
    if ((rc = msm_piece_plan(ctx, arena, plan, msm_piece_len(ctx, M)))) return rc;
  }
  return GM_OK;
}

// Bucket reduction of a launched MSM (k_msm_seg, LDS bit-sum levels, export
// into t.wsum); sets t.Q, the points per exported node.
template <class C, bool G2>
int msm_reduce(gm_ctx* ctx, MsmTail& t) {
  using DF = typename GroupSel<C, G2>::DF;
  hipStream_t st = ctx->stream;
  ProfScope ps(ctx, "msm_bucket_reduce");
  uint32_t Q = 2;  // points per node: [G, U, Y_0..Y_{Q-3}]
  constexpr bool pairs = PairSel<DF>::ok;
  if constexpr (PairSel<DF>::ok) {
    if (pairs)
      hipLaunchKernelGGL(PairSel<DF>::seg(), dim3(blocks_for(2 * (size_t)t.Wr * t.nseg, 128)), dim3(128), 0, st,
                         (const uint32_t*)t.buckets, (const uint32_t*)t.offsets, t.nb, t.L, t.nseg, t.Wr,
                         (uint32_t*)t.nodes_a);
  }
  if constexpr (kOneLane<DF>) {
    if (!pairs)
      hipLaunchKernelGGL(k_msm_seg<DF>, dim3(blocks_for((size_t)t.Wr * t.nseg, 128)), dim3(128), 0, st,
                         (const XYZZ<DF>*)t.buckets, (const uint32_t*)t.offsets, t.nb, t.L, t.nseg, t.Wr,
                         (XYZZ<DF>*)t.nodes_a);
  }
  // LDS tree levels until one node per window (msm_tree_geom, msm.hpp)
  MsmTreeGeom tg;
  if (!msm_tree_geom(t.nseg, sizeof(XYZZ<DF>), tg)) {
    set_error("msm: bucket reduction does not fit LDS");
    return GM_ERR_INVALID;
  }
  uint32_t m = t.nseg;
  XYZZ<DF>* cur = (XYZZ<DF>*)t.nodes_a;
  XYZZ<DF>* nxt = (XYZZ<DF>*)t.nodes_b;
  for (uint32_t lv = 0; lv < tg.levels; lv++) {
    const uint32_t lg = tg.lg[lv];
    const uint32_t NT = 1u << lg;
    const uint32_t groups = m / NT;
    if constexpr (PairSel<DF>::ok) {
      if (pairs)
        hipLaunchKernelGGL(PairSel<DF>::bitsum(), dim3(t.Wr * groups), dim3(BS_PAIR_THREADS), sizeof(XYZZ<DF>) * NT * Q,
                           st, (const uint32_t*)cur, m, Q, NT, lg, (uint32_t*)nxt);
    }
    if constexpr (kOneLane<DF>) {
      if (!pairs)
        hipLaunchKernelGGL(k_msm_bitsum<DF>, dim3(t.Wr * groups), dim3(BS_THREADS), sizeof(XYZZ<DF>) * NT * Q, st,
                           cur, m, Q, NT, lg, nxt);
    }
    Q += lg;
    m = groups;
    std::swap(cur, nxt);
  }
  hipLaunchKernelGGL(k_msm_export<DF>, dim3(blocks_for((size_t)t.Wr * Q, 128)), dim3(128), 0, st, cur, t.Wr * Q,
                     (uint32_t*)t.wsum);
  GM_HIP(hipGetLastError());
  t.Q = Q;
  return GM_OK;
}

// Buckets spanning more than FIX_SERIAL slices: tree fixup over part_first.
template <class C, bool G2>
int msm_fix_long(gm_ctx* ctx, MsmTail& t, uint32_t maxspan) {
  using DF = typename GroupSel<C, G2>::DF;
  hipStream_t st = ctx->stream;
  if constexpr (PairSel<DF>::ok) {
    {
      const size_t nslices = (t.M + t.K - 1) / t.K;
      for (uint32_t d = 0; (1u << d) < maxspan; d++)
        hipLaunchKernelGGL(PairSel<DF>::fix_tree(), dim3(blocks_for(2 * nslices, 128)), dim3(128), 0, st, t.keys,
                           t.offsets, t.total, t.K, (uint32_t)nslices, d, (uint32_t*)t.pfirst, FIX_SERIAL);
      hipLaunchKernelGGL(PairSel<DF>::fixup_long(), dim3(blocks_for(2 * (size_t)t.total, 128)), dim3(128), 0, st,
                         t.offsets, t.total, t.K, (uint32_t*)t.buckets, (const uint32_t*)t.pfirst,
                         (const uint32_t*)t.plast, FIX_SERIAL);
      GM_HIP(hipGetLastError());
      return GM_OK;
    }
  }
  if constexpr (kOneLane<DF>) {  // maxspan = parts - 1 of the longest bucket
    for (uint32_t d = 0; (1u << d) <= maxspan; d++)
      hipLaunchKernelGGL(k_msm_fix_tree<DF>, dim3(blocks_for(t.max_parts, 128)), dim3(128), 0, st, t.offsets, t.T,
                         t.pcount, t.pbase, t.partb, d, (XYZZ<DF>*)t.pfirst);
    hipLaunchKernelGGL(k_msm_fixup_long<DF>, dim3(blocks_for(t.total, 128)), dim3(128), 0, st, t.offsets, t.total,
                       t.T, (XYZZ<DF>*)t.buckets, (const XYZZ<DF>*)t.pfirst, t.pbase);
  }
  GM_HIP(hipGetLastError());
  return GM_OK;
}

// readback of (error, max span) and the exported nodes into t.stage, event after it
template <class C, bool G2>
int msm_readback(gm_ctx* ctx, MsmTail& t) {
  using DF = typename GroupSel<C, G2>::DF;
  constexpr int WORDS = Coord<DF>::WORDS;
  hipStream_t st = ctx->stream;
  const size_t wbytes = sizeof(uint32_t) * 4 * WORDS * t.Wr * t.Q;
  if (!t.stage) {  // a re-readback (after a long-span fixup) reuses the tail's buffer
    if (int r = tail_pinned_acquire(ctx, 16 + wbytes, &t.stage, &t.stage_idx)) return r;
    t.stage_ctx = ctx;
  }
  GM_HIP(hipMemcpyAsync(t.stage, t.errw, 16, hipMemcpyDeviceToHost, st));
  GM_HIP(hipMemcpyAsync(t.stage + 16, t.wsum, wbytes, hipMemcpyDeviceToHost, st));
  if (!t.done) GM_HIP(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  GM_HIP(hipEventRecord(t.done, st));
  return GM_OK;
}

// Bucket accumulation and (speculative) reduction over a plan, queued on the
// context's stream; msm_finish completes it.
template <class C, bool G2>
int msm_launch(gm_ctx* ctx, Arena& arena, const MsmPlan& plan, const void* points_internal, MsmTail& t) {
  using DF = typename GroupSel<C, G2>::DF;
  using HF = typename GroupSel<C, G2>::HF;
  hipStream_t st = ctx->stream;
  t.n = plan.n;
  if (plan.n == 0) return GM_OK;
  t.c = plan.c;
  t.W = plan.W;
  t.wn = plan.wn;
  t.nb = plan.nb;
  t.total = plan.total;
  t.Wr = plan.Wred;
  t.M = plan.M;
  t.keys = plan.keys;
  t.offsets = plan.offsets;
  // level-1 segment length (buckets) and segments per window: msm_seg_geom, msm.hpp
  msm_seg_geom(t.Wr, t.nb, t.L, t.nseg);
  // G2: entries per accumulation lane pair (slice length), 64; K % 4 == 0 (keys /
  // values arrive four entries per load), and the long-span bound FIX_SERIAL * K
  // stays above the fullest uniform bucket.  (128 for the Groth16 2^24 MSMs:
  // within noise, profiles/r06d_g16_k128_ab.txt.)  G1 runs on the plan's pieces of
  // at most T entries instead (MsmPlan; T from msm_piece_len, sweep in
  // profiles/piece_plan_ab.txt; the slice grid's K = 24 / 32 / 64 sweeps for G1 are
  // in r04ae_slice_sweep.txt and r06ai_slice_ab.txt).
  t.K = 64u;
  if (!G2) {
    if (!plan.T || !plan.pieces) {
      set_error("msm: the plan has no piece plan (built for G2 only)");
      return GM_ERR_INVALID;
    }
    t.T = plan.T;
    t.max_parts = plan.max_parts;
    t.pcount = plan.pcount;
    t.pbase = plan.pbase;
    t.partb = plan.partb;
  } else if (!plan.keys) {
    set_error("msm: the plan has no sorted keys (built for G1 only)");
    return GM_ERR_INVALID;
  }
  int rc;
  constexpr int WORDS = Coord<DF>::WORDS;  // u32 words of one gnark-layout coordinate
  static_assert(sizeof(HF) == 4 * WORDS, "host/device layout mismatch");
  // part buffers: G2 one part_first / part_last per slice; G1 the cut buckets'
  // part slots (in pfirst)
  const size_t nslices = G2 ? (t.M + t.K - 1) / t.K : plan.max_parts;
  DevBuf buckets, nodes_a, nodes_b, wsum, errw, pfirst, plast;
  if ((rc = errw.alloc(arena, 16)) || (rc = buckets.alloc(arena, sizeof(XYZZ<DF>) * (size_t)t.total)) ||
      (rc = nodes_a.alloc(arena, sizeof(XYZZ<DF>) * 2 * (size_t)t.Wr * t.nseg)) ||
      (rc = nodes_b.alloc(arena, sizeof(XYZZ<DF>) * 2 * (size_t)t.Wr * t.nseg)) ||
      (rc = wsum.alloc(arena, sizeof(uint32_t) * 4 * WORDS * t.Wr * (2 + t.c))) ||
      (rc = pfirst.alloc(arena, sizeof(XYZZ<DF>) * nslices)) ||
      (rc = plast.alloc(arena, G2 ? sizeof(XYZZ<DF>) * nslices : 16)))
    return rc;
  t.buckets = buckets.p;
  t.nodes_a = nodes_a.p;
  t.nodes_b = nodes_b.p;
  t.wsum = wsum.p;
  t.errw = errw.p;
  t.pfirst = pfirst.p;
  t.plast = plast.p;
  GM_HIP(hipMemsetAsync(errw.p, 0, 16, st));
  {
    // async MSMs: this accumulation starts after the previous one (gm_ctx::acc_tail)
    if (ctx->acc_chain) {
      if (!ctx->acc_tail) GM_HIP(hipEventCreateWithFlags(&ctx->acc_tail, hipEventDisableTiming));
      else GM_HIP(hipStreamWaitEvent(st, ctx->acc_tail, 0));
    }
    struct TailMark {  // recorded once the accumulation is queued
      gm_ctx* c;
      hipStream_t s;
      ~TailMark() {
        if (c->acc_chain) hipEventRecord(c->acc_tail, s);
      }
    } tail_mark{ctx, st};
    ProfScope ps(ctx, G2 ? "msm_accum_g2" : "msm_accum_g1", true);  // stamped by the launch
    if constexpr (PairSel<DF>::ok) {
      hipExtLaunchKernelGGL(PairSel<DF>::kernel(), dim3(blocks_for(2 * nslices, 128)), dim3(128), 0, st, ps.a, ps.b,
                            0, reinterpret_cast<const uint32_t*>(points_internal), (uint32_t)plan.npts, plan.keys,
                            plan.vals, plan.offsets, t.total, t.K, buckets.as<uint32_t>(), pfirst.as<uint32_t>(),
                            plast.as<uint32_t>(), errw.as<uint32_t>());
    } else {
      hipExtLaunchKernelGGL(g1_accum_kernel<DF>(), dim3(blocks_for(plan.max_pieces, 128)), dim3(128), 0, st, ps.a,
                            ps.b, 0, reinterpret_cast<const uint32_t*>(points_internal), (uint32_t)plan.npts,
                            plan.vals, plan.pieces, plan.pcount, buckets.as<XYZZ<DF>>(), pfirst.as<XYZZ<DF>>(),
                            errw.as<uint32_t>(), ps.wave_stamp("msm_accum_g1_exec"));
    }
  }
  {
    ProfScope ps(ctx, "msm_fixup");
    if constexpr (PairSel<DF>::ok) {
      if (plan.M < (size_t)t.K * t.total) {  // buckets shorter than a slice: per edge (pair_fp2.hpp)
        if (nslices > 1)
          hipLaunchKernelGGL(PairSel<DF>::fixup_edge(), dim3(blocks_for(2 * (nslices - 1), 128)), dim3(128), 0, st,
                             plan.keys, plan.offsets, t.total, t.K, (uint32_t)nslices, buckets.as<uint32_t>(),
                             pfirst.as<uint32_t>(), plast.as<uint32_t>(), errw.as<uint32_t>() + 1, FIX_SERIAL);
      } else {
        hipLaunchKernelGGL(PairSel<DF>::fixup(), dim3(blocks_for(2 * (size_t)t.total, 128)), dim3(128), 0, st,
                           plan.offsets, t.total, t.K, buckets.as<uint32_t>(), pfirst.as<uint32_t>(),
                           plast.as<uint32_t>(), errw.as<uint32_t>() + 1, FIX_SERIAL);
      }
    } else if (plan.M > t.T) {  // no bucket can be cut otherwise
      hipLaunchKernelGGL(k_msm_fixup<DF>, dim3(blocks_for(t.total, 128)), dim3(128), 0, st, plan.offsets, t.total,
                         t.T, buckets.as<XYZZ<DF>>(), pfirst.as<XYZZ<DF>>(), plan.pbase, errw.as<uint32_t>() + 1);
    }
  }
  // Bucket reduction, launched speculatively: buckets spanning more than
  // FIX_SERIAL slices (G1: of more than FIX_SERIAL + 1 parts; skewed scalars) are only known once errw[1] (max span)
  // reaches the host, so the reduction is queued right away and redone after the
  // long-span fixup in that (rare) case.  Speculate only when uniform scalars
  // would give no long span: the fullest bucket is then a top-window digit
  // (n / 2^top_bits entries; plus the other windows' share when buckets are
  // shared).  Large MSMs whose top window is narrow (2^24: 1024-4096 entries per
  // top digit) sync on the max span first.
  {
    // expected entries of the fullest bucket: bucket 0 gets n / h_w from window
    // w, h_w = the largest digit of w (its width, or the bits left above it)
    double fullest = 0;
    for (uint32_t w = 0; w < t.W; w++) {
      uint32_t off, cw;
      window_geom(t.c, plan.wn, w, off, cw);
      const int left = plan.bits - (int)off;
      const double h = std::ldexp(1.0, std::max(0, std::min((int)cw - 1, left)));
      const double load = (double)plan.n / h;
      fullest = t.Wr == 1 ? fullest + load : std::max(fullest, load);
    }
    if (fullest > 0.5 * FIX_SERIAL * (G2 ? t.K : t.T)) {
      uint8_t* pb;
      int pbi;
      if ((rc = tail_pinned_acquire(ctx, 16, &pb, &pbi))) return rc;
      const hipError_t e1 = hipMemcpyAsync(pb, errw.p, 16, hipMemcpyDeviceToHost, st);
      const hipError_t e2 = e1 == hipSuccess ? hipStreamSynchronize(st) : e1;
      uint32_t ms;
      memcpy(&ms, pb + 4, 4);
      tail_pinned_release(ctx, pbi);
      GM_HIP(e2);
      if (ms > FIX_SERIAL) {
        if ((rc = msm_fix_long<C, G2>(ctx, t, ms))) return rc;
        GM_HIP(hipMemsetAsync(errw.as<uint32_t>() + 1, 0, 4, st));  // long spans resolved
      }
    }
  }
  if ((rc = msm_reduce<C, G2>(ctx, t))) return rc;
  return msm_readback<C, G2>(ctx, t);
}

// Host tail of a launched MSM: waits for its readback (not for the stream),
// redoes the reduction after a tree fixup if a long span showed up, then the
// host Horner over the window / bit-position nodes.
template <class C, bool G2>
int msm_finish(gm_ctx* ctx, MsmTail& t, typename GroupSel<C, G2>::HF (&jac_out)[3]) {
  using HF = typename GroupSel<C, G2>::HF;
  using HJ = host::Jac<HF>;
  if (t.n == 0) {
    HJ inf = HJ::inf();
    jac_out[0] = inf.x;
    jac_out[1] = inf.y;
    jac_out[2] = inf.z;
    return GM_OK;
  }
  int rc;
  GM_HIP(hipEventSynchronize(t.done));
  uint32_t herr, maxspan;
  memcpy(&herr, t.stage, 4);
  memcpy(&maxspan, t.stage + 4, 4);
  if (maxspan > FIX_SERIAL) {
    if ((rc = msm_fix_long<C, G2>(ctx, t, maxspan)) || (rc = msm_reduce<C, G2>(ctx, t)) ||
        (rc = msm_readback<C, G2>(ctx, t)))
      return rc;
    GM_HIP(hipEventSynchronize(t.done));
    memcpy(&herr, t.stage, 4);
  }
  if (herr) {
    set_error("msm: internal consistency check failed (code " + std::to_string(herr) + ")");
    return GM_ERR_DEVICE;
  }
  const uint32_t Wr = t.Wr, Q = t.Q, c = t.c;
  std::vector<HF> hw(4 * (size_t)Wr * Q);
  memcpy(hw.data(), t.stage + 16, sizeof(HF) * hw.size());
  t.release_stage();  // the buffer may serve the next readback
  // Host Horner over bit positions: window w (bit offset off_w, window_geom)
  // contributes U_w at 2^off_w and Y_{w,b} at 2^(off_w + log2 L + b)
  // (b < Q - 2 = log2(nseg), log2 L + log2 nseg = c - 1, so every exponent
  // stays below the next window's offset).  Shared buckets: one window, w = 0.
  uint32_t lgL = 0;
  while ((1u << lgL) < t.L) lgL++;
  const int top = (int)(c * Wr);
  std::vector<std::vector<uint32_t>> at(top + 1);  // point ids per exponent
  for (uint32_t w = 0; w < Wr; w++) {
    uint32_t off, cw;
    window_geom(c, Wr == 1 ? 1u : t.wn, w, off, cw);
    at[off].push_back(w * Q + 1);
    for (uint32_t b = 0; b + 2 < Q; b++) at[off + lgL + b].push_back(w * Q + 2 + b);
  }
  HJ acc = HJ::inf();
  for (int e = top; e >= 0; e--) {
    if (!acc.is_inf()) acc = host::jdbl(acc);
    for (uint32_t id : at[e]) {
      const HF* p = &hw[4 * (size_t)id];
      if (p[2].is_zero()) continue;
      acc = host::jadd(acc, host::xyzz_to_jac(p[0], p[1], p[2], p[3]));
    }
  }
  jac_out[0] = acc.x;
  jac_out[1] = acc.y;
  jac_out[2] = acc.z;
  return GM_OK;
}

template <class C, bool G2>
int msm_run(gm_ctx* ctx, const MsmPlan& plan, const void* points_internal,
            typename GroupSel<C, G2>::HF (&jac_out)[3]) {
  Arena arena(ctx);
  MsmTail t;
  int rc = msm_launch<C, G2>(ctx, arena, plan, points_internal, t);
  return rc ? rc : msm_finish<C, G2>(ctx, t, jac_out);
}

template <class C, bool G2>
int msm_device_launch(gm_ctx* ctx, Arena& arena, const void* scalars_dev, const void* points_dev, size_t n,
                      bool points_internal, const MsmPrecomp* pre, MsmTail& t, hipEvent_t inputs_read) {
  using DF = typename GroupSel<C, G2>::DF;
  int rc;
  const void* pts = points_dev;
  DevBuf ipts;
  bool glv = false;
  if (!points_internal && n) {
    if (pre && pre->c) {
      set_error("msm: a precomputed point set must be device-internal");
      return GM_ERR_INVALID;
    }
    glv = Glv<C>::ok && msm_glv_on(ctx, G2, n);
    if ((rc = ipts.alloc(arena, 2 * Coord<DF>::WORDS * sizeof(uint32_t) * n * (glv ? 2 : 1)))) return rc;
    ProfScope ps(ctx, "msm_convert_points");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(points_dev);
    if (glv)
      hipLaunchKernelGGL((k_msm_convert_points_lds<DF, true>), dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream,
                         src, n, ipts.as<uint32_t>());
    else
      hipLaunchKernelGGL((k_msm_convert_points_lds<DF, false>), dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream,
                         src, n, ipts.as<uint32_t>());
    pts = ipts.p;
  }
  MsmPlan plan;
  if ((rc = msm_plan<C>(ctx, arena, scalars_dev, n, pre, plan, glv, !G2, G2))) return rc;
  // the caller's scalars (digits) and gnark-layout points (conversion) are not
  // read past this point
  if (inputs_read) GM_HIP(hipEventRecord(inputs_read, ctx->stream));
  return msm_launch<C, G2>(ctx, arena, plan, pts, t);
}

template <class C, bool G2>
int msm_device(gm_ctx* ctx, const void* scalars_dev, const void* points_dev, size_t n,
               typename GroupSel<C, G2>::HF (&jac_out)[3], bool points_internal, const MsmPrecomp* pre) {
  Arena arena(ctx);
  MsmTail t;
  int rc = msm_device_launch<C, G2>(ctx, arena, scalars_dev, points_dev, n, points_internal, pre, t);
  return rc ? rc : msm_finish<C, G2>(ctx, t, jac_out);
}

template <class C, bool G2>
size_t msm_internal_point_bytes() {
  return 2 * Coord<typename GroupSel<C, G2>::DF>::WORDS * sizeof(uint32_t);
}

template <class C, bool G2>
int msm_prepare_points(gm_ctx* ctx, const void* gnark_points, size_t n, void* dst) {
  using DF = typename GroupSel<C, G2>::DF;
  if (n == 0) return GM_OK;
  hipLaunchKernelGGL(k_msm_convert_points<DF>, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<const uint32_t*>(gnark_points), n, reinterpret_cast<uint32_t*>(dst));
  GM_HIP(hipGetLastError());
  return GM_OK;
}

template <class C, bool G2>
int msm_precompute_points(gm_ctx* ctx, const void* gnark_points, size_t n, const MsmPrecomp& pre, void* dst) {
  using DF = typename GroupSel<C, G2>::DF;
  if (n == 0) return GM_OK;
  if (pre.stride < n || pre.W == 0 || pre.c == 0) {
    set_error("msm precompute: bad layout");
    return GM_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_msm_convert_points<DF>, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<const uint32_t*>(gnark_points), n, reinterpret_cast<uint32_t*>(dst));
  if (pre.W > 1)
    hipLaunchKernelGGL(k_msm_precompute<DF>, dim3(blocks_for(n, 128)), dim3(128), 0, ctx->stream,
                       reinterpret_cast<uint32_t*>(dst), n, pre.stride, pre.c, pre.W, pre.W - pre.narrow);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

// Explicit instantiation for one (curve, group); each lives in its own
// translation unit (msm_<curve>_<group>.hip) so the four compile in parallel.
// The scalar-only plan is instantiated with the G1 unit.
#define GM_MSM_INSTANTIATE(C, G2)                                                              \
  template size_t msm_internal_point_bytes<C, G2>();                                          \
  template int msm_prepare_points<C, G2>(gm_ctx*, const void*, size_t, void*);                \
  template int msm_precompute_points<C, G2>(gm_ctx*, const void*, size_t, const MsmPrecomp&, void*); \
  template int msm_run<C, G2>(gm_ctx*, const MsmPlan&, const void*, typename GroupSel<C, G2>::HF (&)[3]); \
  template int msm_launch<C, G2>(gm_ctx*, Arena&, const MsmPlan&, const void*, MsmTail&);      \
  template int msm_finish<C, G2>(gm_ctx*, MsmTail&, typename GroupSel<C, G2>::HF (&)[3]);     \
  template int msm_device_launch<C, G2>(gm_ctx*, Arena&, const void*, const void*, size_t, bool, \
                                        const MsmPrecomp*, MsmTail&, hipEvent_t);              \
  template int msm_device<C, G2>(gm_ctx*, const void*, const void*, size_t,                    \
                                 typename GroupSel<C, G2>::HF (&)[3], bool, const MsmPrecomp*);
#define GM_MSM_INSTANTIATE_PLAN(C) \
  template int msm_plan<C>(gm_ctx*, Arena&, const void*, size_t, const MsmPrecomp*, MsmPlan&, bool, bool, bool);

}  // namespace gm
