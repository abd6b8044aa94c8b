// Element-wise test hooks for the device field / curve layer (used by the
// parity tests to pin each arithmetic primitive against the oracle).  Not on
// the proving path.
#include <chrono>
#include <initializer_list>
#include <vector>

#include "curves.hpp"
#include "field_sqrt.hpp"
#include "msm.hpp"
#include "pair_fp2.hpp"
#include "runtime.hpp"
#include "scan.hpp"
#include "../../include/gnark_mi355x_testhooks.h"

namespace gm {

// gnark-layout element i -> internal, and back
template <class F>
struct ElemIO {
  GM_DEV static F load(const uint8_t* p, size_t i) {
    return Coord<F>::load_internal(reinterpret_cast<const uint32_t*>(p) + i * Coord<F>::WORDS);
  }
  GM_DEV static void store(uint8_t* p, size_t i, const F& v) {
    Coord<F>::store_gnark(reinterpret_cast<uint32_t*>(p) + i * Coord<F>::WORDS, v);
  }
};

template <class F>
__global__ void k_field_op(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F x = ElemIO<F>::load(a, i), y = ElemIO<F>::load(b, i), r;
  switch (op) {
    case 0: r = fe_mul(x, y); break;
    case 1: r = fe_add(x, y); break;
    case 2: r = fe_sub(x, y); break;
    case 3: r = fe_neg(x); break;
    case 4: r = fe_inv(x); break;
    case 5: r = fe_sqr(x); break;
    default: r = x; break;
  }
  ElemIO<F>::store(out, i, r);
}

template <class F>
GM_DEV Affine<F> to_affine_dev(const XYZZ<F>& a) {
  Affine<F> r;
  if (xyzz_is_inf(a)) {
    r.x = FOps<F>::zero();
    r.y = FOps<F>::zero();
    return r;
  }
  F t = fe_inv(fe_mul(a.zz, a.zzz));
  r.x = fe_mul(a.x, fe_mul(t, a.zzz));
  r.y = fe_mul(a.y, fe_mul(t, a.zz));
  return r;
}

template <class F>
GM_DEV XYZZ<F> from_affine_dev(const Affine<F>& p) {
  XYZZ<F> r = xyzz_inf<F>();
  xyzz_add_aff(r, p);
  return r;
}

template <class F>
__global__ void k_point_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int PW = 2 * Coord<F>::WORDS;
  Affine<F> p = load_affine_gnark<F>(a + i * PW), q = load_affine_gnark<F>(b + i * PW);
  XYZZ<F> r;
  switch (op) {
    case 0: r = from_affine_dev(p); xyzz_add_aff(r, q); break;          // mixed add
    case 1: r = xyzz_dbl(from_affine_dev(p)); break;                      // double
    case 2: r = xyzz_add(from_affine_dev(p), from_affine_dev(q)); break;  // full add
    case 3: r = xyzz_mul_small(from_affine_dev(p), 1000003u); break;      // small scalar mul
    default: r = from_affine_dev(p); break;
  }
  store_affine_gnark<F>(out + i * PW, to_affine_dev(r));
}

// ---------------------------------------------------------------------------
// Raw-limb hooks (gm_test_field_raw_op / gm_test_point_raw_op): internal limbs
// in and out, as they are.
//
// Template constants, as the library instantiates them (raw_field_valid is the
// one list; everything else is GM_ERR_INVALID):
//   fe_sub_lz<K>      Fr 2, 4, 8, 16, 32 (ntt.hip butterflies, B and 2B of the
//                     growing rounds); Fp 1, 2, 4 (pf2_sqr<IN>), 8 (G1 mixed add),
//                     10, 20 (fe2_mul_lz / fe2_sqr_lz<4>, BETA = -5)
//   fe_sub2x_lz<K>    Fp 6 (X3 of the mixed adds)
//   fe_sub_cf<K>      Fr 3, 5, 9, 17 (ntt.hip: 3, 5, B + 1, 2B + 1); Fp 9 (BN254
//                     G1 mixed add; N <= 11)
//   fe_negk_cf<K>     Fp 3 (xyzz_add_lz), 5 (G1 mixed add, pf2_mul)
//   cneg2p + sub_lz<K> Fp 4 (G1 mixed add), 2 (lane-pair mixed add)
//   fe_reduce_k<K>    Fr 1, 2, 4, 8, 16 (ntt.hip, plonk_lin.hip); Fp 1, 2, 4, 8
//   fe_canon<L>       1..4
//   fe_to2p<M>        Fp 4, 6, 8, 10, 12
//   fe_is_zero_lz<K>  Fp 4, 6, 10
//   fe2_sqr_lz<IN>    4;  pf2_sqr<IN>  1, 2, 4
//   chain             0, 1, 2 for the one-lane products; 0, 1 (CH false / true)
//                     for the lane-pair ones
// ---------------------------------------------------------------------------
template <class P>
GM_DEV Fe<P> raw_load(const uint32_t* p, size_t idx) {
  Fe<P> r;
#pragma unroll
  for (int k = 0; k < P::N; k++) r.v[k] = p ? p[idx * P::N + k] : 0u;
  return r;
}
template <class P>
GM_DEV void raw_store(uint32_t* p, size_t idx, const Fe<P>& a) {
#pragma unroll
  for (int k = 0; k < P::N; k++) p[idx * P::N + k] = a.v[k];
}

#define RAW_K(K, ...) \
  case K: {           \
    __VA_ARGS__;      \
  } break;

// scalar families; the ones without a CHAIN parameter live in the CH = 0 kernel
template <class P, int CH>
__global__ void k_field_raw_op(int fam, int par, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                               const uint32_t* d, uint32_t* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe<P> x = raw_load<P>(a, i), y = raw_load<P>(b, i), z = raw_load<P>(c, i), w = raw_load<P>(d, i);
  Fe<P> r = fe_zero<P>();
  switch (fam) {
    case GM_TRAW_MUL_LZ: r = fe_mul<P, false, CH>(x, y); break;
    case GM_TRAW_SQR_LZ: r = fe_sqr<P, false, CH>(x); break;
    case GM_TRAW_MUL: r = fe_mul<P, true, CH>(x, y); break;
    case GM_TRAW_MUL2: r = fe_mul2_redc_u<P, CH>(x, y, z, w); break;
    case GM_TRAW_MUL2_NEGK:
      switch (par) {
        RAW_K(3, r = fe_mul2_redc_u<P, CH>(x, y, fe_negk_cf<3>(z), w))
        RAW_K(5, r = fe_mul2_redc_u<P, CH>(x, y, fe_negk_cf<5>(z), w))
      }
      break;
    case GM_TRAW_SUB_CF_MUL:
      if constexpr (P::N <= 11) {
        switch (par) {
          RAW_K(3, r = fe_mul<P, false, CH>(fe_sub_cf<3>(x, y), z))
          RAW_K(5, r = fe_mul<P, false, CH>(fe_sub_cf<5>(x, y), z))
          RAW_K(9, r = fe_mul<P, false, CH>(fe_sub_cf<9>(x, y), z))
          RAW_K(17, r = fe_mul<P, false, CH>(fe_sub_cf<17>(x, y), z))
        }
      }
      break;
    default: break;
  }
  if constexpr (CH == 0) {
    switch (fam) {
      case GM_TRAW_ADD_LZ: r = fe_add_lz(x, y); break;
      case GM_TRAW_SUB_LZ:
        switch (par) {
          RAW_K(1, r = fe_sub_lz<1>(x, y))
          RAW_K(2, r = fe_sub_lz<2>(x, y))
          RAW_K(4, r = fe_sub_lz<4>(x, y))
          RAW_K(8, r = fe_sub_lz<8>(x, y))
          RAW_K(10, r = fe_sub_lz<10>(x, y))
          RAW_K(16, r = fe_sub_lz<16>(x, y))
          RAW_K(20, r = fe_sub_lz<20>(x, y))
          RAW_K(32, r = fe_sub_lz<32>(x, y))
        }
        break;
      case GM_TRAW_SUB2X_LZ: r = fe_sub2x_lz<6>(x, y, z); break;
      case GM_TRAW_CNEG_SUB:
        switch (par) {
          RAW_K(2, r = fe_sub_lz<2>(fe_cneg2p_cf(x, (w.v[0] & 1) != 0), y))
          RAW_K(4, r = fe_sub_lz<4>(fe_cneg2p_cf(x, (w.v[0] & 1) != 0), y))
        }
        break;
      case GM_TRAW_PMINUS: r = fe_pminus(x); break;
      case GM_TRAW_REDUCE_K:
        r = x;
        switch (par) {
          RAW_K(1, fe_reduce_k<1>(r))
          RAW_K(2, fe_reduce_k<2>(r))
          RAW_K(4, fe_reduce_k<4>(r))
          RAW_K(8, fe_reduce_k<8>(r))
          RAW_K(16, fe_reduce_k<16>(r))
        }
        break;
      case GM_TRAW_CANON:
        switch (par) {
          RAW_K(1, r = fe_canon<1>(x))
          RAW_K(2, r = fe_canon<2>(x))
          RAW_K(3, r = fe_canon<3>(x))
          RAW_K(4, r = fe_canon<4>(x))
        }
        break;
      case GM_TRAW_TO2P:
        r = x;
        switch (par) {
          RAW_K(4, fe_to2p<4>(r))
          RAW_K(6, fe_to2p<6>(r))
          RAW_K(8, fe_to2p<8>(r))
          RAW_K(10, fe_to2p<10>(r))
          RAW_K(12, fe_to2p<12>(r))
        }
        break;
      case GM_TRAW_IS_ZERO:
        switch (par) {
          RAW_K(4, r.v[0] = fe_is_zero_lz<4>(x) ? 1u : 0u)
          RAW_K(6, r.v[0] = fe_is_zero_lz<6>(x) ? 1u : 0u)
          RAW_K(10, r.v[0] = fe_is_zero_lz<10>(x) ? 1u : 0u)
        }
        break;
      case GM_TRAW_TIMES5: r = fe_times5_lz(x); break;
      default: break;
    }
  }
  raw_store<P>(out, i, r);
}

// one-lane Fp2 families and fe_mul4_redc: operands and result are 2 N limbs
template <class P, int BETA>
__global__ void k_field_raw_fe2(int fam, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                                uint32_t* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  using F2 = Fe2<P, BETA>;
  const F2 x{raw_load<P>(a, 2 * i), raw_load<P>(a, 2 * i + 1)}, y{raw_load<P>(b, 2 * i), raw_load<P>(b, 2 * i + 1)};
  F2 r{fe_zero<P>(), fe_zero<P>()};
  switch (fam) {
    case GM_TRAW_FE2_MUL: r = fe2_mul_lz(x, y); break;
    case GM_TRAW_FE2_SQR: r = fe2_sqr_lz<4>(x); break;
    case GM_TRAW_MUL4_REDC:
      if constexpr (P::N <= 9) {
        const F2 z{raw_load<P>(c, 2 * i), raw_load<P>(c, 2 * i + 1)}, w{raw_load<P>(d, 2 * i), raw_load<P>(d, 2 * i + 1)};
        r.a0 = fe_mul4_redc(x.a0, x.a1, y.a0, y.a1, z.a0, z.a1, w.a0, w.a1);
      }
      break;
    default: break;
  }
  raw_store<P>(out, 2 * i, r.a0);
  raw_store<P>(out, 2 * i + 1, r.a1);
}

// lane-pair Fp2 families: element i on lanes 2i (a0) and 2i + 1 (a1), whole
// pairs active (both lanes of a pair leave together)
template <class P, int BETA, bool CH>
__global__ void k_field_raw_pair(int fam, int par, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                 const uint32_t* d, uint32_t* out, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if ((t >> 1) >= n) return;
  const Fe<P> x = raw_load<P>(a, t), y = raw_load<P>(b, t);
  Fe<P> r = fe_zero<P>();
  switch (fam) {
    case GM_TRAW_PF2_MUL: r = pf2_mul<P, BETA, CH>(x, y); break;
    case GM_TRAW_PF2_SQR:
      switch (par) {
        RAW_K(1, r = pf2_sqr<P, BETA, 1, CH>(x))
        RAW_K(2, r = pf2_sqr<P, BETA, 2, CH>(x))
        RAW_K(4, r = pf2_sqr<P, BETA, 4, CH>(x))
      }
      break;
    case GM_TRAW_PF2_MUL_SUB:
      if constexpr (P::N <= 9 && BETA == -1 && !CH) r = pf2_mul_sub(x, y, raw_load<P>(c, t), raw_load<P>(d, t));
      break;
    default: break;
  }
  raw_store<P>(out, t, r);
}

template <class P>
GM_DEV XYZZ<Fe<P>> raw_load_xyzz(const uint32_t* p, size_t i) {
  return {raw_load<P>(p, 4 * i), raw_load<P>(p, 4 * i + 1), raw_load<P>(p, 4 * i + 2), raw_load<P>(p, 4 * i + 3)};
}
template <class P, int CH>
__global__ void k_point_raw_g1(int op, const uint32_t* acc_in, const uint32_t* other, const uint8_t* flags,
                               uint32_t* acc_out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  XYZZ<Fe<P>> a = raw_load_xyzz<P>(acc_in, i);
  if (op == GM_TRAW_G1_ADD_AFF) {
    xyzz_add_aff_lz<P, CH>(a, load_affine_gnark<Fe<P>>(other + i * 2 * P::NG), (flags[i] & 1) != 0);
  } else if constexpr (CH == 0) {
    if (op == GM_TRAW_G1_ADD) a = xyzz_add_lz(a, raw_load_xyzz<P>(other, i));
    else a = xyzz_canon_raw(a);
  }
  raw_store<P>(acc_out, 4 * i, a.x);
  raw_store<P>(acc_out, 4 * i + 1, a.y);
  raw_store<P>(acc_out, 4 * i + 2, a.zz);
  raw_store<P>(acc_out, 4 * i + 3, a.zzz);
}
template <class P, int BETA>
__global__ void k_point_raw_g2(const uint32_t* acc_in, const uint32_t* other, const uint8_t* flags,
                               uint32_t* acc_out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  using F2 = Fe2<P, BETA>;
  auto ld = [&](int k) { return F2{raw_load<P>(acc_in, 8 * i + 2 * k), raw_load<P>(acc_in, 8 * i + 2 * k + 1)}; };
  XYZZ<F2> a{ld(0), ld(1), ld(2), ld(3)};
  Affine<F2> p = load_affine_gnark<F2>(other + i * 4 * P::NG);
  if (flags[i] & 1) p = aff_neg(p);
  xyzz_add_aff_lz(a, p);
  auto st = [&](int k, const F2& v) {
    raw_store<P>(acc_out, 8 * i + 2 * k, v.a0);
    raw_store<P>(acc_out, 8 * i + 2 * k + 1, v.a1);
  };
  st(0, a.x);
  st(1, a.y);
  st(2, a.zz);
  st(3, a.zzz);
}
template <class P, int BETA, bool CH>
__global__ void k_point_raw_pair(int op, const uint32_t* acc_in, const uint32_t* other, const uint8_t* flags,
                                 uint32_t* acc_out, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t >> 1;
  if (i >= n) return;
  constexpr int XW = 8 * P::N;
  PXYZZ<P> a = pxyzz_load<P>(acc_in + i * XW);
  if (op == GM_TRAW_G2P_ADD_AFF || op == GM_TRAW_G2P_DBL_AFF) {
    // this lane's components of the gnark-layout point (X.a0, X.a1, Y.a0, Y.a1)
    const uint32_t* pt = other + i * 4 * P::NG + (pair_odd() ? P::NG : 0);
    const Fe<P> px = Coord<Fe<P>>::load_internal(pt), py = Coord<Fe<P>>::load_internal(pt + 2 * P::NG);
    if (op == GM_TRAW_G2P_ADD_AFF) {
      pxyzz_add_aff<P, BETA, CH>(a, px, py, (flags[i] & 1) != 0);
    } else if constexpr (!CH) {
      a = pxyzz_dbl_aff<P, BETA>(px, py);
    }
  } else if constexpr (!CH) {
    if (op == GM_TRAW_G2P_ADD) a = pxyzz_add<P, BETA>(a, pxyzz_load<P>(other + i * XW));
    else a = pxyzz_dbl<P, BETA>(a);
  }
  pxyzz_store<P>(acc_out + i * XW, a);
}
#undef RAW_K

}  // namespace gm

using namespace gm;

extern "C++" {
// the (family, K, chain) combinations the library instantiates, per field
static bool raw_in(int k, std::initializer_list<int> l) {
  for (int v : l)
    if (v == k) return true;
  return false;
}
static bool raw_field_valid(bool fr, int N, int fam, int K, int chain) {
  if (chain < 0 || chain > 2) return false;
  switch (fam) {
    case GM_TRAW_MUL_LZ: case GM_TRAW_SQR_LZ: case GM_TRAW_MUL: return K == 0;
    case GM_TRAW_MUL2: return !fr && K == 0;
    case GM_TRAW_MUL2_NEGK: return !fr && raw_in(K, {3, 5});
    case GM_TRAW_ADD_LZ: return K == 0;
    case GM_TRAW_SUB_LZ: return fr ? raw_in(K, {2, 4, 8, 16, 32}) : raw_in(K, {1, 2, 4, 8, 10, 20});
    case GM_TRAW_SUB2X_LZ: return !fr && K == 6;
    case GM_TRAW_SUB_CF_MUL: return N <= 11 && (fr ? raw_in(K, {3, 5, 9, 17}) : K == 9);
    case GM_TRAW_CNEG_SUB: return !fr && raw_in(K, {2, 4});
    case GM_TRAW_PMINUS: case GM_TRAW_TIMES5: return !fr && K == 0;
    case GM_TRAW_REDUCE_K: return fr ? raw_in(K, {1, 2, 4, 8, 16}) : raw_in(K, {1, 2, 4, 8});
    case GM_TRAW_CANON: return K >= 1 && K <= 4;
    case GM_TRAW_TO2P: return !fr && raw_in(K, {4, 6, 8, 10, 12});
    case GM_TRAW_IS_ZERO: return !fr && raw_in(K, {4, 6, 10});
    case GM_TRAW_FE2_MUL: return !fr && K == 0;
    case GM_TRAW_FE2_SQR: return !fr && K == 4;
    case GM_TRAW_PF2_MUL: return !fr && K == 0 && chain <= 1;
    case GM_TRAW_PF2_SQR: return !fr && raw_in(K, {1, 2, 4}) && chain <= 1;
    case GM_TRAW_PF2_MUL_SUB: return !fr && N <= 9 && K == 0 && chain == 0;
    case GM_TRAW_MUL4_REDC: return !fr && N <= 9 && K == 0;
    default: return false;
  }
}
// FR: a scalar field -- the Fp2 families are not compiled for it (their bounds are
// asserted against the base field's headroom, which an Fr need not meet)
template <class P, int BETA, bool FR>
static int field_raw_t(gm_ctx* ctx, bool fr, int fam, int K, int chain, const void* a, const void* b, const void* c,
                       const void* d, void* out, size_t n) {
  if (!raw_field_valid(fr, P::N, fam, K, chain)) return GM_ERR_INVALID;
  auto A = (const uint32_t*)a, B = (const uint32_t*)b, C = (const uint32_t*)c, D = (const uint32_t*)d;
  auto O = (uint32_t*)out;
  const dim3 t(64), g(blocks_for(n, 64)), g2(blocks_for(2 * n, 64));
  hipStream_t s = ctx->stream;
  if (fam == GM_TRAW_FE2_MUL || fam == GM_TRAW_FE2_SQR || fam == GM_TRAW_MUL4_REDC) {
    if constexpr (!FR) hipLaunchKernelGGL((k_field_raw_fe2<P, BETA>), g, t, 0, s, fam, A, B, C, D, O, n);
    else return GM_ERR_INVALID;
  } else if (fam >= GM_TRAW_PF2_MUL) {
    if constexpr (!FR) {
      if (chain) hipLaunchKernelGGL((k_field_raw_pair<P, BETA, true>), g2, t, 0, s, fam, K, A, B, C, D, O, n);
      else hipLaunchKernelGGL((k_field_raw_pair<P, BETA, false>), g2, t, 0, s, fam, K, A, B, C, D, O, n);
    } else {
      return GM_ERR_INVALID;
    }
  } else {
    const bool chained = fam <= GM_TRAW_MUL2_NEGK || fam == GM_TRAW_SUB_CF_MUL;
    const int ch = chained ? chain : 0;
    if (ch == 0) hipLaunchKernelGGL((k_field_raw_op<P, 0>), g, t, 0, s, fam, K, A, B, C, D, O, n);
    else if (ch == 1) hipLaunchKernelGGL((k_field_raw_op<P, 1>), g, t, 0, s, fam, K, A, B, C, D, O, n);
    else hipLaunchKernelGGL((k_field_raw_op<P, 2>), g, t, 0, s, fam, K, A, B, C, D, O, n);
  }
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(s));
  return GM_OK;
}
template <class P, int BETA>
static int point_raw_t(gm_ctx* ctx, int g2, int op, int chain, const void* acc_in, const void* other,
                       const void* flags, void* acc_out, size_t n) {
  auto A = (const uint32_t*)acc_in, B = (const uint32_t*)other;
  auto F = (const uint8_t*)flags;
  auto O = (uint32_t*)acc_out;
  const dim3 t(64), g(blocks_for(n, 64)), gp(blocks_for(2 * n, 64));
  hipStream_t s = ctx->stream;
  const bool needs_other = op != GM_TRAW_G1_CANON && op != GM_TRAW_G2P_DBL;
  const bool needs_flags = op == GM_TRAW_G1_ADD_AFF || op == GM_TRAW_G2_ADD_AFF || op == GM_TRAW_G2P_ADD_AFF;
  if ((needs_other && !B) || (needs_flags && !F)) return GM_ERR_INVALID;
  if (!g2) {
    if (op == GM_TRAW_G1_ADD_AFF && chain == 2) {
      hipLaunchKernelGGL((k_point_raw_g1<P, 2>), g, t, 0, s, op, A, B, F, O, n);
    } else if (op >= GM_TRAW_G1_ADD_AFF && op <= GM_TRAW_G1_CANON && chain == 0) {
      hipLaunchKernelGGL((k_point_raw_g1<P, 0>), g, t, 0, s, op, A, B, F, O, n);
    } else {
      return GM_ERR_INVALID;
    }
  } else if (op == GM_TRAW_G2_ADD_AFF && chain == 0) {
    hipLaunchKernelGGL((k_point_raw_g2<P, BETA>), g, t, 0, s, A, B, F, O, n);
  } else if (op == GM_TRAW_G2P_ADD_AFF && chain == 1) {
    hipLaunchKernelGGL((k_point_raw_pair<P, BETA, true>), gp, t, 0, s, op, A, B, F, O, n);
  } else if (op >= GM_TRAW_G2P_ADD_AFF && op <= GM_TRAW_G2P_DBL && chain == 0) {
    hipLaunchKernelGGL((k_point_raw_pair<P, BETA, false>), gp, t, 0, s, op, A, B, F, O, n);
  } else {
    return GM_ERR_INVALID;
  }
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(s));
  return GM_OK;
}
}

extern "C" {
int gm_test_field_raw_op(gm_ctx* ctx, int curve, int kind, int op, int chain, const void* a_dev, const void* b_dev,
                         const void* c_dev, const void* d_dev, void* out_dev, size_t n) {
  if (!ctx || !a_dev || !out_dev || n == 0 || op < 0 || (kind != 0 && kind != 1)) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_test_field_raw_op")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const int fam = op / 100, K = op % 100;
  return GM_CURVE(curve, kind == 0 ? field_raw_t<typename C::Fr, Fp2Beta<C>::value, true>(ctx, true, fam, K, chain, a_dev,
                                                                                    b_dev, c_dev, d_dev, out_dev, n)
                                   : field_raw_t<typename C::Fp, Fp2Beta<C>::value, false>(ctx, false, fam, K, chain, a_dev,
                                                                                    b_dev, c_dev, d_dev, out_dev, n));
}
int gm_test_point_raw_op(gm_ctx* ctx, int curve, int g2, int op, int chain, const void* acc_in_dev,
                         const void* other_dev, const void* flags_dev, void* acc_out_dev, size_t n) {
  if (!ctx || !acc_in_dev || !acc_out_dev || n == 0) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_test_point_raw_op")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE(curve, point_raw_t<typename C::Fp, Fp2Beta<C>::value>(ctx, g2, op, chain, acc_in_dev, other_dev,
                                                                        flags_dev, acc_out_dev, n));
}
}

extern "C++" {
// fe_sqrt (field_sqrt.hpp) on its own: gnark-form elements in, a root in gnark
// form and the exists byte out
template <class F>
__global__ void k_fe_sqrt(const uint8_t* a, uint8_t* root, uint8_t* exists, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F r;
  const bool ok = fe_sqrt(ElemIO<F>::load(a, i), r);
  ElemIO<F>::store(root, i, r);
  exists[i] = ok ? 1 : 0;
}
template <class C>
static int fe_sqrt_t(gm_ctx* ctx, int kind, const void* a, size_t n, void* root, void* exists) {
  auto g = dim3(blocks_for(n, 64)), t = dim3(64);
  if (kind == 1)
    hipLaunchKernelGGL(k_fe_sqrt<typename C::G1F>, g, t, 0, ctx->stream, (const uint8_t*)a, (uint8_t*)root,
                       (uint8_t*)exists, n);
  else
    hipLaunchKernelGGL(k_fe_sqrt<typename C::G2F>, g, t, 0, ctx->stream, (const uint8_t*)a, (uint8_t*)root,
                       (uint8_t*)exists, n);
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}
template <class C>
static int field_op_t(gm_ctx* ctx, int kind, int op, const void* a, const void* b, void* out, size_t n) {
  auto g = dim3(blocks_for(n, 64)), t = dim3(64);
  auto A = (const uint8_t*)a, B = (const uint8_t*)b;
  auto O = (uint8_t*)out;
  if (kind == 0) hipLaunchKernelGGL(k_field_op<Fe<typename C::Fr>>, g, t, 0, ctx->stream, op, A, B, O, n);
  else if (kind == 1) hipLaunchKernelGGL(k_field_op<typename C::G1F>, g, t, 0, ctx->stream, op, A, B, O, n);
  else hipLaunchKernelGGL(k_field_op<typename C::G2F>, g, t, 0, ctx->stream, op, A, B, O, n);
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}
template <class C, bool G2>
static int point_op_t(gm_ctx* ctx, int op, const void* a, const void* b, void* out, size_t n) {
  using DF = typename GroupSel<C, G2>::DF;
  hipLaunchKernelGGL(k_point_op<DF>, dim3(blocks_for(n, 64)), dim3(64), 0, ctx->stream, op,
                     (const uint32_t*)a, (const uint32_t*)b, (uint32_t*)out, n);
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}
}

extern "C" {
int gm_test_field_op(gm_ctx* ctx, int curve, int kind, int op, const void* a_dev, const void* b_dev,
                     void* out_dev, size_t n) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_test_field_op")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  if (kind < 0 || kind > 2) return GM_ERR_INVALID;
  return GM_CURVE(curve, field_op_t<C>(ctx, kind, op, a_dev, b_dev, out_dev, n));
}
int gm_test_fe_sqrt(gm_ctx* ctx, int curve, int kind, const void* a_dev, size_t n, void* root_dev,
                    uint8_t* exists_dev) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_test_fe_sqrt")) return rc;
  if (!ctx || kind < 1 || kind > 2 || (n && (!a_dev || !root_dev || !exists_dev))) return GM_ERR_INVALID;
  if (n == 0) return GM_OK;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE(curve, fe_sqrt_t<C>(ctx, kind, a_dev, n, root_dev, exists_dev));
}
int gm_test_point_op(gm_ctx* ctx, int curve, int g2, int op, const void* a_dev, const void* b_dev,
                     void* out_dev, size_t n) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_test_point_op")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE(curve, g2 ? point_op_t<C, true>(ctx, op, a_dev, b_dev, out_dev, n)
                            : point_op_t<C, false>(ctx, op, a_dev, b_dev, out_dev, n));
}
}

extern "C++" {
template <class C>
static int g2_keyless_plan_t(gm_ctx* ctx, const void* scalars_dev, const void* points_dev, size_t n) {
  Arena arena(ctx);
  MsmPlan plan;
  if (int rc = msm_plan<C>(ctx, arena, scalars_dev, n, nullptr, plan, false, false, false)) return rc;
  MsmTail t;
  const int rc = msm_launch<C, true>(ctx, arena, plan, points_dev, t);
  GM_HIP(hipStreamSynchronize(ctx->stream));  // the plan's kernels, before the arena is released
  return rc;
}
}

extern "C" int gm_test_msm_g2_keyless_plan(gm_ctx* ctx, int curve, const void* scalars_dev, const void* points_dev,
                                           size_t n) {
  if (!ctx || !scalars_dev || !points_dev || n == 0) return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE(curve, g2_keyless_plan_t<C>(ctx, scalars_dev, points_dev, n));
}

// The u32 scans of scan.hpp on their own.  op 0: device_excl_scan (out_dev may be
// in_dev; the workspace holds 0xFF bytes going in); op 1: the one-block max scan
// over a copy of the input in out_dev.
extern "C" int gm_test_scan(gm_ctx* ctx, int op, const void* in_dev, size_t n, void* out_dev) {
  if (!ctx || !out_dev || (n && !in_dev) || op < 0 || op > 1 || (op == 1 && n > 0xffffffffu)) return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  gm::Arena arena(ctx);
  int rc;
  if (op == 0) {
    gm::DevBuf ws;
    const size_t bytes = sizeof(uint32_t) * gm::scan_ws_words(n);
    if ((rc = ws.alloc(arena, bytes))) return rc;
    if (bytes) GM_HIP(hipMemsetAsync(ws.p, 0xFF, bytes, ctx->stream));
    rc = gm::device_excl_scan(ctx, (const uint32_t*)in_dev, n, (uint32_t*)out_dev, ws.as<uint32_t>());
  } else {
    if (n && out_dev != in_dev)
      GM_HIP(hipMemcpyAsync(out_dev, in_dev, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, ctx->stream));
    rc = gm::block_scan_inplace(ctx, (uint32_t*)out_dev, (uint32_t)n, true);
  }
  GM_HIP(hipStreamSynchronize(ctx->stream));  // before the arena is released
  return rc;
}

// The geometry of an MSM from the driver's own host functions (msm.hpp): no
// context, no device call.  The allocations are msm_plan's offsets and
// msm_launch's buckets and two node buffers.
extern "C++" {
template <class C, bool G2>
static int msm_geometry_t(size_t n, int c_override, int layout, int curve, gm_test_msm_geom* out) {
  using DF = typename GroupSel<C, G2>::DF;
  MsmPrecomp pre;
  bool glv = layout == GM_TGEOM_GLV;
  if (layout == GM_TGEOM_DEFAULT) glv = msm_glv_on(nullptr, G2, n);
  if (layout == GM_TGEOM_PRECOMP) {
    int c = 0, W = 0;
    if (int rc = gm_precompute_layout(curve, n, c_override, &c, &W)) return rc;
    pre.c = (uint32_t)c;
    pre.W = (uint32_t)W;
    pre.narrow = precomp_narrow(pre.c, pre.W, C::FR_BITS);
    pre.stride = n;
  }
  MsmPlanGeom pg;
  if (const char* refusal = msm_plan_geom(n, C::FR_BITS, glv, pre.c ? &pre : nullptr, c_override, pg)) {
    set_error(refusal);
    return GM_ERR_INVALID;
  }
  gm_test_msm_geom& o = *out;
  memset(&o, 0, sizeof(o));
  o.c = pg.c;
  o.W = pg.W;
  o.wn = pg.wn;
  o.narrow = pg.W - pg.wn;
  o.Wred = pg.Wred;
  o.nb = pg.nb;
  o.total = pg.total;
  o.glv = glv;
  o.shared = pre.c != 0;
  o.bits = (uint32_t)pg.bits;
  o.F = pg.sg.F;
  o.G = pg.sg.G;
  o.NC = pg.sg.NC;
  o.NS = pg.sg.NS;
  o.compact = pg.sg.compact;
  o.piece_len = msm_piece_len(nullptr, pg.M);
  o.n = pg.n;
  o.M = pg.M;
  o.npts = pg.npts;
  msm_seg_geom(pg.Wred, pg.nb, o.L, o.nseg);
  MsmTreeGeom tg;
  if (!msm_tree_geom(o.nseg, sizeof(XYZZ<DF>), tg)) {
    set_error("msm: bucket reduction does not fit LDS");
    return GM_ERR_INVALID;
  }
  static_assert(GM_TGEOM_MAX_LEVELS == MsmTreeGeom::MAX_LEVELS, "report and driver hold the same levels");
  o.levels = tg.levels;
  for (uint32_t i = 0; i < tg.levels; i++) o.lg[i] = tg.lg[i];
  o.Q = tg.Q;
  o.xyzz_bytes = (uint32_t)sizeof(XYZZ<DF>);
  o.bucket_bytes = (uint64_t)sizeof(XYZZ<DF>) * pg.total;
  o.node_bytes = 2 * (uint64_t)sizeof(XYZZ<DF>) * 2 * pg.Wred * o.nseg;
  o.offset_bytes = (uint64_t)sizeof(uint32_t) * ((uint64_t)pg.total + 1);
  return GM_OK;
}
}

extern "C" int gm_test_msm_geometry(int curve, int g2, size_t n, int c_override, int layout, gm_test_msm_geom* out) {
  if (!out || n == 0 || layout < GM_TGEOM_PLAIN || layout > GM_TGEOM_DEFAULT ||
      curve < 0 || curve >= CURVE_COUNT) {
    set_error("msm geometry: bad curve, size or layout");
    return GM_ERR_INVALID;
  }
  // the window range of gm_set_msm_window (the precomputed range is checked by gm_precompute_layout)
  if (c_override != 0 && (c_override < 2 || c_override > 24)) {
    set_error("msm geometry: window must be 0 (auto) or in [2, 24]");
    return GM_ERR_INVALID;
  }
  return GM_CURVE(curve, g2 ? msm_geometry_t<C, true>(n, c_override, layout, curve, out)
                            : msm_geometry_t<C, false>(n, c_override, layout, curve, out));
}

/* The solver-side cost of staging the reference benchmark circuit's level shape
 * (backend/groth16/groth16_test.go:120-156: a chain of squarings; the solver runs
 * it as one one-instruction level after another, constraint/bn254/solver.go:
 * 471-484).  Level j finishes constraint j and solves wire nb_inputs + j (the
 * last level, the final assertion, solves no wire).  mode 0: one put per level
 * and vector; mode 1: the Go hook's pattern (integration/go/icicle_bn254/
 * staged.go): ids appended to pending lists, handed over every `flush_at` ids and
 * at the end.  abc = 0: wires only (resident constraint system).  The put range
 * of the witness inputs comes first.  *ns_per_level = host time / levels. */
extern "C" int gm_test_stage_replay_chain(gm_g16_stage* st, const void* wires, size_t nb_inputs, const void* a,
                                          const void* b, const void* c, size_t nb_constraints, int mode, int abc,
                                          size_t flush_at, double* ns_per_level) {
  if (!st || !wires || !ns_per_level || (abc && (!a || !b || !c)) || nb_constraints == 0 || flush_at == 0)
    return GM_ERR_INVALID;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = gm_g16_stage_put_range(st, GM_STAGE_WIRES, 0, nb_inputs, wires);
  std::vector<uint32_t> pw, pc;
  pw.reserve(flush_at);
  pc.reserve(flush_at);
  auto put_abc = [&](const uint32_t* ids, size_t k) {
    int r = gm_g16_stage_put_indexed(st, GM_STAGE_A, a, ids, k);
    if (!r) r = gm_g16_stage_put_indexed(st, GM_STAGE_B, b, ids, k);
    if (!r) r = gm_g16_stage_put_indexed(st, GM_STAGE_C, c, ids, k);
    return r;
  };
  for (size_t j = 0; j < nb_constraints && !rc; j++) {
    const uint32_t cid = (uint32_t)j, wid = (uint32_t)(nb_inputs + j);
    const bool solves = j + 1 < nb_constraints;
    if (mode == 0) {
      if (solves) rc = gm_g16_stage_put_indexed(st, GM_STAGE_WIRES, wires, &wid, 1);
      if (!rc && abc) rc = put_abc(&cid, 1);
      continue;
    }
    if (solves) pw.push_back(wid);
    if (pw.size() >= flush_at) {
      rc = gm_g16_stage_put_indexed(st, GM_STAGE_WIRES, wires, pw.data(), pw.size());
      pw.clear();
    }
    if (!abc || rc) continue;
    pc.push_back(cid);
    if (pc.size() >= flush_at) {
      rc = put_abc(pc.data(), pc.size());
      pc.clear();
    }
  }
  if (!rc && !pw.empty()) rc = gm_g16_stage_put_indexed(st, GM_STAGE_WIRES, wires, pw.data(), pw.size());
  if (!rc && !pc.empty()) rc = put_abc(pc.data(), pc.size());
  *ns_per_level = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() /
                  (double)nb_constraints;
  return rc;
}
