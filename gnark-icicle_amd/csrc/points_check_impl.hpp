// The point-check kernel (one lane per point) and its launcher; included by the
// per-curve units points_check_<curve>.hip, which instantiate G1 and G2.
//
// Classes, first that applies (include/gnark_mi355x.h): a coordinate word
// string >= p as stored -> NOT_REDUCED, before any arithmetic; (0, 0) -> OK and an
// infinity; y^2 != x^3 + b -> OFF_CURVE; [r]P != infinity -> OFF_SUBGROUP.  The
// last one is decided by an endomorphism equation that holds exactly when
// [r]P = infinity (tools/subgroup_constants.py asserts the
// integer identities and derives the constants):
//   BN254 G1      nothing: the cofactor is 1
//   BLS12 G1      [u]([u]P) - P = phi(P),  phi(x, y) = (beta x, y)
//   BN254 G2      [6]([u]([u]Q)) = psi(Q)
//   BLS12 G2      [|u|]Q = +-psi(Q) (the sign of u),  psi(x, y) = (gx conj(x), gy conj(y))
//
// Arithmetic: canonical operands throughout (fe_mul / fe_sqr / fe_add / fe_sub
// of field.hpp, each canonical in and out), so fe_eq on limbs is equality in the
// field and no lazily reduced bound has to hold.  The ladders' scalar is the same
// in every lane (no divergence on its bits); the group law's exceptional cases
// are those of xyzz_dbl / xyzz_add_aff / xyzz_add (curve.hpp): an accumulator at
// infinity (ZZ = 0) doubles to infinity and takes the addend, acc = +-addend
// doubles or goes to infinity, and a point with y = 0 doubles to ZZ = 0.
#pragma once
#include "curves.hpp"
#include "points_check.hpp"
#include "subgroup_constants.hpp"

namespace gm {

constexpr unsigned PC_TPB = 128;

#define GM_PC_FE(P, ...)                                                      \
  ([]() {                                                                     \
    constexpr uint32_t a_[P::N] = __VA_ARGS__;                                \
    ::gm::Fe<P> r_;                                                           \
    _Pragma("unroll") for (int i_ = 0; i_ < P::N; i_++) r_.v[i_] = a_[i_];    \
    return r_;                                                                \
  }())

template <class C>
struct PcConst;
#define GM_PC_CONST(CURVE, TAG, IS_BN)                                                           \
  template <>                                                                                    \
  struct PcConst<CURVE> {                                                                        \
    using P = typename CURVE::Fp;                                                                \
    using F2 = typename CURVE::G2F;                                                              \
    static constexpr uint64_t U = GM_SUB_##TAG##_U_ABS;                                          \
    static constexpr bool U_NEG = GM_SUB_##TAG##_U_NEG != 0;                                     \
    static constexpr bool BN = IS_BN;                                                            \
    GM_DEV static Fe<P> b(const Fe<P>*) { return GM_PC_FE(P, GM_SUB_##TAG##_B); }                \
    GM_DEV static F2 b(const F2*) {                                                              \
      return {GM_PC_FE(P, GM_SUB_##TAG##_B2_A0), GM_PC_FE(P, GM_SUB_##TAG##_B2_A1)};             \
    }                                                                                            \
    GM_DEV static F2 psi_x() {                                                                   \
      return {GM_PC_FE(P, GM_SUB_##TAG##_PSI_X_A0), GM_PC_FE(P, GM_SUB_##TAG##_PSI_X_A1)};       \
    }                                                                                            \
    GM_DEV static F2 psi_y() {                                                                   \
      return {GM_PC_FE(P, GM_SUB_##TAG##_PSI_Y_A0), GM_PC_FE(P, GM_SUB_##TAG##_PSI_Y_A1)};       \
    }                                                                                            \
  };
GM_PC_CONST(CurveBN254, BN254, true)
GM_PC_CONST(CurveBLS12377, BLS12377, false)
GM_PC_CONST(CurveBLS12381, BLS12381, false)

// phi's beta (the BLS12 curves; BN254 G1 has no subgroup test)
template <class C>
struct PcBeta;
template <>
struct PcBeta<CurveBLS12377> {
  GM_DEV static Fe<Bls377Fp> get() { return GM_PC_FE(Bls377Fp, GM_SUB_BLS12377_BETA); }
};
template <>
struct PcBeta<CurveBLS12381> {
  GM_DEV static Fe<Bls381Fp> get() { return GM_PC_FE(Bls381Fp, GM_SUB_BLS12381_BETA); }
};

// ---- raw coordinates: the words as stored, before any arithmetic ---------------
// g < p as integers (one borrow chain over the gnark words)
template <class P>
GM_DEV bool feg_below_p(const FeG<P>& g) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < P::NG; i++) {
    const uint64_t d = (uint64_t)g.w[i] - (uint64_t)P::pg(i) - borrow;
    borrow = d >> 63;
  }
  return borrow != 0;
}
// loads one coordinate: the unpacked words (gnark form, not yet internal), whether
// every component is below p, and the OR of all its words
template <class P>
GM_DEV void pc_load_raw(const uint32_t* __restrict__ src, Fe<P>& out, bool& reduced, uint32_t& any) {
  const FeG<P> g = feg_load<P>(src);
  reduced = reduced && feg_below_p(g);
#pragma unroll
  for (int i = 0; i < P::NG; i++) any |= g.w[i];
  out = fe_unpack<P>(g);
}
template <class P, int B>
GM_DEV void pc_load_raw(const uint32_t* __restrict__ src, Fe2<P, B>& out, bool& reduced, uint32_t& any) {
  pc_load_raw(src, out.a0, reduced, any);
  pc_load_raw(src + P::NG, out.a1, reduced, any);
}
template <class P>
GM_DEV Fe<P> pc_to_internal(const Fe<P>& raw) { return fe_to_internal(raw); }
template <class P, int B>
GM_DEV Fe2<P, B> pc_to_internal(const Fe2<P, B>& raw) { return {fe_to_internal(raw.a0), fe_to_internal(raw.a1)}; }

template <class P>
GM_DEV bool pc_eq(const Fe<P>& a, const Fe<P>& b) { return fe_eq(a, b); }
template <class P, int B>
GM_DEV bool pc_eq(const Fe2<P, B>& a, const Fe2<P, B>& b) { return fe_eq(a.a0, b.a0) && fe_eq(a.a1, b.a1); }

// ---- ladders over a scalar shared by all lanes -----------------------------------
// [k]p for affine p != infinity, k != 0: double-and-add from the bit below the top
template <class F>
GM_DEV XYZZ<F> pc_mul_aff(const Affine<F>& p, uint64_t k) {
  XYZZ<F> acc;
  acc.x = p.x;
  acc.y = p.y;
  acc.zz = FOps<F>::one();
  acc.zzz = FOps<F>::one();
#pragma unroll 1
  for (int b = 62 - __builtin_clzll(k); b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if ((k >> b) & 1) xyzz_add_aff(acc, p);
  }
  return acc;
}
// [k]q for any q (infinity included), k != 0
template <class F>
GM_DEV XYZZ<F> pc_mul_xyzz(const XYZZ<F>& q, uint64_t k) {
  XYZZ<F> acc = q;
#pragma unroll 1
  for (int b = 62 - __builtin_clzll(k); b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if ((k >> b) & 1) acc = xyzz_add(acc, q);
  }
  return acc;
}
// t == the affine point (x, y), projectively: X = x ZZ, Y = y ZZZ, ZZ != 0
template <class F>
GM_DEV bool pc_same_point(const XYZZ<F>& t, const F& x, const F& y) {
  if (xyzz_is_inf(t)) return false;
  return pc_eq(t.x, fe_mul(x, t.zz)) && pc_eq(t.y, fe_mul(y, t.zzz));
}

// [r]p = infinity for p on the curve and not infinity
template <class C, bool G2, class F>
GM_DEV bool pc_in_subgroup(const Affine<F>& p) {
  using K = PcConst<C>;
  if constexpr (!G2) {
    if constexpr (K::BN) {
      return true;
    } else {
      // [u^2 - 1]P = phi(P); u^2 does not see the sign of u
      XYZZ<F> t = pc_mul_xyzz(pc_mul_aff(p, K::U), K::U);
      xyzz_add_aff(t, aff_neg(p));
      return pc_same_point(t, fe_mul(p.x, PcBeta<C>::get()), p.y);
    }
  } else {
    // psi(Q) = (gx conj(x), gy conj(y))
    F cx = p.x, cy = p.y;
    cx.a1 = fe_neg(cx.a1);
    cy.a1 = fe_neg(cy.a1);
    const F px = fe_mul(K::psi_x(), cx);
    F py = fe_mul(K::psi_y(), cy);
    if constexpr (K::BN) {
      XYZZ<F> t = pc_mul_xyzz(pc_mul_aff(p, K::U), K::U);  // [u^2]Q
      const XYZZ<F> t2 = xyzz_dbl(t);
      t = xyzz_dbl(xyzz_add(t2, t));                         // [6 u^2]Q = [t - 1]Q
      return pc_same_point(t, px, py);
    } else {
      if constexpr (K::U_NEG) py = fe_neg(py);               // [u]Q = -[|u|]Q
      return pc_same_point(pc_mul_aff(p, K::U), px, py);
    }
  }
}

template <class C, bool G2, class F>
GM_DEV uint32_t pc_classify(const uint32_t* __restrict__ src, bool& infinity) {
  Affine<F> p;
  bool reduced = true;
  uint32_t any = 0;
  pc_load_raw(src, p.x, reduced, any);
  pc_load_raw(src + Coord<F>::WORDS, p.y, reduced, any);
  infinity = false;
  if (!reduced) return GM_POINT_NOT_REDUCED;
  if (any == 0) {
    infinity = true;
    return GM_POINT_OK;
  }
  p.x = pc_to_internal(p.x);
  p.y = pc_to_internal(p.y);
  const F rhs = fe_add(fe_mul(fe_sqr(p.x), p.x), PcConst<C>::b((const F*)nullptr));
  if (!pc_eq(fe_sqr(p.y), rhs)) return GM_POINT_OFF_CURVE;
  return pc_in_subgroup<C, G2, F>(p) ? GM_POINT_OK : GM_POINT_OFF_SUBGROUP;
}

// One lane per point.  A wave adds each of its non-zero counts with one atomicAdd
// (ballot + popcount) and sends its lowest failing lane's 4 * index + class to the
// atomicMin, as k_scs_check reports its first failure.  Lanes past n take part in
// the ballots with nothing to report.
template <class C, bool G2>
__global__ void __launch_bounds__(PC_TPB)
    k_points_check(const uint32_t* __restrict__ pts, size_t n, size_t base, uint8_t* __restrict__ status,
                   unsigned long long* __restrict__ res) {
  using F = typename GroupSel<C, G2>::DF;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  uint32_t cls = GM_POINT_OK;
  bool inf = false;
  if (live) {
    cls = pc_classify<C, G2, F>(pts + i * 2 * Coord<F>::WORDS, inf);
    if (status) status[i] = (uint8_t)cls;
  }
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long m_inf = __ballot(live && inf);
  const unsigned long long m_bad = __ballot(live && cls != GM_POINT_OK);
  if (m_inf && lane == (unsigned)(__ffsll((long long)m_inf) - 1))
    atomicAdd(res + PC_INFINITIES, (unsigned long long)__popcll(m_inf));
  if (m_bad) {
#pragma unroll
    for (uint32_t c = GM_POINT_NOT_REDUCED; c <= GM_POINT_OFF_SUBGROUP; c++) {
      const unsigned long long m = __ballot(live && cls == c);
      if (m && lane == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(res + c, (unsigned long long)__popcll(m));
    }
    if (lane == (unsigned)(__ffsll((long long)m_bad) - 1))
      atomicMin(res + PC_FIRST_KEY, (unsigned long long)(base + i) * 4 + cls);
  }
}

template <class C, bool G2>
int points_check_launch(gm_ctx* ctx, const void* pts_dev, size_t n, size_t base, uint8_t* status_dev,
                        unsigned long long* res_dev) {
  if (n == 0) return GM_OK;
  ProfScope ps(ctx, G2 ? "points_check_g2" : "points_check_g1");
  hipLaunchKernelGGL((k_points_check<C, G2>), dim3(blocks_for(n, PC_TPB)), dim3(PC_TPB), 0, ctx->stream,
                     (const uint32_t*)pts_dev, n, base, status_dev, res_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

#define GM_PC_INSTANTIATE(CURVE)                                                                              \
  template int points_check_launch<CURVE, false>(gm_ctx*, const void*, size_t, size_t, uint8_t*,              \
                                                 unsigned long long*);                                        \
  template int points_check_launch<CURVE, true>(gm_ctx*, const void*, size_t, size_t, uint8_t*,               \
                                                unsigned long long*);

}  // namespace gm
