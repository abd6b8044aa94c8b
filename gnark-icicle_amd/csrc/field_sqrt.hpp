// Square roots in Fp and Fp2 on the device, all three curves (internal form in
// and out, canonical operands throughout: fe_mul / fe_sqr / fe_add / fe_sub of
// field.hpp, so no lazily reduced bound has to hold).  Either root may come
// back; the point codec picks by the record's flag.  Constants and the
// identities behind them: tools/sqrt_constants.py -> sqrt_constants.hpp.
//
//   Fp, p = 3 mod 4 (BN254, BLS12-381): x = a^((p + 1) / 4), a root iff x^2 = a.
//   Fp, p = 1 mod 4 (BLS12-377, p - 1 = 2^46 s): Tonelli-Shanks.  Its loop is data
//     dependent and diverges inside a wave: a lane whose a^s has order 2^k runs k
//     rounds.  Bound relied on: m starts at S = 46 and falls strictly every
//     round, and a round squares at most m times (i to find the order, m - i - 1
//     for the multiplier, one for c), so at most S (S + 1) / 2 = 1081 squarings
//     and 3 S = 138 products follow the exponentiation by (s - 1) / 2 (352
//     squarings: all 11 x 32 bit positions of the exponent words, leading zeros
//     included); a wave pays for its slowest lane.
//   Fp2 = Fp[u] / (u^2 - beta), the norm method: n = sqrt(a0^2 - beta a1^2), then
//     x0 = sqrt((a0 + n) / 2) or sqrt((a0 - n) / 2) -- their product beta a1^2 / 4
//     is a non-residue when a1 != 0, so exactly one is a square -- and
//     x1 = a1 / (2 x0).  a1 = 0 with a0 a non-residue: (0, sqrt(a0 / beta)).
//     One loop body holds the Fp root of the up to three candidates.
#pragma once
#include "field.hpp"
#include "sqrt_constants.hpp"

namespace gm {

template <class P>
struct SqrtConst;
#define GM_SQRT_CONST(FIELD, TAG)                                                  \
  template <>                                                                      \
  struct SqrtConst<FIELD> {                                                        \
    static constexpr int S = GM_SQRT_##TAG##_S;                                    \
    static constexpr int EXP_WORDS = GM_SQRT_##TAG##_EXP_WORDS;                    \
    GM_CONST_ARRAY_FN(exp, GM_SQRT_##TAG##_EXP_WORDS, GM_SQRT_##TAG##_EXP)         \
    GM_CONST_ARRAY_FN(root, FIELD::N, GM_SQRT_##TAG##_ROOT)                        \
    GM_CONST_ARRAY_FN(half_p, FIELD::N, GM_SQRT_##TAG##_HALF_P)                    \
    GM_CONST_ARRAY_FN(inv2, FIELD::N, GM_SQRT_##TAG##_INV2)                        \
    GM_CONST_ARRAY_FN(beta_inv, FIELD::N, GM_SQRT_##TAG##_BETA_INV)                \
  };
GM_SQRT_CONST(Bn254Fp, BN254)
GM_SQRT_CONST(Bls377Fp, BLS12377)
GM_SQRT_CONST(Bls381Fp, BLS12381)

#define GM_SQRT_FE(P, FN)                                                                    \
  ([]() {                                                                                    \
    ::gm::Fe<P> r_;                                                                          \
    _Pragma("unroll") for (int i_ = 0; i_ < P::N; i_++) r_.v[i_] = SqrtConst<P>::FN(i_);     \
    return r_;                                                                               \
  }())

// a^EXP, the exponent shared by every lane (no divergence on its bits)
template <class P>
GM_DEV Fe<P> fe_pow_sqrt_exp(const Fe<P>& a) {
  using K = SqrtConst<P>;
  Fe<P> r = fe_one<P>();
#pragma unroll 1
  for (int i = K::EXP_WORDS - 1; i >= 0; i--) {
    const uint32_t e = K::exp(i);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      r = fe_sqr(r);
      if ((e >> b) & 1) r = fe_mul(r, a);
    }
  }
  return r;
}

// A square root of a in `out` and true, or false when a is not a square (out is
// then some value whose square is not a).
template <class P>
GM_DEV bool fe_sqrt(const Fe<P>& a, Fe<P>& out) {
  using K = SqrtConst<P>;
  if constexpr (K::S == 1) {
    out = fe_pow_sqrt_exp(a);
  } else {
    const Fe<P> one = fe_one<P>();
    const Fe<P> w = fe_pow_sqrt_exp(a);  // a^((s - 1) / 2)
    Fe<P> x = fe_mul(a, w);              // a^((s + 1) / 2): x^2 = a t
    Fe<P> t = fe_mul(x, w);              // a^s, in the 2-Sylow group (or 0)
    Fe<P> c = GM_SQRT_FE(P, root);
    int m = K::S;
    // invariant: x^2 = a t, c has order 2^m, t has order dividing 2^(m - 1) iff a is a square
#pragma unroll 1
    while (!fe_eq(t, one) && !fe_is_zero(t)) {
      Fe<P> t2 = t;
      int i = 0;
#pragma unroll 1
      while (!fe_eq(t2, one) && i < m) {
        t2 = fe_sqr(t2);
        i++;
      }
      if (i >= m) break;  // t^(2^(m - 1)) != 1: not a square
      Fe<P> b = c;
#pragma unroll 1
      for (int j = 0; j < m - i - 1; j++) b = fe_sqr(b);
      x = fe_mul(x, b);
      c = fe_sqr(b);
      t = fe_mul(t, c);
      m = i;
    }
    out = x;
  }
  return fe_eq(fe_sqr(out), a);
}

template <class P, int BETA>
GM_DEV bool fe_sqrt(const Fe2<P, BETA>& a, Fe2<P, BETA>& out) {
  out.a0 = fe_zero<P>();
  out.a1 = fe_zero<P>();
  if (fe_is_zero(a)) return true;
  const bool real = fe_is_zero(a.a1);
  Fe<P> n;
  if (!fe_sqrt(fe_sub(fe_sqr(a.a0), mul_by_beta<P, BETA>(fe_sqr(a.a1))), n)) return false;
  const Fe<P> inv2 = GM_SQRT_FE(P, inv2);
  // candidates: (a0 + n) / 2, (a0 - n) / 2, and for a1 = 0 also a0 / beta
  bool found = false;
  int k = 0;
  Fe<P> s;
#pragma unroll 1
  for (; k < (real ? 3 : 2) && !found; k++) {
    const Fe<P> cand = k == 2 ? fe_mul(a.a0, GM_SQRT_FE(P, beta_inv))
                              : fe_mul(k == 0 ? fe_add(a.a0, n) : fe_sub(a.a0, n), inv2);
    found = fe_sqrt(cand, s) && (k == 2 || !fe_is_zero(s));
  }
  if (!found) return false;
  if (k == 3) {  // left the loop after k = 2
    out.a1 = s;
  } else {
    out.a0 = s;
    out.a1 = fe_mul(a.a1, fe_inv(fe_dbl(s)));
  }
  const Fe2<P, BETA> sq = fe_sqr(out);
  return fe_eq(sq.a0, a.a0) && fe_eq(sq.a1, a.a1);
}

// canonical limbs a > (p - 1) / 2: gnark-crypto's LexicographicallyLargest on Fp
template <class P>
GM_DEV bool fe_canonical_above_half(const Fe<P>& canon) {
  int32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < P::N; i++) {
    const int32_t d = (int32_t)SqrtConst<P>::half_p(i) - (int32_t)canon.v[i] + borrow;
    borrow = d >> RADIX;
  }
  return borrow != 0;  // half_p - a < 0
}
// the same of an internal-form element; Fp2: decided by a1 unless a1 = 0
template <class P>
GM_DEV bool fe_is_larger(const Fe<P>& a) { return fe_canonical_above_half(fe_from_mont(a)); }
template <class P, int BETA>
GM_DEV bool fe_is_larger(const Fe2<P, BETA>& a) {
  return fe_is_zero(a.a1) ? fe_is_larger(a.a0) : fe_is_larger(a.a1);
}

}  // namespace gm
