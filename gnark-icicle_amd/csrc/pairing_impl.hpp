// The optimal ate pairing on the device: the Fp12 tower, the Miller loop (one lane
// per pair), the product of Miller values (one lane per 16 values) and the final
// exponentiation (one lane per product).  Included by the per-curve units
// pairing_<curve>.hip, which instantiate the launchers, and by the test hooks.
//
// Tower (gnark-crypto's): Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v), so
// w^6 = xi; an element sum c_i w^i is C0 = (c0, c2, c4), C1 = (c1, c3, c5).
// xi = 9 + u (BN254), u (BLS12-377), 1 + u (BLS12-381).
//
// Lines.  T = (X : Y : Z) on the twist E'(Fp2), homogeneous; P = (xP, yP) in
// E(Fp).  A line with slope l on the twist is, after the untwist and up to a
// factor of a proper subfield (which the final exponentiation sends to 1),
//   D-twist (BN254, BLS12-377)   yP + (-l xP) w + (l xT - yT) w^3
//   M-twist (BLS12-381)          (l xT - yT) + (-l xP) w^2 + yP w^3
// kept as Line{ly, lx, lc}: the coefficient of yP, of -l xP and the constant, all
// scaled by the same Fp2 factor (2 Y Z^2 for a tangent, x2 Z - X for a chord).
//
// The value computed is e(P, Q)^s with gnark-crypto's s: 3 on the BLS12 curves,
// 2u(6u^2 + 3u + 1) on BN254 (tools/pairing_constants.py asserts the hard-part
// identities).
//
// Arithmetic: canonical operands throughout (fe_mul / fe_sqr / fe_add / fe_sub of
// field.hpp), so equality on limbs is equality in the field and no lazily reduced
// bound has to hold.  The loop counters are the same in every lane.  The Fp2, Fp6
// and Fp12 products are real calls (__noinline__): a lane's Fp12 value alone is
// 108 (BN254) or 168 registers, so the operands live in scratch whatever is
// inlined, and one copy of each product keeps the units' build time in minutes.
#pragma once
#include "curves.hpp"
#include "pairing.hpp"
#include "pairing_constants.hpp"
#include "points_check_impl.hpp"

namespace gm {

constexpr unsigned PR_TPB = 64;
#define GM_PR_CALL __device__ __noinline__

template <class C>
struct PrConst;
#define GM_PR_FROB(P, TAG, K, I)                                            \
  GM_DEV static F2 frob##K##_##I() {                                        \
    return {GM_PC_FE(P, GM_PAIR_##TAG##_FROB##K##_##I##_A0),                \
            GM_PC_FE(P, GM_PAIR_##TAG##_FROB##K##_##I##_A1)};               \
  }
#define GM_PR_FROB_ROW(P, TAG, K) \
  GM_PR_FROB(P, TAG, K, 1) GM_PR_FROB(P, TAG, K, 2) GM_PR_FROB(P, TAG, K, 3) GM_PR_FROB(P, TAG, K, 4) GM_PR_FROB(P, TAG, K, 5)
#define GM_PR_CONST(CURVE, TAG)                                             \
  template <>                                                               \
  struct PrConst<CURVE> {                                                   \
    using P = typename CURVE::Fp;                                           \
    using F2 = typename CURVE::G2F;                                         \
    static constexpr bool M_TWIST = GM_PAIR_##TAG##_M_TWIST != 0;           \
    static constexpr int LOOP_BITS = GM_PAIR_##TAG##_LOOP_BITS;             \
    static constexpr uint64_t LOOP_LOW = GM_PAIR_##TAG##_LOOP_LOW;          \
    GM_PR_FROB_ROW(P, TAG, 1) GM_PR_FROB_ROW(P, TAG, 2) GM_PR_FROB_ROW(P, TAG, 3) \
  };
GM_PR_CONST(CurveBN254, BN254)
GM_PR_CONST(CurveBLS12377, BLS12377)
GM_PR_CONST(CurveBLS12381, BLS12381)

template <class C>
struct Pr {
  using P = typename C::Fp;
  using F1 = Fe<P>;
  using F2 = typename C::G2F;
  using K = PrConst<C>;
  using S = PcConst<C>;  // the seed u and psi
  static constexpr int GT_WORDS = 12 * P::NG;  // one Fp12 in gnark layout

  struct F6 {
    F2 b0, b1, b2;
  };
  struct F12 {
    F6 c0, c1;
  };
  struct Line {
    F2 ly, lx, lc;
  };
  struct Proj {
    F2 x, y, z;
  };

  // ---- Fp2 ----------------------------------------------------------------------
  GM_PR_CALL static F2 m2(const F2& a, const F2& b) { return fe_mul(a, b); }
  GM_PR_CALL static F2 s2(const F2& a) { return fe_sqr(a); }
  GM_DEV static F2 conj2(const F2& a) { return {a.a0, fe_neg(a.a1)}; }
  GM_DEV static F2 scale2(const F2& a, const F1& k) { return {fe_mul(a.a0, k), fe_mul(a.a1, k)}; }
  GM_DEV static bool eq2(const F2& a, const F2& b) { return fe_eq(a.a0, b.a0) && fe_eq(a.a1, b.a1); }
  // a xi
  GM_DEV static F2 mxi(const F2& a) {
    if constexpr (C::id == CurveBN254::id) {  // (9 + u)(a0 + a1 u) = 9 a0 - a1 + (9 a1 + a0) u
      const F2 a8 = fe_dbl(fe_dbl(fe_dbl(a)));
      const F2 a9 = fe_add(a8, a);
      return {fe_sub(a9.a0, a.a1), fe_add(a9.a1, a.a0)};
    } else if constexpr (C::id == CurveBLS12377::id) {  // u (a0 + a1 u) = -5 a1 + a0 u
      return {mul_by_beta<P, Fp2Beta<C>::value>(a.a1), a.a0};
    } else {  // (1 + u)(a0 + a1 u) = a0 - a1 + (a0 + a1) u
      return {fe_sub(a.a0, a.a1), fe_add(a.a0, a.a1)};
    }
  }

  // ---- Fp6 ----------------------------------------------------------------------
  GM_DEV static F6 zero6() { return {FOps<F2>::zero(), FOps<F2>::zero(), FOps<F2>::zero()}; }
  GM_DEV static F6 add6(const F6& a, const F6& b) { return {fe_add(a.b0, b.b0), fe_add(a.b1, b.b1), fe_add(a.b2, b.b2)}; }
  GM_DEV static F6 sub6(const F6& a, const F6& b) { return {fe_sub(a.b0, b.b0), fe_sub(a.b1, b.b1), fe_sub(a.b2, b.b2)}; }
  GM_DEV static F6 neg6(const F6& a) { return {fe_neg(a.b0), fe_neg(a.b1), fe_neg(a.b2)}; }
  GM_DEV static F6 mulv6(const F6& a) { return {mxi(a.b2), a.b0, a.b1}; }
  GM_DEV static bool eq6(const F6& a, const F6& b) { return eq2(a.b0, b.b0) && eq2(a.b1, b.b1) && eq2(a.b2, b.b2); }
  // Karatsuba over Fp2: 6 products
  GM_PR_CALL static F6 mul6(const F6& a, const F6& b) {
    const F2 t0 = m2(a.b0, b.b0), t1 = m2(a.b1, b.b1), t2 = m2(a.b2, b.b2);
    F6 r;
    r.b0 = fe_add(t0, mxi(fe_sub(fe_sub(m2(fe_add(a.b1, a.b2), fe_add(b.b1, b.b2)), t1), t2)));
    r.b1 = fe_add(fe_sub(fe_sub(m2(fe_add(a.b0, a.b1), fe_add(b.b0, b.b1)), t0), t1), mxi(t2));
    r.b2 = fe_add(fe_sub(fe_sub(m2(fe_add(a.b0, a.b2), fe_add(b.b0, b.b2)), t0), t2), t1);
    return r;
  }
  // a (b0 + b1 v)
  GM_PR_CALL static F6 mul6_01(const F6& a, const F2& b0, const F2& b1) {
    F6 r;
    r.b0 = fe_add(m2(a.b0, b0), mxi(m2(a.b2, b1)));
    r.b1 = fe_add(m2(a.b0, b1), m2(a.b1, b0));
    r.b2 = fe_add(m2(a.b1, b1), m2(a.b2, b0));
    return r;
  }
  // a (b1 v)
  GM_DEV static F6 mul6_1(const F6& a, const F2& b1) { return {mxi(m2(a.b2, b1)), m2(a.b0, b1), m2(a.b1, b1)}; }
  GM_DEV static F6 scale6(const F6& a, const F2& k) { return {m2(a.b0, k), m2(a.b1, k), m2(a.b2, k)}; }
  // 1 / a; inv(0) = 0 (fe_inv sends 0 to 0)
  GM_PR_CALL static F6 inv6(const F6& a) {
    const F2 A = fe_sub(s2(a.b0), mxi(m2(a.b1, a.b2)));
    const F2 B = fe_sub(mxi(s2(a.b2)), m2(a.b0, a.b1));
    const F2 Cc = fe_sub(s2(a.b1), m2(a.b0, a.b2));
    const F2 d = fe_add(m2(a.b0, A), mxi(fe_add(m2(a.b2, B), m2(a.b1, Cc))));
    const F2 di = fe_inv(d);
    return {m2(A, di), m2(B, di), m2(Cc, di)};
  }

  // ---- Fp12 ---------------------------------------------------------------------
  GM_DEV static F12 one12() {
    F12 r{zero6(), zero6()};
    r.c0.b0 = FOps<F2>::one();
    return r;
  }
  GM_DEV static bool eq12(const F12& a, const F12& b) { return eq6(a.c0, b.c0) && eq6(a.c1, b.c1); }
  GM_DEV static F12 conj12(const F12& a) { return {a.c0, neg6(a.c1)}; }
  GM_PR_CALL static F12 mul12(const F12& a, const F12& b) {
    const F6 t0 = mul6(a.c0, b.c0), t1 = mul6(a.c1, b.c1);
    F12 r;
    r.c1 = sub6(sub6(mul6(add6(a.c0, a.c1), add6(b.c0, b.c1)), t0), t1);
    r.c0 = add6(t0, mulv6(t1));
    return r;
  }
  // complex squaring: 2 Fp6 products
  GM_PR_CALL static F12 sqr12(const F12& a) {
    const F6 t = mul6(a.c0, a.c1);
    F12 r;
    r.c0 = sub6(sub6(mul6(add6(a.c0, a.c1), add6(a.c0, mulv6(a.c1))), t), mulv6(t));
    r.c1 = add6(t, t);
    return r;
  }
  GM_PR_CALL static F12 inv12(const F12& a) {
    const F6 ti = inv6(sub6(mul6(a.c0, a.c0), mulv6(mul6(a.c1, a.c1))));
    return {mul6(a.c0, ti), neg6(mul6(a.c1, ti))};
  }
  // a^(p^KF): conj^KF on every coefficient, then c_i xi^(i (p^KF - 1) / 6)
  template <int KF>
  GM_PR_CALL static F12 frob12(const F12& a) {
    static_assert(KF >= 1 && KF <= 3, "Frobenius powers 1..3");
    F12 r = a;
    if constexpr (KF & 1) {
      r.c0.b0 = conj2(r.c0.b0);
      r.c0.b1 = conj2(r.c0.b1);
      r.c0.b2 = conj2(r.c0.b2);
      r.c1.b0 = conj2(r.c1.b0);
      r.c1.b1 = conj2(r.c1.b1);
      r.c1.b2 = conj2(r.c1.b2);
    }
    if constexpr (KF == 1) {
      r.c1.b0 = m2(r.c1.b0, K::frob1_1());
      r.c0.b1 = m2(r.c0.b1, K::frob1_2());
      r.c1.b1 = m2(r.c1.b1, K::frob1_3());
      r.c0.b2 = m2(r.c0.b2, K::frob1_4());
      r.c1.b2 = m2(r.c1.b2, K::frob1_5());
    } else if constexpr (KF == 2) {
      r.c1.b0 = m2(r.c1.b0, K::frob2_1());
      r.c0.b1 = m2(r.c0.b1, K::frob2_2());
      r.c1.b1 = m2(r.c1.b1, K::frob2_3());
      r.c0.b2 = m2(r.c0.b2, K::frob2_4());
      r.c1.b2 = m2(r.c1.b2, K::frob2_5());
    } else {
      r.c1.b0 = m2(r.c1.b0, K::frob3_1());
      r.c0.b1 = m2(r.c0.b1, K::frob3_2());
      r.c1.b1 = m2(r.c1.b1, K::frob3_3());
      r.c0.b2 = m2(r.c0.b2, K::frob3_4());
      r.c1.b2 = m2(r.c1.b2, K::frob3_5());
    }
    return r;
  }
  // Granger-Scott squaring of an element of the cyclotomic subgroup.  Over
  // Fp4 = Fp2[s]/(s^2 - xi), s = w^3, the element is A + B w + C w^2 with
  // A = (c0, c3), B = (c1, c4), C = (c2, c5), and its square is
  // (3 A^2 - 2 conj A) + (3 s C^2 + 2 conj B) w + (3 B^2 - 2 conj C) w^2.
  GM_DEV static F2 m3s2(const F2& t, const F2& x) {  // 3t - 2x
    const F2 d = fe_sub(t, x);
    return fe_add(fe_dbl(d), t);
  }
  GM_DEV static F2 m3a2(const F2& t, const F2& x) {  // 3t + 2x
    const F2 d = fe_add(t, x);
    return fe_add(fe_dbl(d), t);
  }
  GM_PR_CALL static F12 cyc_sqr12(const F12& a) {
    F2 t0 = s2(a.c1.b1), t1 = s2(a.c0.b0);
    const F2 t6 = fe_sub(fe_sub(s2(fe_add(a.c1.b1, a.c0.b0)), t0), t1);  // 2 c3 c0
    F2 t2 = s2(a.c0.b2), t3 = s2(a.c1.b0);
    const F2 t7 = fe_sub(fe_sub(s2(fe_add(a.c0.b2, a.c1.b0)), t2), t3);  // 2 c4 c1
    F2 t4 = s2(a.c1.b2), t5 = s2(a.c0.b1);
    const F2 t8 = mxi(fe_sub(fe_sub(s2(fe_add(a.c1.b2, a.c0.b1)), t4), t5));  // 2 c5 c2 xi
    t0 = fe_add(mxi(t0), t1);  // c3^2 xi + c0^2
    t2 = fe_add(mxi(t2), t3);  // c4^2 xi + c1^2
    t4 = fe_add(mxi(t4), t5);  // c5^2 xi + c2^2
    F12 r;
    r.c0.b0 = m3s2(t0, a.c0.b0);
    r.c0.b1 = m3s2(t2, a.c0.b1);
    r.c0.b2 = m3s2(t4, a.c0.b2);
    r.c1.b0 = m3a2(t8, a.c1.b0);
    r.c1.b1 = m3a2(t6, a.c1.b1);
    r.c1.b2 = m3a2(t7, a.c1.b2);
    return r;
  }
  // a^|u| for a in the cyclotomic subgroup: square-and-multiply from the bit below the top
  GM_PR_CALL static F12 exp_abs_u12(const F12& a) {
    F12 r = a;
#pragma unroll 1
    for (int b = 62 - __builtin_clzll(S::U); b >= 0; b--) {
      r = cyc_sqr12(r);
      if ((S::U >> b) & 1) r = mul12(r, a);
    }
    return r;
  }
  // a^u: the inverse of a cyclotomic element is its conjugate
  GM_DEV static F12 exp_u12(const F12& a) {
    const F12 r = exp_abs_u12(a);
    if constexpr (S::U_NEG) return conj12(r);
    else return r;
  }
  // f times the line (the header comment has the slots)
  GM_PR_CALL static F12 line_mul12(const F12& f, const Line& l) {
    F6 t0, t1, s;
    if constexpr (!K::M_TWIST) {
      // ly + (lx + lc v) w
      t0 = scale6(f.c0, l.ly);
      t1 = mul6_01(f.c1, l.lx, l.lc);
      s = mul6_01(add6(f.c0, f.c1), fe_add(l.ly, l.lx), l.lc);
    } else {
      // (lc + lx v) + (ly v) w
      t0 = mul6_01(f.c0, l.lc, l.lx);
      t1 = mul6_1(f.c1, l.ly);
      s = mul6_01(add6(f.c0, f.c1), l.lc, fe_add(l.lx, l.ly));
    }
    F12 r;
    r.c1 = sub6(sub6(s, t0), t1);
    r.c0 = add6(t0, mulv6(t1));
    return r;
  }

  // ---- Miller loop ----------------------------------------------------------------
  // T <- 2T and the tangent at T, evaluated at P and scaled by 2 Y Z^2:
  //   ly = 2 Y Z^2 yP,  lx = -3 X^2 Z xP,  lc = 3 X^3 - 2 Y^2 Z
  // The doubling is the homogeneous one for a = 0 (it does not see b').
  GM_PR_CALL static void dbl_step(Proj& T, const Affine<F1>& p, Line& l) {
    const F2 xx = s2(T.x);
    const F2 W = fe_add(fe_dbl(xx), xx);
    const F2 Sv = m2(T.y, T.z);
    const F2 yy = s2(T.y);
    l.ly = scale2(fe_dbl(m2(Sv, T.z)), p.y);
    l.lx = scale2(fe_neg(m2(W, T.z)), p.x);
    l.lc = fe_sub(m2(W, T.x), fe_dbl(m2(yy, T.z)));
    const F2 R = m2(T.y, Sv);
    const F2 B4 = fe_dbl(fe_dbl(m2(T.x, R)));
    const F2 H = fe_sub(s2(W), fe_dbl(B4));
    const F2 RR8 = fe_dbl(fe_dbl(fe_dbl(s2(R))));
    T.x = fe_dbl(m2(H, Sv));
    T.y = fe_sub(m2(W, fe_sub(B4, H)), RR8);
    T.z = fe_dbl(fe_dbl(fe_dbl(m2(s2(Sv), Sv))));
  }
  // T <- T + Q (Q affine, T != +-Q) and the chord, scaled by mu = x2 Z - X:
  //   ly = mu yP,  lx = -th xP,  lc = th x2 - mu y2,  th = y2 Z - Y
  GM_PR_CALL static void add_step(Proj& T, const Affine<F2>& q, const Affine<F1>& p, Line& l) {
    const F2 th = fe_sub(m2(q.y, T.z), T.y);
    const F2 mu = fe_sub(m2(q.x, T.z), T.x);
    l.ly = scale2(mu, p.y);
    l.lx = scale2(fe_neg(th), p.x);
    l.lc = fe_sub(m2(th, q.x), m2(mu, q.y));
    const F2 vv = s2(mu);
    const F2 vvv = m2(vv, mu);
    const F2 R = m2(vv, T.x);
    const F2 A = fe_sub(fe_sub(m2(s2(th), T.z), vvv), fe_dbl(R));
    const F2 y3 = fe_sub(m2(th, fe_sub(R, A)), m2(vvv, T.y));
    T.x = m2(mu, A);
    T.y = y3;
    T.z = m2(vvv, T.z);
  }
  GM_DEV static Affine<F2> psi(const Affine<F2>& q) {
    return {m2(S::psi_x(), conj2(q.x)), m2(S::psi_y(), conj2(q.y))};
  }
  // The Miller value of (P, Q), neither at infinity, both in their subgroups.
  GM_PR_CALL static F12 miller(const Affine<F1>& p, const Affine<F2>& q) {
    F12 f = one12();
    Proj T{q.x, q.y, FOps<F2>::one()};
    Line l;
#pragma unroll 1
    for (int b = K::LOOP_BITS - 2; b >= 0; b--) {
      f = sqr12(f);
      dbl_step(T, p, l);
      f = line_mul12(f, l);
      if ((K::LOOP_LOW >> b) & 1) {
        add_step(T, q, p, l);
        f = line_mul12(f, l);
      }
    }
    if constexpr (S::BN) {
      const Affine<F2> q1 = psi(q);
      Affine<F2> q2 = psi(q1);
      q2.y = fe_neg(q2.y);
      add_step(T, q1, p, l);
      f = line_mul12(f, l);
      add_step(T, q2, p, l);
      f = line_mul12(f, l);
    } else if constexpr (S::U_NEG) {
      f = conj12(f);
    }
    return f;
  }

  // ---- final exponentiation: f^(s (p^12 - 1) / r) -----------------------------------
  GM_PR_CALL static F12 final_exp(const F12& f0) {
    F12 f = mul12(conj12(f0), inv12(f0));  // p^6 - 1
    f = mul12(frob12<2>(f), f);            // p^2 + 1
    if constexpr (S::BN) {
      // l0 + l1 p + l2 p^2 + l3 p^3 with a = f^l1 = f^(12u^3 + 6u^2 + 4u):
      // l0 = l1 + 6u^2 + 2u + 1, l2 = l1 + 2u, l3 = l1 - 1
      const F12 fu = exp_u12(f);
      const F12 fu2 = exp_u12(fu);
      const F12 fu3 = exp_u12(fu2);
      const F12 t2 = cyc_sqr12(fu);
      const F12 s2v = cyc_sqr12(fu2);
      const F12 s6 = mul12(cyc_sqr12(s2v), s2v);
      const F12 v4 = cyc_sqr12(cyc_sqr12(fu3));
      F12 a = mul12(cyc_sqr12(v4), v4);          // fu3^12
      a = mul12(mul12(a, s6), cyc_sqr12(t2));
      F12 r = mul12(mul12(mul12(a, s6), t2), f);  // y0
      r = mul12(r, frob12<1>(a));
      r = mul12(r, frob12<2>(mul12(a, t2)));
      return mul12(r, frob12<3>(mul12(a, conj12(f))));
    } else {
      // (u - 1)^2 (u + p) (u^2 + p^2 - 1) + 3
      F12 a = mul12(exp_u12(f), conj12(f));
      a = mul12(exp_u12(a), conj12(a));
      const F12 b = mul12(exp_u12(a), frob12<1>(a));
      const F12 c = mul12(mul12(exp_u12(exp_u12(b)), frob12<2>(b)), conj12(b));
      return mul12(c, mul12(cyc_sqr12(f), f));
    }
  }

  // ---- memory: twelve Fp in gnark Montgomery form, gnark-crypto's E12 order ----------
  GM_DEV static F2 load2(const uint32_t* src) { return Coord<F2>::load_internal(src); }
  GM_DEV static F12 load12(const uint32_t* base, size_t i) {
    const uint32_t* s = base + i * GT_WORDS;
    constexpr int W = Coord<F2>::WORDS;
    return {{load2(s), load2(s + W), load2(s + 2 * W)}, {load2(s + 3 * W), load2(s + 4 * W), load2(s + 5 * W)}};
  }
  GM_DEV static void store12(uint32_t* base, size_t i, const F12& a) {
    uint32_t* d = base + i * GT_WORDS;
    constexpr int W = Coord<F2>::WORDS;
    Coord<F2>::store_gnark(d, a.c0.b0);
    Coord<F2>::store_gnark(d + W, a.c0.b1);
    Coord<F2>::store_gnark(d + 2 * W, a.c0.b2);
    Coord<F2>::store_gnark(d + 3 * W, a.c1.b0);
    Coord<F2>::store_gnark(d + 4 * W, a.c1.b1);
    Coord<F2>::store_gnark(d + 5 * W, a.c1.b2);
  }
};

// ---- kernels ------------------------------------------------------------------------
// One lane per pair: out[i] = the Miller value of (g1[i], g2[i]), 1 when either is infinity.
template <class C>
__global__ void __launch_bounds__(PR_TPB)
    k_pairing_miller(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2, size_t n,
                     uint32_t* __restrict__ out) {
  using T = Pr<C>;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<typename T::F1> p = load_affine_gnark<typename T::F1>(g1 + i * 2 * Coord<typename T::F1>::WORDS);
  const Affine<typename T::F2> q = load_affine_gnark<typename T::F2>(g2 + i * 2 * Coord<typename T::F2>::WORDS);
  if (aff_is_inf(p) || aff_is_inf(q)) {
    T::store12(out, i, T::one12());
    return;
  }
  T::store12(out, i, T::miller(p, q));
}

// Lane (j, t) multiplies values [16 t, min(cnt, 16 t + 16)) of product j's cnt values:
// in holds n_products x cnt values, out n_products x newcnt, newcnt = ceil(cnt / 16).
constexpr size_t PR_FAN = 16;
template <class C>
__global__ void __launch_bounds__(PR_TPB)
    k_pairing_reduce(const uint32_t* __restrict__ in, size_t n_products, size_t cnt, size_t newcnt,
                     uint32_t* __restrict__ out) {
  using T = Pr<C>;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_products * newcnt) return;
  const size_t j = idx / newcnt, t = idx % newcnt;
  const size_t lo = t * PR_FAN, hi = lo + PR_FAN < cnt ? lo + PR_FAN : cnt;
  typename T::F12 f = T::load12(in, j * cnt + lo);
#pragma unroll 1
  for (size_t q = lo + 1; q < hi; q++) f = T::mul12(f, T::load12(in, j * cnt + q));
  T::store12(out, idx, f);
}

// One lane per product: ok[j] = (f[j]^(s (p^12 - 1) / r) == 1).
template <class C>
__global__ void __launch_bounds__(PR_TPB)
    k_pairing_final(const uint32_t* __restrict__ f, size_t n, uint8_t* __restrict__ ok) {
  using T = Pr<C>;
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  ok[j] = T::eq12(T::final_exp(T::load12(f, j)), T::one12()) ? 1 : 0;
}

template <class C>
int pairing_miller_launch(gm_ctx* ctx, const void* g1_dev, const void* g2_dev, size_t n, void* f_dev) {
  if (n == 0) return GM_OK;
  ProfScope ps(ctx, "pairing_miller");
  hipLaunchKernelGGL((k_pairing_miller<C>), dim3(blocks_for(n, PR_TPB)), dim3(PR_TPB), 0, ctx->stream,
                     (const uint32_t*)g1_dev, (const uint32_t*)g2_dev, n, (uint32_t*)f_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int pairing_reduce_launch(gm_ctx* ctx, const void* in_dev, size_t n_products, size_t cnt, size_t newcnt,
                          void* out_dev) {
  if (n_products == 0) return GM_OK;
  ProfScope ps(ctx, "pairing_reduce");
  hipLaunchKernelGGL((k_pairing_reduce<C>), dim3(blocks_for(n_products * newcnt, PR_TPB)), dim3(PR_TPB), 0,
                     ctx->stream, (const uint32_t*)in_dev, n_products, cnt, newcnt, (uint32_t*)out_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int pairing_final_launch(gm_ctx* ctx, const void* f_dev, size_t n, uint8_t* ok_dev) {
  if (n == 0) return GM_OK;
  ProfScope ps(ctx, "pairing_final_exp");
  hipLaunchKernelGGL((k_pairing_final<C>), dim3(blocks_for(n, PR_TPB)), dim3(PR_TPB), 0, ctx->stream,
                     (const uint32_t*)f_dev, n, ok_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

// ---- batched Groth16 verification -------------------------------------------------------
// A proof record is {Ar G1Affine, Bs G2Affine, Krs G1Affine}; the key's arrays are
// vk_g1 = {-alpha, K[0], K[1], ...} and vk_g2 = {beta, -gamma, -delta}.
template <class C>
struct G16Rec {
  static constexpr int W1 = 2 * Coord<typename C::G1F>::WORDS, W2 = 2 * Coord<typename C::G2F>::WORDS;
  static constexpr int WORDS = 2 * W1 + W2;
  static constexpr int XW = 4 * C::Fp::NG;  // one packed XYZZ term
};
template <int N>
GM_DEV void pr_copy_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src) {
  static_assert(N % 4 == 0, "whole 16-byte words");
#pragma unroll
  for (int q = 0; q < N / 4; q++) reinterpret_cast<uint4*>(dst)[q] = reinterpret_cast<const uint4*>(src)[q];
}
template <int N>
GM_DEV void pr_zero_words(uint32_t* __restrict__ dst) {
#pragma unroll
  for (int q = 0; q < N / 4; q++) reinterpret_cast<uint4*>(dst)[q] = make_uint4(0, 0, 0, 0);
}

// One lane per proof: Ar and Krs to chk_g1[2i], [2i + 1], Bs to chk_g2[i] (the
// point check takes whole arrays).
template <class C>
__global__ void __launch_bounds__(128)
    k_g16_verify_split(const uint32_t* __restrict__ proofs, size_t m, uint32_t* __restrict__ chk_g1,
                       uint32_t* __restrict__ chk_g2) {
  using R = G16Rec<C>;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t* rec = proofs + i * R::WORDS;
  pr_copy_words<R::W1>(chk_g1 + 2 * i * R::W1, rec);
  pr_copy_words<R::W2>(chk_g2 + i * R::W2, rec + R::W1);
  pr_copy_words<R::W1>(chk_g1 + (2 * i + 1) * R::W1, rec + R::W1 + R::W2);
}

// One lane per (proof, input): terms[i][j] = [x_ij] K[j + 1], one double-and-add
// ladder over the canonical scalar; an input whose words are not below r sets
// bad_input[i] (zeroed by the host) and leaves infinity.
template <class C>
__global__ void __launch_bounds__(128)
    k_g16_verify_terms(const uint32_t* __restrict__ publics, const uint32_t* __restrict__ vk_g1, size_t m,
                       size_t nb_in, uint32_t* __restrict__ terms, uint8_t* __restrict__ bad_input) {
  using R = G16Rec<C>;
  using Fr = typename C::Fr;
  using F = typename C::G1F;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * nb_in) return;
  const size_t i = idx / nb_in, j = idx % nb_in;
  const FeG<Fr> raw = feg_load<Fr>(publics + idx * Fr::NG);
  XYZZ<F> acc = xyzz_inf<F>();
  if (!feg_below_p(raw)) {
    bad_input[i] = 1;
  } else {
    const FeG<Fr> k = fe_pack(fe_gnark_to_canonical(fe_unpack<Fr>(raw)));
    const Affine<F> base = load_affine_gnark<F>(vk_g1 + (2 + j) * R::W1);
#pragma unroll 1
    for (int w = Fr::NG - 1; w >= 0; w--) {
#pragma unroll 1
      for (int b = 31; b >= 0; b--) {
        acc = xyzz_dbl(acc);
        if ((k.w[w] >> b) & 1) xyzz_add_aff(acc, base);
      }
    }
  }
  uint32_t* t = terms + idx * R::XW;
  Coord<F>::store_packed(t, acc.x);
  Coord<F>::store_packed(t + C::Fp::NG, acc.y);
  Coord<F>::store_packed(t + 2 * C::Fp::NG, acc.zz);
  Coord<F>::store_packed(t + 3 * C::Fp::NG, acc.zzz);
}

// One lane per proof: pre[i] from the point classes and bad_input, kSum = K[0] +
// sum_j terms[i][j], and the proof's four pairs
//   (Ar, Bs) (Krs, -delta) (kSum, -gamma) (-alpha, beta);
// a proof with pre[i] != 0 gets four infinity pairs (its Miller lanes store 1).
template <class C>
__global__ void __launch_bounds__(128)
    k_g16_verify_assemble(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ vk_g1,
                          const uint32_t* __restrict__ vk_g2, const uint32_t* __restrict__ terms,
                          const uint8_t* __restrict__ st_g1, const uint8_t* __restrict__ st_g2,
                          const uint8_t* __restrict__ bad_input, size_t m, size_t nb_in, uint32_t* __restrict__ pair_g1,
                          uint32_t* __restrict__ pair_g2, uint8_t* __restrict__ pre) {
  using R = G16Rec<C>;
  using F = typename C::G1F;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t* o1 = pair_g1 + 4 * i * R::W1;
  uint32_t* o2 = pair_g2 + 4 * i * R::W2;
  const bool bad_point = (st_g1[2 * i] | st_g1[2 * i + 1] | st_g2[i]) != 0;
  const uint8_t pr = bad_point ? GM_G16_VERIFY_BAD_POINT : (bad_input[i] ? GM_G16_VERIFY_BAD_INPUT : GM_G16_VERIFY_OK);
  pre[i] = pr;
  if (pr != GM_G16_VERIFY_OK) {
    pr_zero_words<4 * R::W1>(o1);
    pr_zero_words<4 * R::W2>(o2);
    return;
  }
  XYZZ<F> acc = xyzz_inf<F>();
  xyzz_add_aff(acc, load_affine_gnark<F>(vk_g1 + R::W1));
#pragma unroll 1
  for (size_t j = 0; j < nb_in; j++) {
    const uint32_t* t = terms + (i * nb_in + j) * R::XW;
    XYZZ<F> term;
    term.x = Coord<F>::load_packed(t);
    term.y = Coord<F>::load_packed(t + C::Fp::NG);
    term.zz = Coord<F>::load_packed(t + 2 * C::Fp::NG);
    term.zzz = Coord<F>::load_packed(t + 3 * C::Fp::NG);
    acc = xyzz_add(acc, term);
  }
  Affine<F> ks;
  if (xyzz_is_inf(acc)) {
    ks.x = FOps<F>::zero();
    ks.y = FOps<F>::zero();
  } else {
    const F t = fe_inv(fe_mul(acc.zz, acc.zzz));
    ks.x = fe_mul(acc.x, fe_mul(t, acc.zzz));  // X / ZZ
    ks.y = fe_mul(acc.y, fe_mul(t, acc.zz));   // Y / ZZZ
  }
  const uint32_t* rec = proofs + i * R::WORDS;
  pr_copy_words<R::W1>(o1, rec);                               // Ar
  pr_copy_words<R::W1>(o1 + R::W1, rec + R::W1 + R::W2);       // Krs
  store_affine_gnark<F>(o1 + 2 * R::W1, ks);                   // kSum
  pr_copy_words<R::W1>(o1 + 3 * R::W1, vk_g1);                 // -alpha
  pr_copy_words<R::W2>(o2, rec + R::W1);                       // Bs
  pr_copy_words<R::W2>(o2 + R::W2, vk_g2 + 2 * R::W2);         // -delta
  pr_copy_words<R::W2>(o2 + 2 * R::W2, vk_g2 + R::W2);         // -gamma
  pr_copy_words<R::W2>(o2 + 3 * R::W2, vk_g2);                 // beta
}

template <class C>
__global__ void k_g16_verify_status(const uint8_t* __restrict__ pre, const uint8_t* __restrict__ ok, size_t m,
                                    uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  status[i] = pre[i] ? pre[i] : (ok[i] ? GM_G16_VERIFY_OK : GM_G16_VERIFY_MISMATCH);
}

template <class C, bool G2>
__global__ void k_points_negate(uint32_t* __restrict__ pts, size_t n) {
  using F = typename GroupSel<C, G2>::DF;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t* p = pts + i * 2 * Coord<F>::WORDS;
  store_affine_gnark<F>(p, aff_neg(load_affine_gnark<F>(p)));
}

template <class C>
int g16_verify_split_launch(gm_ctx* ctx, const G16VerifyDev& d) {
  ProfScope ps(ctx, "g16_verify_split");
  hipLaunchKernelGGL((k_g16_verify_split<C>), dim3(blocks_for(d.m, 128)), dim3(128), 0, ctx->stream,
                     (const uint32_t*)d.proofs, d.m, (uint32_t*)d.chk_g1, (uint32_t*)d.chk_g2);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int g16_verify_terms_launch(gm_ctx* ctx, const G16VerifyDev& d) {
  if (d.nb_in == 0) return GM_OK;
  ProfScope ps(ctx, "g16_verify_ksum_terms");
  hipLaunchKernelGGL((k_g16_verify_terms<C>), dim3(blocks_for(d.m * d.nb_in, 128)), dim3(128), 0, ctx->stream,
                     (const uint32_t*)d.publics, (const uint32_t*)d.vk_g1, d.m, d.nb_in, (uint32_t*)d.terms,
                     d.bad_input);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int g16_verify_assemble_launch(gm_ctx* ctx, const G16VerifyDev& d) {
  ProfScope ps(ctx, "g16_verify_ksum_assemble");
  hipLaunchKernelGGL((k_g16_verify_assemble<C>), dim3(blocks_for(d.m, 128)), dim3(128), 0, ctx->stream,
                     (const uint32_t*)d.proofs, (const uint32_t*)d.vk_g1, (const uint32_t*)d.vk_g2,
                     (const uint32_t*)d.terms, d.st_g1, d.st_g2, d.bad_input, d.m, d.nb_in, (uint32_t*)d.pair_g1,
                     (uint32_t*)d.pair_g2, d.pre);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int g16_verify_status_launch(gm_ctx* ctx, const uint8_t* pre_dev, const uint8_t* ok_dev, size_t m,
                             uint8_t* status_dev) {
  hipLaunchKernelGGL((k_g16_verify_status<C>), dim3(blocks_for(m, 256)), dim3(256), 0, ctx->stream, pre_dev, ok_dev,
                     m, status_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C, bool G2>
int points_negate_launch(gm_ctx* ctx, void* pts_dev, size_t n) {
  if (n == 0) return GM_OK;
  hipLaunchKernelGGL((k_points_negate<C, G2>), dim3(blocks_for(n, 64)), dim3(64), 0, ctx->stream, (uint32_t*)pts_dev,
                     n);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

#define GM_PR_INSTANTIATE(CURVE)                                                                     \
  template int pairing_miller_launch<CURVE>(gm_ctx*, const void*, const void*, size_t, void*);       \
  template int pairing_reduce_launch<CURVE>(gm_ctx*, const void*, size_t, size_t, size_t, void*);    \
  template int pairing_final_launch<CURVE>(gm_ctx*, const void*, size_t, uint8_t*);                  \
  template int g16_verify_split_launch<CURVE>(gm_ctx*, const G16VerifyDev&);                         \
  template int g16_verify_terms_launch<CURVE>(gm_ctx*, const G16VerifyDev&);                         \
  template int g16_verify_assemble_launch<CURVE>(gm_ctx*, const G16VerifyDev&);                      \
  template int g16_verify_status_launch<CURVE>(gm_ctx*, const uint8_t*, const uint8_t*, size_t, uint8_t*); \
  template int points_negate_launch<CURVE, false>(gm_ctx*, void*, size_t);                           \
  template int points_negate_launch<CURVE, true>(gm_ctx*, void*, size_t);

}  // namespace gm
