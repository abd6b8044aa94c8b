// The kernels of batched KZG and PLONK verification; included by the per-curve
// units plonk_verify_<curve>.hip, which instantiate the launchers.
//
// PLONK (backend/plonk/bn254/verify.go:128-322 with kzg.FoldProof and
// kzg.BatchVerifyMultiPoints unrolled): with the caller's challenges gamma, beta,
// alpha, zeta, the folding challenge v and the multiplier u of the second opening,
//   A = [l] Ql + [r] Qr + [l r] Qm + [o] Qo + Qk + [_s1] S3 + [coeffZ + u] Z
//       + sum_j [qcp_j(zeta)] Bsb_j - zh ([1] H0 + [zeta^(n+2)] H1 + [zeta^(2(n+2))] H2)
//       + [v] L + [v^2] R + [v^3] O + [v^4] S1 + [v^5] S2 + sum_j [v^(6+j)] Qcp_j
//       - [y + u zu] G + [zeta] Hb + [u w zeta] Hz,           y = sum_i v^i claimed_i
//   B = Hb + [u] Hz
// and the proof is accepted when constLin = claimed_0 and e(A, G2[0]) e(B, -G2[1]) = 1.
//
// Fr arithmetic: fully reduced operands throughout (fe_mul / fe_sqr / fe_add /
// fe_sub of field.hpp), internal form, so fe_eq and fe_is_zero on limbs decide in
// the field on all three curves.  fe_inv sends 0 to 0, gnark's convention.
#pragma once
#include "pairing_impl.hpp"
#include "plonk_verify.hpp"

namespace gm {

template <class F>
GM_DEV XYZZ<F> pv_load_xyzz(const uint32_t* __restrict__ t) {
  constexpr int W = Coord<F>::WORDS;
  XYZZ<F> r;
  r.x = Coord<F>::load_packed(t);
  r.y = Coord<F>::load_packed(t + W);
  r.zz = Coord<F>::load_packed(t + 2 * W);
  r.zzz = Coord<F>::load_packed(t + 3 * W);
  return r;
}
template <class F>
GM_DEV void pv_store_xyzz(uint32_t* __restrict__ t, const XYZZ<F>& a) {
  constexpr int W = Coord<F>::WORDS;
  Coord<F>::store_packed(t, a.x);
  Coord<F>::store_packed(t + W, a.y);
  Coord<F>::store_packed(t + 2 * W, a.zz);
  Coord<F>::store_packed(t + 3 * W, a.zzz);
}

// [k] base by double-and-add over the canonical value of the gnark-form scalar
template <class C>
GM_DEV XYZZ<typename C::G1F> pv_ladder(const Affine<typename C::G1F>& base, const Fe<typename C::Fr>& k_gnark) {
  using Fr = typename C::Fr;
  using F = typename C::G1F;
  const FeG<Fr> k = fe_pack(fe_gnark_to_canonical(k_gnark));
  XYZZ<F> acc = xyzz_inf<F>();
#pragma unroll 1
  for (int w = Fr::NG - 1; w >= 0; w--) {
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      acc = xyzz_dbl(acc);
      if ((k.w[w] >> b) & 1) xyzz_add_aff(acc, base);
    }
  }
  return acc;
}

// a and b to affine form with one inversion between them; infinity is (0, 0)
template <class F>
GM_DEV void pv_to_affine2(const XYZZ<F>& a, const XYZZ<F>& b, Affine<F>& oa, Affine<F>& ob) {
  const bool ia = xyzz_is_inf(a), ib = xyzz_is_inf(b);
  const F da = ia ? FOps<F>::one() : fe_mul(a.zz, a.zzz);
  const F db = ib ? FOps<F>::one() : fe_mul(b.zz, b.zzz);
  const F inv = fe_inv(fe_mul(da, db));
  const F ta = fe_mul(inv, db), tb = fe_mul(inv, da);
  oa.x = ia ? FOps<F>::zero() : fe_mul(a.x, fe_mul(ta, a.zzz));  // X / ZZ
  oa.y = ia ? FOps<F>::zero() : fe_mul(a.y, fe_mul(ta, a.zz));   // Y / ZZZ
  ob.x = ib ? FOps<F>::zero() : fe_mul(b.x, fe_mul(tb, b.zzz));
  ob.y = ib ? FOps<F>::zero() : fe_mul(b.y, fe_mul(tb, b.zz));
}

// ---- PLONK: the verifier's scalars ---------------------------------------------------
// One lane per proof.  Writes the proof's pv_terms scalars (gnark form) in the order
// of the ladders,
//   key:    G -(y + u zu), Ql l, Qr r, Qm l r, Qo o, S3 _s1, S1 v^4, S2 v^5, Qcp_j v^(6+j)
//   proof:  L v, R v^2, O v^3, Z coeffZ + u, H0 -zh, H1 -zeta^(n+2) zh, H2 -zeta^(2(n+2)) zh,
//           Hb zeta, Hz u w zeta, Bsb_j qcp_j(zeta)
//   last:   u (the ladder [u] Hz of B)
// PI(zeta) and constLin to aux, and pre[i]: BAD_POINT if st_g1 classes one of the
// proof's points bad, else BAD_INPUT if an Fr word string of the proof is not below r
// or u = 0, else ALGEBRAIC if constLin != claimed_0, else 0.
// The nb_public + nb_bsb + 1 denominators zeta - w^k, zeta - w^row_j and zeta - 1 are
// inverted together (fr.BatchInvert: one inversion, zeros left zero); the prefix
// products lie in d.prefix, element k of proof i at [k m + i].
template <class C>
__global__ void __launch_bounds__(64) k_pv_scalars(PvDev d) {
  using Fr = typename C::Fr;
  using E = Fe<Fr>;
  constexpr int NG = Fr::NG;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.m) return;
  const size_t nb = d.nb_bsb, nbp = d.nb_public, NV = pv_values(nb), T = pv_terms(nb), NP = pv_proof_points(nb);
  bool bad = false;
  auto ld = [&](const void* base, size_t idx) -> E {
    const FeG<Fr> g = feg_load<Fr>((const uint32_t*)base + idx * NG);
    if (!feg_below_p(g)) {
      bad = true;
      return fe_zero<Fr>();
    }
    return fe_to_internal(fe_unpack<Fr>(g));
  };
  auto key = [&](size_t idx) -> E { return fe_to_internal(fe_load_g<Fr>(d.key_fr, idx)); };
  const E one = fe_one<Fr>();
  const E gamma = ld(d.chal, 6 * i), beta = ld(d.chal, 6 * i + 1), alpha = ld(d.chal, 6 * i + 2),
          zeta = ld(d.chal, 6 * i + 3), v = ld(d.chal, 6 * i + 4), u = ld(d.chal, 6 * i + 5);
  const size_t v0 = NV * i;
  const E lin = ld(d.values, v0), l = ld(d.values, v0 + 1), r = ld(d.values, v0 + 2), o = ld(d.values, v0 + 3),
          s1 = ld(d.values, v0 + 4), s2 = ld(d.values, v0 + 5), zu = ld(d.values, v0 + 6 + nb);
  const E size_inv = key(0), omega = key(1), omega_inv = key(2), shift = key(3);

  E zn = zeta;
#pragma unroll 1
  for (uint32_t q = 0; q < d.logn; q++) zn = fe_sqr(zn);
  const E zh = fe_sub(zn, one);

  // forward: the prefix products over the non-zero denominators
  E* const pre = reinterpret_cast<E*>(d.prefix);
  E acc = one, w = one;
#pragma unroll 1
  for (size_t k = 0; k < nbp; k++) {
    const E den = fe_sub(zeta, w);
    if (!fe_is_zero(den)) {
      pre[k * d.m + i] = acc;
      acc = fe_mul(acc, den);
    }
    w = fe_mul(w, omega);
  }
#pragma unroll 1
  for (size_t j = 0; j < nb; j++) {
    const E den = fe_sub(zeta, key(PV_KEY_FR + j));
    if (!fe_is_zero(den)) {
      pre[(nbp + j) * d.m + i] = acc;
      acc = fe_mul(acc, den);
    }
  }
  {
    const E den = fe_sub(zeta, one);
    if (!fe_is_zero(den)) {
      pre[(nbp + nb) * d.m + i] = acc;
      acc = fe_mul(acc, den);
    }
  }
  E inv = fe_inv(acc);
  // backward: each inverse, used where it falls
  E lag0 = fe_zero<Fr>();  // L1(zeta) = (zeta^n - 1) / (n (zeta - 1))
  {
    const E den = fe_sub(zeta, one);
    if (!fe_is_zero(den)) {
      lag0 = fe_mul(fe_mul(fe_mul(inv, pre[(nbp + nb) * d.m + i]), zh), size_inv);
      inv = fe_mul(inv, den);
    }
  }
  E pi = fe_zero<Fr>();  // sum of x_k w^k / (zeta - w^k); zh / n is multiplied in once below
#pragma unroll 1
  for (size_t j = nb; j-- > 0;) {
    const E wr = key(PV_KEY_FR + j);
    const E den = fe_sub(zeta, wr);
    const E h = ld(d.hashed, nb * i + j);
    if (!fe_is_zero(den)) {
      pi = fe_add(pi, fe_mul(fe_mul(h, wr), fe_mul(inv, pre[(nbp + j) * d.m + i])));
      inv = fe_mul(inv, den);
    }
  }
#pragma unroll 1
  for (size_t k = nbp; k-- > 0;) {
    w = fe_mul(w, omega_inv);  // w^k
    const E den = fe_sub(zeta, w);
    const E x = ld(d.publics, nbp * i + k);
    if (!fe_is_zero(den)) {
      pi = fe_add(pi, fe_mul(fe_mul(x, w), fe_mul(inv, pre[k * d.m + i])));
      inv = fe_mul(inv, den);
    }
  }
  pi = fe_mul(pi, fe_mul(zh, size_inv));

  // verify.go:205-221
  const E a2l = fe_mul(fe_mul(lag0, alpha), alpha);
  const E p12 = fe_mul(fe_add(fe_add(fe_mul(beta, s1), gamma), l), fe_add(fe_add(fe_mul(s2, beta), gamma), r));
  const E azu = fe_mul(alpha, zu);
  E const_lin = fe_mul(fe_mul(fe_add(o, gamma), p12), azu);
  const_lin = fe_neg(fe_add(fe_sub(const_lin, a2l), pi));
  const bool algebraic = !fe_eq(const_lin, lin);
  // :238-265
  const E s1c = fe_mul(fe_mul(p12, beta), azu);
  const E bz = fe_mul(beta, zeta), bgz = fe_mul(bz, shift), bggz = fe_mul(bgz, shift);
  E s2c = fe_mul(fe_add(fe_add(bz, gamma), l), fe_add(fe_add(bgz, gamma), r));
  s2c = fe_neg(fe_mul(fe_mul(s2c, fe_add(fe_add(bggz, o), gamma)), alpha));
  const E coeff_z = fe_add(a2l, s2c);
  const E znp2 = fe_mul(zn, fe_sqr(zeta));
  const E h1 = fe_mul(znp2, zh), h2 = fe_mul(znp2, h1);

  uint32_t* const out = (uint32_t*)d.scal + i * T * NG;
  auto st = [&](size_t t, const E& x) { feg_store<Fr>(out + t * NG, fe_pack(fe_to_gnark(x))); };
  const size_t P0 = PV_KEY_LADDERS + nb;
  st(1, l);
  st(2, r);
  st(3, fe_mul(l, r));
  st(4, o);
  st(5, s1c);
  // y = sum_i v^i claimed_i, the powers stored where they are scalars
  E y = lin, vp = v;
  st(P0 + 0, vp);
  y = fe_add(y, fe_mul(vp, l));
  vp = fe_mul(vp, v);
  st(P0 + 1, vp);
  y = fe_add(y, fe_mul(vp, r));
  vp = fe_mul(vp, v);
  st(P0 + 2, vp);
  y = fe_add(y, fe_mul(vp, o));
  vp = fe_mul(vp, v);
  st(6, vp);
  y = fe_add(y, fe_mul(vp, s1));
  vp = fe_mul(vp, v);
  st(7, vp);
  y = fe_add(y, fe_mul(vp, s2));
#pragma unroll 1
  for (size_t j = 0; j < nb; j++) {
    const E q = ld(d.values, v0 + 6 + j);
    vp = fe_mul(vp, v);
    st(PV_KEY_LADDERS + j, vp);
    y = fe_add(y, fe_mul(vp, q));
    st(P0 + PV_PROOF_POINTS + j, q);
  }
  st(0, fe_neg(fe_add(y, fe_mul(u, zu))));
  st(P0 + 3, fe_add(coeff_z, u));
  st(P0 + 4, fe_neg(zh));
  st(P0 + 5, fe_neg(h1));
  st(P0 + 6, fe_neg(h2));
  st(P0 + 7, zeta);
  st(P0 + 8, fe_mul(fe_mul(u, omega), zeta));
  st(T - 1, u);
  feg_store<Fr>((uint32_t*)d.aux + (2 * i) * NG, fe_pack(fe_to_gnark(pi)));
  feg_store<Fr>((uint32_t*)d.aux + (2 * i + 1) * NG, fe_pack(fe_to_gnark(const_lin)));

  if (fe_is_zero(u)) bad = true;
  uint8_t cls = bad ? GM_PLONK_VERIFY_BAD_INPUT : (algebraic ? GM_PLONK_VERIFY_ALGEBRAIC : GM_PLONK_VERIFY_OK);
  if (d.st_g1) {
    uint8_t any = 0;
#pragma unroll 1
    for (size_t q = 0; q < NP; q++) any |= d.st_g1[i * NP + q];
    if (any) cls = GM_PLONK_VERIFY_BAD_POINT;
  }
  d.pre[i] = cls;
}

// One lane per (proof, ladder): terms[i][t] = [scal[i][t]] base(i, t); the base is
// the key's point t, the proof's point t - (8 + nb_bsb), or Hz for the last ladder.
// A proof with pre[i] != 0 is skipped: its terms are never read.
template <class C>
__global__ void __launch_bounds__(128) k_pv_terms(PvDev d) {
  using Fr = typename C::Fr;
  using F = typename C::G1F;
  constexpr int W1 = 2 * Coord<F>::WORDS, XW = 4 * Coord<F>::WORDS;
  const size_t nb = d.nb_bsb, T = pv_terms(nb), NP = pv_proof_points(nb), NK = PV_KEY_LADDERS + nb;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= d.m * T) return;
  const size_t i = idx / T, t = idx % T;
  if (d.pre[i]) return;
  const uint32_t* bp = t < NK ? (const uint32_t*)d.key_g1 + t * W1
                              : (const uint32_t*)d.points + (i * NP + (t < NK + NP ? t - NK : PV_HZ)) * W1;
  const XYZZ<F> acc = pv_ladder<C>(load_affine_gnark<F>(bp), fe_load_g<Fr>(d.scal, idx));
  pv_store_xyzz<F>((uint32_t*)d.terms + idx * XW, acc);
}

// One lane per proof: A = Qk + the first pv_terms - 1 terms, B = Hb + the last, both
// to affine form with one inversion, and the proof's pairs (A, G2[0]) (B, -G2[1]);
// a proof with pre[i] != 0 gets two infinity pairs (its Miller lanes store 1).
template <class C>
__global__ void __launch_bounds__(128) k_pv_assemble(PvDev d) {
  using F = typename C::G1F;
  constexpr int W1 = 2 * Coord<F>::WORDS, W2 = 2 * Coord<typename C::G2F>::WORDS, XW = 4 * Coord<F>::WORDS;
  const size_t nb = d.nb_bsb, T = pv_terms(nb), NP = pv_proof_points(nb), NK = PV_KEY_LADDERS + nb;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.m) return;
  uint32_t* o1 = (uint32_t*)d.pair_g1 + 2 * i * W1;
  uint32_t* o2 = (uint32_t*)d.pair_g2 + 2 * i * W2;
  if (d.pre[i]) {
    pr_zero_words<2 * W1>(o1);
    pr_zero_words<2 * W2>(o2);
    return;
  }
  const uint32_t* terms = (const uint32_t*)d.terms + i * T * XW;
  XYZZ<F> a = xyzz_inf<F>();
  xyzz_add_aff(a, load_affine_gnark<F>((const uint32_t*)d.key_g1 + NK * W1));  // Qk
#pragma unroll 1
  for (size_t t = 0; t + 1 < T; t++) a = xyzz_add(a, pv_load_xyzz<F>(terms + t * XW));
  XYZZ<F> b = pv_load_xyzz<F>(terms + (T - 1) * XW);
  xyzz_add_aff(b, load_affine_gnark<F>((const uint32_t*)d.points + (i * NP + PV_HZ - 1) * W1));  // Hb
  Affine<F> pa, pb;
  pv_to_affine2(a, b, pa, pb);
  store_affine_gnark<F>(o1, pa);
  store_affine_gnark<F>(o1 + W1, pb);
  pr_copy_words<2 * W2>(o2, (const uint32_t*)d.key_g2);
}

// ---- KZG --------------------------------------------------------------------------------
// One lane per (opening, ladder).  Per opening: [y] G and [z] H.  Folded: [lambda y] G,
// [lambda z] H, [lambda] C, [lambda] H, lambda = 1 for the batch's opening 0.  Fr
// words not below r, and a zero lambda other than the batch's first, set
// bad_input[i] (zeroed by the host) and leave infinity.
template <class C, bool FOLD>
__global__ void __launch_bounds__(128) k_kzgv_terms(KzgvDev d) {
  using Fr = typename C::Fr;
  using F = typename C::G1F;
  constexpr int W1 = 2 * Coord<F>::WORDS, XW = 4 * Coord<F>::WORDS, L = FOLD ? 4 : 2;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= d.m * L) return;
  const size_t i = idx / L, j = idx % L;
  const FeG<Fr> zr = feg_load<Fr>((const uint32_t*)d.z + i * Fr::NG), yr = feg_load<Fr>((const uint32_t*)d.y + i * Fr::NG);
  bool bad = !feg_below_p(zr) || !feg_below_p(yr);
  Fe<Fr> k = fe_unpack<Fr>(j == 0 ? yr : zr);  // gnark form
  if constexpr (FOLD) {
    const bool forced = d.first && i == 0;
    const FeG<Fr> lr = feg_load<Fr>((const uint32_t*)d.lambda + i * Fr::NG);
    if (!forced) {
      const Fe<Fr> lam = fe_unpack<Fr>(lr);
      bad = bad || !feg_below_p(lr) || fe_is_zero(lam);
      // gnark form times internal form is gnark form
      k = j < 2 ? fe_mul(k, fe_to_internal(lam)) : lam;
    } else if (j >= 2) {
      k = fe_to_gnark(fe_one<Fr>());
    }
  }
  XYZZ<F> acc = xyzz_inf<F>();
  if (bad) {
    d.bad_input[i] = 1;
  } else {
    const uint32_t* bp = j == 0 ? (const uint32_t*)d.key_g1
                                : (const uint32_t*)(j == 2 ? d.digests : d.proofs) + i * W1;
    acc = pv_ladder<C>(load_affine_gnark<F>(bp), k);
  }
  pv_store_xyzz<F>((uint32_t*)d.terms + idx * XW, acc);
}

// One lane per opening: pre[i] from the point classes and bad_input, and
//   per opening: the pairs (C - [y] G + [z] H, G2[0]) (H, -G2[1]), infinity pairs when pre[i] != 0;
//   folded: part[1 + i] = ([lambda] C - [lambda y] G + [lambda z] H, [lambda] H), infinities when pre[i] != 0.
template <class C, bool FOLD>
__global__ void __launch_bounds__(128) k_kzgv_assemble(KzgvDev d) {
  using F = typename C::G1F;
  constexpr int W1 = 2 * Coord<F>::WORDS, W2 = 2 * Coord<typename C::G2F>::WORDS, XW = 4 * Coord<F>::WORDS,
                L = FOLD ? 4 : 2;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.m) return;
  const bool bad_point = (d.st_c[i] | d.st_h[i]) != 0;
  const uint8_t pr = bad_point ? GM_KZG_VERIFY_BAD_POINT : (d.bad_input[i] ? GM_KZG_VERIFY_BAD_INPUT : GM_KZG_VERIFY_OK);
  d.pre[i] = pr;
  const uint32_t* terms = (const uint32_t*)d.terms + i * L * XW;
  if constexpr (FOLD) {
    uint32_t* out = (uint32_t*)d.part + (1 + i) * 2 * XW;
    if (pr) {
      pr_zero_words<2 * XW>(out);
      return;
    }
    XYZZ<F> t0 = pv_load_xyzz<F>(terms);
    t0.y = fe_neg(t0.y);
    const XYZZ<F> a = xyzz_add(xyzz_add(pv_load_xyzz<F>(terms + 2 * XW), t0), pv_load_xyzz<F>(terms + XW));
    pv_store_xyzz<F>(out, a);
    pr_copy_words<XW>(out + XW, terms + 3 * XW);
  } else {
    uint32_t* o1 = (uint32_t*)d.pair_g1 + 2 * i * W1;
    uint32_t* o2 = (uint32_t*)d.pair_g2 + 2 * i * W2;
    if (pr) {
      pr_zero_words<2 * W1>(o1);
      pr_zero_words<2 * W2>(o2);
      return;
    }
    XYZZ<F> t0 = pv_load_xyzz<F>(terms);
    t0.y = fe_neg(t0.y);
    XYZZ<F> a = xyzz_add(t0, pv_load_xyzz<F>(terms + XW));
    xyzz_add_aff(a, load_affine_gnark<F>((const uint32_t*)d.digests + i * W1));
    Affine<F> pa, unused;
    pv_to_affine2(a, xyzz_inf<F>(), pa, unused);
    store_affine_gnark<F>(o1, pa);
    pr_copy_words<W1>(o1 + W1, (const uint32_t*)d.proofs + i * W1);
    pr_copy_words<2 * W2>(o2, (const uint32_t*)d.key_g2);
  }
}

// Lane t sums pairs [16 t, min(cnt, 16 t + 16)) of (A, B) partial sums.
template <class C>
__global__ void __launch_bounds__(128)
    k_kzgv_sum(const uint32_t* __restrict__ in, size_t cnt, size_t newcnt, uint32_t* __restrict__ out) {
  using F = typename C::G1F;
  constexpr int XW = 4 * Coord<F>::WORDS;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= newcnt) return;
  const size_t lo = t * PR_FAN, hi = lo + PR_FAN < cnt ? lo + PR_FAN : cnt;
  XYZZ<F> a = pv_load_xyzz<F>(in + lo * 2 * XW), b = pv_load_xyzz<F>(in + lo * 2 * XW + XW);
#pragma unroll 1
  for (size_t q = lo + 1; q < hi; q++) {
    a = xyzz_add(a, pv_load_xyzz<F>(in + q * 2 * XW));
    b = xyzz_add(b, pv_load_xyzz<F>(in + q * 2 * XW + XW));
  }
  pv_store_xyzz<F>(out + t * 2 * XW, a);
  pv_store_xyzz<F>(out + t * 2 * XW + XW, b);
}

// One lane: the folded sums to the pairs (A, G2[0]) (B, -G2[1]).
template <class C>
__global__ void k_kzgv_fold_pairs(const uint32_t* __restrict__ sum, const uint32_t* __restrict__ key_g2,
                                  uint32_t* __restrict__ pair_g1, uint32_t* __restrict__ pair_g2) {
  using F = typename C::G1F;
  constexpr int W1 = 2 * Coord<F>::WORDS, W2 = 2 * Coord<typename C::G2F>::WORDS, XW = 4 * Coord<F>::WORDS;
  if (blockIdx.x || threadIdx.x) return;
  Affine<F> pa, pb;
  pv_to_affine2(pv_load_xyzz<F>(sum), pv_load_xyzz<F>(sum + XW), pa, pb);
  store_affine_gnark<F>(pair_g1, pa);
  store_affine_gnark<F>(pair_g1 + W1, pb);
  pr_copy_words<2 * W2>(pair_g2, key_g2);
}

// ---- launchers ------------------------------------------------------------------------------
template <class C>
int pv_scalars_launch(gm_ctx* ctx, const PvDev& d) {
  ProfScope ps(ctx, "plonk_verify_scalars");
  hipLaunchKernelGGL((k_pv_scalars<C>), dim3(blocks_for(d.m, 64)), dim3(64), 0, ctx->stream, d);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int pv_terms_launch(gm_ctx* ctx, const PvDev& d) {
  ProfScope ps(ctx, "plonk_verify_terms");
  hipLaunchKernelGGL((k_pv_terms<C>), dim3(blocks_for(d.m * pv_terms(d.nb_bsb), 128)), dim3(128), 0, ctx->stream, d);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int pv_assemble_launch(gm_ctx* ctx, const PvDev& d) {
  ProfScope ps(ctx, "plonk_verify_assemble");
  hipLaunchKernelGGL((k_pv_assemble<C>), dim3(blocks_for(d.m, 128)), dim3(128), 0, ctx->stream, d);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int kzgv_terms_launch(gm_ctx* ctx, const KzgvDev& d, bool fold) {
  ProfScope ps(ctx, "kzg_verify_terms");
  if (fold)
    hipLaunchKernelGGL((k_kzgv_terms<C, true>), dim3(blocks_for(d.m * 4, 128)), dim3(128), 0, ctx->stream, d);
  else
    hipLaunchKernelGGL((k_kzgv_terms<C, false>), dim3(blocks_for(d.m * 2, 128)), dim3(128), 0, ctx->stream, d);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int kzgv_assemble_launch(gm_ctx* ctx, const KzgvDev& d, bool fold) {
  ProfScope ps(ctx, "kzg_verify_assemble");
  if (fold)
    hipLaunchKernelGGL((k_kzgv_assemble<C, true>), dim3(blocks_for(d.m, 128)), dim3(128), 0, ctx->stream, d);
  else
    hipLaunchKernelGGL((k_kzgv_assemble<C, false>), dim3(blocks_for(d.m, 128)), dim3(128), 0, ctx->stream, d);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int kzgv_sum_launch(gm_ctx* ctx, const void* in_dev, size_t cnt, size_t newcnt, void* out_dev) {
  hipLaunchKernelGGL((k_kzgv_sum<C>), dim3(blocks_for(newcnt, 128)), dim3(128), 0, ctx->stream,
                     (const uint32_t*)in_dev, cnt, newcnt, (uint32_t*)out_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class C>
int kzgv_fold_pairs_launch(gm_ctx* ctx, const void* sum_dev, const void* key_g2, void* pair_g1, void* pair_g2) {
  hipLaunchKernelGGL((k_kzgv_fold_pairs<C>), dim3(1), dim3(64), 0, ctx->stream, (const uint32_t*)sum_dev,
                     (const uint32_t*)key_g2, (uint32_t*)pair_g1, (uint32_t*)pair_g2);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

#define GM_PV_INSTANTIATE(CURVE)                                                            \
  template int pv_scalars_launch<CURVE>(gm_ctx*, const PvDev&);                             \
  template int pv_terms_launch<CURVE>(gm_ctx*, const PvDev&);                               \
  template int pv_assemble_launch<CURVE>(gm_ctx*, const PvDev&);                            \
  template int kzgv_terms_launch<CURVE>(gm_ctx*, const KzgvDev&, bool);                     \
  template int kzgv_assemble_launch<CURVE>(gm_ctx*, const KzgvDev&, bool);                  \
  template int kzgv_sum_launch<CURVE>(gm_ctx*, const void*, size_t, size_t, void*);         \
  template int kzgv_fold_pairs_launch<CURVE>(gm_ctx*, const void*, const void*, void*, void*);

}  // namespace gm
