// Curve bundles tying together device field types, host field types and the
// constants each instantiation needs (BN254, BLS12-377, BLS12-381; G1 and G2),
// and the one map from a gm_curve id to its bundle (with_curve).
#pragma once
#include "curve.hpp"
#include "host_arith.hpp"

namespace gm {

struct CurveBN254 {
  static constexpr int id = 0;
  using Fr = Bn254Fr;
  using Fp = Bn254Fp;
  using G1F = Fe<Bn254Fp>;
  using G2F = Bn254Fp2;
  using HFr = host::HBnFr;
  using HFp = host::HBnFp;
  using HG1F = host::F<host::HBnFp>;
  using HG2F = host::F2<host::HBnFp, -1>;
  static constexpr int FR_BITS = 254;  // r < 2^254
  static constexpr int TWO_ADICITY = 28;
  static constexpr uint64_t COSET_GEN = 5;  // fft FrMultiplicativeGen
};

struct CurveBLS12377 {
  static constexpr int id = 1;
  using Fr = Bls377Fr;
  using Fp = Bls377Fp;
  using G1F = Fe<Bls377Fp>;
  using G2F = Bls377Fp2;
  using HFr = host::HBlsFr;
  using HFp = host::HBlsFp;
  using HG1F = host::F<host::HBlsFp>;
  using HG2F = host::F2<host::HBlsFp, -5>;
  static constexpr int FR_BITS = 253;
  static constexpr int TWO_ADICITY = 47;
  static constexpr uint64_t COSET_GEN = 22;
};

struct CurveBLS12381 {
  static constexpr int id = 2;
  using Fr = Bls381Fr;
  using Fp = Bls381Fp;
  using G1F = Fe<Bls381Fp>;
  using G2F = Bls381Fp2;
  using HFr = host::HBls381Fr;
  using HFp = host::HBls381Fp;
  using HG1F = host::F<host::HBls381Fp>;
  using HG2F = host::F2<host::HBls381Fp, -1>;
  static constexpr int FR_BITS = 255;  // the least lazy-reduction headroom: R' / r ~ 70.66
  static constexpr int TWO_ADICITY = 32;
  static constexpr uint64_t COSET_GEN = 7;
};

// ---------------------------------------------------------------------------
// Curve ids (gm_curve) -> bundles.  Every dispatch on a curve id goes through
// with_curve / with_curve01: a switch with no default branch into another
// curve's code.  An entry first runs its capability check (curve_refusal):
//   CURVES_ALL   ids 0, 1 and 2;
//   CURVES_01    ids 0 and 1; id 2 is refused with GM_ERR_UNSUPPORTED (deferred
//                entries).
// Any other id is GM_ERR_INVALID, "unknown curve id".
// ---------------------------------------------------------------------------
constexpr int CURVE_COUNT = 3;
enum CurveCaps { CURVES_01 = 0, CURVES_ALL = 1 };

template <class C>
struct CurveTag {
  using type = C;
};

// f(CurveTag<C>()) for the bundle of `curve`; `other` for an id outside 0..2
// (callers have checked the id: it is what a call with an unknown id returns).
template <class Fn>
inline auto with_curve(int curve, Fn&& f, decltype(f(CurveTag<CurveBN254>())) other)
    -> decltype(f(CurveTag<CurveBN254>())) {
  switch (curve) {
    case 0: return f(CurveTag<CurveBN254>());
    case 1: return f(CurveTag<CurveBLS12377>());
    case 2: return f(CurveTag<CurveBLS12381>());
  }
  return other;
}
// the same over the curves of the deferred entries: no BLS12-381 instantiation
template <class Fn>
inline auto with_curve01(int curve, Fn&& f, decltype(f(CurveTag<CurveBN254>())) other)
    -> decltype(f(CurveTag<CurveBN254>())) {
  switch (curve) {
    case 0: return f(CurveTag<CurveBN254>());
    case 1: return f(CurveTag<CurveBLS12377>());
  }
  return other;
}

// GM_CURVE(curve, expr): expr with C = the bundle of `curve`, GM_ERR_INVALID for
// an id outside 0..2; GM_CURVE01: over curves 0 and 1 only (deferred entries).
#define GM_CURVE(curve, ...) \
  ::gm::with_curve((curve), [&](auto tag_) { using C = typename decltype(tag_)::type; return (__VA_ARGS__); }, (int)GM_ERR_INVALID)
#define GM_CURVE01(curve, ...) \
  ::gm::with_curve01((curve), [&](auto tag_) { using C = typename decltype(tag_)::type; return (__VA_ARGS__); }, (int)GM_ERR_INVALID)

// The capability check of an entry (capi.hip): GM_OK, or the refusal with the
// error text set -- GM_ERR_INVALID "unknown curve id" outside 0..2,
// GM_ERR_UNSUPPORTED naming BLS12-381 and `entry` for id 2 under CURVES_01.
int check_curve(int curve, CurveCaps caps, const char* entry);

// per-curve sizes, by id (0 for an unknown id); fp_bytes: runtime.hpp
inline int fr_bits(int curve) {
  constexpr int t[CURVE_COUNT] = {CurveBN254::FR_BITS, CurveBLS12377::FR_BITS, CurveBLS12381::FR_BITS};
  return curve >= 0 && curve < CURVE_COUNT ? t[curve] : 0;
}
inline const char* curve_name(int curve) {
  constexpr const char* t[CURVE_COUNT] = {"BN254", "BLS12-377", "BLS12-381"};
  return curve >= 0 && curve < CURVE_COUNT ? t[curve] : "unknown curve";
}

// the non-residue of a bundle's Fp2 (G2F = Fe2<Fp, BETA>)
template <class F2>
struct Fe2Beta;
template <class P, int B>
struct Fe2Beta<Fe2<P, B>> {
  static constexpr int value = B;
};
template <class C>
struct Fp2Beta {
  static constexpr int value = Fe2Beta<typename C::G2F>::value;
};

// Select coordinate field by group.
template <class C, bool G2>
struct GroupSel;
template <class C>
struct GroupSel<C, false> {
  using DF = typename C::G1F;
  using HF = typename C::HG1F;
};
template <class C>
struct GroupSel<C, true> {
  using DF = typename C::G2F;
  using HF = typename C::HG2F;
};

}  // namespace gm
