// The point codec kernels (one lane per record) and their launchers; included by
// the per-curve units points_codec_<curve>.hip, which instantiate G1 and G2 in
// both widths.  The format is gnark-crypto's ecc/<curve>/marshal.go, restated in
// include/gnark_mi355x.h "point encodings": big-endian canonical coordinates
// (G2: A1 before A0), the flag in the top bits of the record's first byte.
//
// Decode, first class that applies: a flag that is invalid or belongs to the
// other width, or an infinity record with other bits set -> BAD_ENCODING; a
// component >= p after the flag is cleared -> NOT_REDUCED; compressed and
// x^3 + b without a root -> NO_ROOT; raw and y^2 != x^3 + b -> OFF_CURVE;
// pc_in_subgroup (points_check_impl.hpp) false -> OFF_SUBGROUP.  The last two
// are skipped under GM_DECODE_NO_SUBGROUP_CHECK.  A refused point and an infinity
// are stored as (0, 0).  An all-zero raw record is the infinity on every curve
// (gnark-crypto reads (0, 0) as the infinity), beside the BLS12 curves' flagged one.
//
// Arithmetic: canonical operands throughout (field_sqrt.hpp, points_check_impl.hpp).
#pragma once
#include "field_sqrt.hpp"
#include "points_check_impl.hpp"
#include "points_codec.hpp"

namespace gm {

constexpr unsigned CD_TPB = 128;

enum CdKind { CD_POINT = 0, CD_INF = 1, CD_BAD = 2 };

// flag bits of a curve: BN254 two (mask 0b11 << 6), the BLS12 curves three
template <class C>
struct CdFlag {
  static constexpr bool BN = PcConst<C>::BN;
  static constexpr int SHIFT = BN ? 30 : 29;  // in the top u32 word of the first coordinate
  // decode: what a record with flag f (other bits: any) is in width RAW; larger: the y asked for
  GM_DEV static CdKind kind(uint32_t f, bool raw, bool any, bool& larger) {
    larger = (f & 1) != 0;
    if constexpr (BN) {
      if (raw) return f == 0 ? (any ? CD_POINT : CD_INF) : CD_BAD;
      if (f >= 2) return CD_POINT;
      return f == 1 && !any ? CD_INF : CD_BAD;
    } else {
      if (raw) {
        if (f == 0) return any ? CD_POINT : CD_INF;
        return f == 2 && !any ? CD_INF : CD_BAD;
      }
      if (f == 4 || f == 5) return CD_POINT;
      return f == 6 && !any ? CD_INF : CD_BAD;
    }
  }
  GM_DEV static uint32_t point(bool raw, bool larger) { return raw ? 0u : ((BN ? 2u : 4u) | (larger ? 1u : 0u)); }
  GM_DEV static uint32_t infinity(bool raw) { return BN ? (raw ? 0u : 1u) : (raw ? 2u : 6u); }
};

// one big-endian coordinate component (NG u32 in memory order) <-> gnark words
template <class P>
GM_DEV FeG<P> cd_load_be(const uint32_t* __restrict__ src) {
  const FeG<P> t = feg_load<P>(src);
  FeG<P> g;
#pragma unroll
  for (int j = 0; j < P::NG; j++) g.w[j] = __builtin_bswap32(t.w[P::NG - 1 - j]);
  return g;
}
template <class P>
GM_DEV void cd_store_be(uint32_t* __restrict__ dst, const FeG<P>& g) {
  FeG<P> t;
#pragma unroll
  for (int j = 0; j < P::NG; j++) t.w[j] = __builtin_bswap32(g.w[P::NG - 1 - j]);
  feg_store<P>(dst, t);
}
template <class P>
GM_DEV FeG<P> feg_zero() {
  FeG<P> g;
#pragma unroll
  for (int j = 0; j < P::NG; j++) g.w[j] = 0;
  return g;
}

// the components of a coordinate in record order (Fp2: A1 then A0)
template <class F>
struct CdCoord;
template <class P>
struct CdCoord<Fe<P>> {
  using Base = P;
  static constexpr int NC = 1;
  GM_DEV static Fe<P>& comp(Fe<P>& a, int) { return a; }
};
template <class P, int B>
struct CdCoord<Fe2<P, B>> {
  using Base = P;
  static constexpr int NC = 2;
  GM_DEV static Fe<P>& comp(Fe2<P, B>& a, int k) { return k == 0 ? a.a1 : a.a0; }
};

template <class C, bool G2, bool RAW, class F>
GM_DEV uint32_t cd_decode(const uint32_t* __restrict__ rec, bool check, Affine<F>& p, bool& infinity) {
  using P = typename CdCoord<F>::Base;
  constexpr int NC = CdCoord<F>::NC, NCOMP = (RAW ? 2 : 1) * NC;
  FeG<P> g[NCOMP];
#pragma unroll
  for (int k = 0; k < NCOMP; k++) g[k] = cd_load_be<P>(rec + k * P::NG);
  const uint32_t f = g[0].w[P::NG - 1] >> CdFlag<C>::SHIFT;
  g[0].w[P::NG - 1] &= (1u << CdFlag<C>::SHIFT) - 1;
  uint32_t any = 0;
  bool reduced = true;
#pragma unroll
  for (int k = 0; k < NCOMP; k++) {
#pragma unroll
    for (int j = 0; j < P::NG; j++) any |= g[k].w[j];
    reduced = reduced && feg_below_p(g[k]);
  }
  bool larger;
  const CdKind kind = CdFlag<C>::kind(f, RAW, any != 0, larger);
  infinity = kind == CD_INF;
  if (kind == CD_BAD) return GM_POINT_BAD_ENCODING;
  if (kind == CD_INF) return GM_POINT_OK;
  if (!reduced) return GM_POINT_NOT_REDUCED;
#pragma unroll
  for (int k = 0; k < NC; k++) CdCoord<F>::comp(p.x, k) = fe_to_mont(fe_unpack<P>(g[k]));
  const F rhs = fe_add(fe_mul(fe_sqr(p.x), p.x), PcConst<C>::b((const F*)nullptr));
  if constexpr (RAW) {
#pragma unroll
    for (int k = 0; k < NC; k++) CdCoord<F>::comp(p.y, k) = fe_to_mont(fe_unpack<P>(g[NC + k]));
    if (!check) return GM_POINT_OK;
    if (!pc_eq(fe_sqr(p.y), rhs)) return GM_POINT_OFF_CURVE;
  } else {
    if (!fe_sqrt(rhs, p.y)) return GM_POINT_NO_ROOT;
    if (fe_is_larger(p.y) != larger) p.y = fe_neg(p.y);  // y = 0 stays 0 under either flag
    if (!check) return GM_POINT_OK;
  }
  return pc_in_subgroup<C, G2, F>(p) ? GM_POINT_OK : GM_POINT_OFF_SUBGROUP;
}

// One lane per record.  Counts and the lowest failing index as k_points_check
// reports them: one atomicAdd per wave and non-zero count, one atomicMin of
// 8 * index + class (three class bits).  Lanes past n take part in the ballots
// with nothing to report.
template <class C, bool G2, bool RAW>
__global__ void __launch_bounds__(CD_TPB)
    k_points_decode(const uint32_t* __restrict__ enc, size_t n, size_t base, uint32_t flags,
                    uint32_t* __restrict__ pts, uint8_t* __restrict__ status, unsigned long long* __restrict__ res) {
  using F = typename GroupSel<C, G2>::DF;
  using P = typename CdCoord<F>::Base;
  constexpr int NC = CdCoord<F>::NC, REC_WORDS = (RAW ? 2 : 1) * NC * P::NG;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  uint32_t cls = GM_POINT_OK;
  bool inf = false;
  if (live) {
    Affine<F> p;
    cls = cd_decode<C, G2, RAW, F>(enc + i * REC_WORDS, !(flags & GM_DECODE_NO_SUBGROUP_CHECK), p, inf);
    uint32_t* dst = pts + i * 2 * Coord<F>::WORDS;
    if (cls == GM_POINT_OK && !inf) {
      Coord<F>::store_gnark(dst, p.x);
      Coord<F>::store_gnark(dst + Coord<F>::WORDS, p.y);
    } else {
#pragma unroll
      for (int k = 0; k < 2 * NC; k++) feg_store<P>(dst + k * P::NG, feg_zero<P>());
    }
    if (status) status[i] = (uint8_t)cls;
  }
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long m_inf = __ballot(live && inf);
  const unsigned long long m_bad = __ballot(live && cls != GM_POINT_OK);
  if (m_inf && lane == (unsigned)(__ffsll((long long)m_inf) - 1))
    atomicAdd(res + CD_INFINITIES, (unsigned long long)__popcll(m_inf));
  if (m_bad) {
#pragma unroll
    for (uint32_t c = GM_POINT_NOT_REDUCED; c <= GM_POINT_NO_ROOT; c++) {
      const unsigned long long m = __ballot(live && cls == c);
      if (m && lane == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(res + c, (unsigned long long)__popcll(m));
    }
    if (lane == (unsigned)(__ffsll((long long)m_bad) - 1))
      atomicMin(res + CD_FIRST_KEY, (unsigned long long)(base + i) * 8 + cls);
  }
}

// The reverse: gnark-layout points to records.  (0, 0) becomes the infinity
// record; a point with a component >= p is counted in res[0] and written as a
// zero record.  Nothing else is checked.
template <class C, bool G2, bool RAW>
__global__ void __launch_bounds__(CD_TPB)
    k_points_encode(const uint32_t* __restrict__ pts, size_t n, uint32_t* __restrict__ enc,
                    unsigned long long* __restrict__ res) {
  using F = typename GroupSel<C, G2>::DF;
  using P = typename CdCoord<F>::Base;
  constexpr int NC = CdCoord<F>::NC, NCOMP = (RAW ? 2 : 1) * NC, REC_WORDS = NCOMP * P::NG;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  bool bad = false;
  if (live) {
    Affine<F> p;
    bool reduced = true;
    uint32_t any = 0;
    const uint32_t* src = pts + i * 2 * Coord<F>::WORDS;
    pc_load_raw(src, p.x, reduced, any);
    pc_load_raw(src + Coord<F>::WORDS, p.y, reduced, any);
    bad = !reduced;
    FeG<P> g[NCOMP];
#pragma unroll
    for (int k = 0; k < NCOMP; k++) g[k] = feg_zero<P>();
    if (reduced) {
      uint32_t f = CdFlag<C>::infinity(RAW);
      if (any) {
        bool larger = false;
#pragma unroll
        for (int k = 0; k < NC; k++) {
          g[k] = fe_pack(fe_gnark_to_canonical(CdCoord<F>::comp(p.x, k)));
          const Fe<P> yc = fe_gnark_to_canonical(CdCoord<F>::comp(p.y, k));
          // Fp2: A1 (k = 0) decides unless it is zero
          if (k == 0 || fe_is_zero(CdCoord<F>::comp(p.y, 0))) larger = fe_canonical_above_half(yc);
          if constexpr (RAW) g[NC + k] = fe_pack(yc);
        }
        f = CdFlag<C>::point(RAW, larger);
      }
      g[0].w[P::NG - 1] |= f << CdFlag<C>::SHIFT;
    }
#pragma unroll
    for (int k = 0; k < NCOMP; k++) cd_store_be<P>(enc + i * REC_WORDS + k * P::NG, g[k]);
  }
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(live && bad);
  if (m && lane == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(res, (unsigned long long)__popcll(m));
}

template <class C, bool G2>
int points_decode_launch(gm_ctx* ctx, const void* enc_dev, size_t n, size_t base, bool raw, unsigned flags,
                         void* points_dev, uint8_t* status_dev, unsigned long long* res_dev) {
  if (n == 0) return GM_OK;
  ProfScope ps(ctx, G2 ? (raw ? "points_decode_raw_g2" : "points_decode_g2")
                       : (raw ? "points_decode_raw_g1" : "points_decode_g1"));
  const dim3 grid(blocks_for(n, CD_TPB)), block(CD_TPB);
  if (raw)
    hipLaunchKernelGGL((k_points_decode<C, G2, true>), grid, block, 0, ctx->stream, (const uint32_t*)enc_dev, n, base,
                       (uint32_t)flags, (uint32_t*)points_dev, status_dev, res_dev);
  else
    hipLaunchKernelGGL((k_points_decode<C, G2, false>), grid, block, 0, ctx->stream, (const uint32_t*)enc_dev, n, base,
                       (uint32_t)flags, (uint32_t*)points_dev, status_dev, res_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

template <class C, bool G2>
int points_encode_launch(gm_ctx* ctx, const void* points_dev, size_t n, bool raw, void* enc_dev,
                         unsigned long long* res_dev) {
  if (n == 0) return GM_OK;
  ProfScope ps(ctx, G2 ? (raw ? "points_encode_raw_g2" : "points_encode_g2")
                       : (raw ? "points_encode_raw_g1" : "points_encode_g1"));
  const dim3 grid(blocks_for(n, CD_TPB)), block(CD_TPB);
  if (raw)
    hipLaunchKernelGGL((k_points_encode<C, G2, true>), grid, block, 0, ctx->stream, (const uint32_t*)points_dev, n,
                       (uint32_t*)enc_dev, res_dev);
  else
    hipLaunchKernelGGL((k_points_encode<C, G2, false>), grid, block, 0, ctx->stream, (const uint32_t*)points_dev, n,
                       (uint32_t*)enc_dev, res_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

#define GM_CD_INSTANTIATE(CURVE)                                                                                   \
  template int points_decode_launch<CURVE, false>(gm_ctx*, const void*, size_t, size_t, bool, unsigned, void*,     \
                                                  uint8_t*, unsigned long long*);                                  \
  template int points_decode_launch<CURVE, true>(gm_ctx*, const void*, size_t, size_t, bool, unsigned, void*,      \
                                                 uint8_t*, unsigned long long*);                                   \
  template int points_encode_launch<CURVE, false>(gm_ctx*, const void*, size_t, bool, void*, unsigned long long*); \
  template int points_encode_launch<CURVE, true>(gm_ctx*, const void*, size_t, bool, void*, unsigned long long*);

}  // namespace gm
