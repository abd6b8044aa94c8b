// MSM entry points (see msm_impl.hpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include "curves.hpp"

struct gm_ctx;
struct gm_msm_pending;

namespace gm {
struct Arena;
// Counting sort of the MSM digits (msm_impl.hpp k_msm_digits, msm_sort.hip).
// T buckets; coarse bin H = bucket >> F (NC bins, ~2K entries each for uniform
// digits, finished in LDS); pass-1 bin = bucket >> (F + G) (NS bins).  G = 0:
// two levels; G > 0: a middle pass splits each of the NS super-bins into its
// 2^G coarse bins (large MSMs).  M = upper bound on the entries.  Coarse bins
// above S2_BIG entries are split into parts.
// Between the passes an entry is 8 bytes (bucket, value), or -- `compact` -- one
// 32-bit word: the low kb = F + G bits of the bucket (its pass-1 bin gives the
// rest), the point index and the sign.  sort_compact_fits is the rule; the
// plan applies it once (msm_plan; GM_MSM_SORT_WIDE=1 forces 8 bytes).
constexpr uint32_t S2_BIG = 1u << 16;
constexpr uint32_t S2_STAGE = 6144;  // bins up to this many entries are sorted in LDS
struct SortGeom {
  uint32_t T = 0, F = 0, G = 0, NC = 0, NS = 0;
  size_t M = 0;
  bool compact = false;
};
// kb + vb <= 32, vb = 1 (sign) + the bits of the largest value, npts - 1
inline bool sort_compact_fits(uint32_t F, uint32_t G, size_t npts) {
  uint32_t vb = 1;
  while (npts && ((npts - 1) >> (vb - 1))) vb++;
  return F + G + vb <= 32;
}
// Digits (k_msm_digits output: window-major, plus the pass-1 bin counts
// `scount`, NS words) -> sorted values, offsets[0..T] and, unless keys_out is
// null, the sorted keys.  Scratch comes from `arena`.
int msm_sort_digits(gm_ctx* ctx, Arena& arena, const SortGeom& g, size_t n, uint32_t W, uint32_t nb,
                    uint32_t shared_stride, const uint32_t* dig, const uint32_t* scount, uint32_t* keys_out,
                    uint32_t* vals_out, uint32_t* offsets);

// Fixed-base precomputation of a resident point set (a proving key's arrays):
// W copies of the n points, copy w = [2^(c w)] P_i at index w * stride + i, so
// every window's digits land in ONE shared set of 2^(c-1) buckets.  The
// accumulation work is unchanged (one mixed add per non-zero digit), but the
// bucket reduction runs once instead of W times, which lets c grow (fewer
// windows).  c == 0 means plain points (no precomputation).
// Version of the precomputed-copy rule below (part of the device-layout cache
// fingerprint, pk_io.hip): bump when the copies' content or order changes.
// Layout 2: the last `narrow` windows are c - 1 bits wide so that the windows
// cover exactly bits + 1 bits: with one shared bucket set, a narrow TOP window
// (e.g. 13 of 22 bits at 2^24) would pile n / 2^12 entries on each of the
// lowest 2^12 buckets (long slice spans, tree fixups, hot sort bins); spreading
// the excess one bit per window keeps every bucket within ~2x of the mean.
constexpr uint32_t PRECOMP_LAYOUT = 2;
struct MsmPrecomp {
  uint32_t c = 0, W = 0;
  uint32_t narrow = 0;  // windows W - narrow .. W - 1 are c - 1 bits wide
  size_t stride = 0;
};
// narrow windows of a (c, W) layout over `bits`-bit scalars: c W - narrow =
// bits + 1 (signed digits), at least one full-width window
inline uint32_t precomp_narrow(uint32_t c, uint32_t W, int bits) {
  const long long e = (long long)c * W - (bits + 1);
  if (e <= 0) return 0;
  return (uint32_t)(e < (long long)W - 1 ? e : (long long)W - 1);
}

// Window size and copy count for a precomputed set of n points of a
// `bits`-bit scalar field: minimises n*W accumulation adds + ~3 adds per bucket.
MsmPrecomp msm_choose_precomp(size_t n, int bits);

// ---------------------------------------------------------------------------
// Derived geometry of one MSM, as host functions of the sizes alone: the driver
// (msm_plan, msm_launch, msm_reduce in msm_impl.hpp) calls them, and so does the
// host-only report gm_test_msm_geometry (testhooks.hip), which needs no device.
// ---------------------------------------------------------------------------
// Window size minimising a cost model in EC adds: n*W accumulation adds plus
// ~3 adds per bucket in the reduction (W*2^(c-1) buckets), W = ceil((bits+1)/c).
// Picks c = 16 for 2^20 BN254 points, 20 for 2^24, and c = 17 (W = 15, a full top
// window) instead of 18 for 2^22 BLS12-377 points.
inline int choose_window(size_t n, int bits) {
  int best = 8;
  double best_cost = 1e300;
  for (int c = 8; c <= 20; c++) {
    const double W = (double)((bits + 1 + c - 1) / c);
    const double cost = (double)n * W + 3.0 * W * (double)(1u << (c - 1));
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}

// Bits the digits of one half of a GLV split cover: every curve's split leaves
// |k1|, |k2| < 2^GLV_HALF_BITS (msm_impl.hpp, Glv<C>; GlvBls381 asserts it).
constexpr int GLV_HALF_BITS = 127;

// What msm_plan derives from (scalars, scalar bits, layout, window override)
// before it allocates or launches anything.
struct MsmPlanGeom {
  size_t n = 0;   // (virtual) points: 2 n0 for a GLV split
  int bits = 0;   // scalar bits the digits cover (fr_bits; 127 for a GLV split)
  uint32_t c = 0, W = 0, nb = 0, Wred = 0, total = 0;
  uint32_t wn = 0;  // first narrow window (W when all are c bits)
  size_t npts = 0, M = 0;
  SortGeom sg;
};
// n0 scalars of an fr_bits-bit field; glv: the split layout; pre: a precomputed
// (shared-bucket) set or null; c_override: gm_set_msm_window's value (0: the cost
// model).  Returns null, or the text of the refusal (GM_ERR_INVALID).
inline const char* msm_plan_geom(size_t n0, int fr_bits, bool glv, const MsmPrecomp* pre, int c_override,
                                 MsmPlanGeom& g) {
  g = MsmPlanGeom();
  size_t n = n0;
  g.bits = fr_bits;
  if (glv) {  // virtual points: P_i and phi(P_i)
    n = 2 * n0;
    g.bits = GLV_HALF_BITS;
  }
  g.n = n;
  if (n >= (size_t(1) << 31)) return "msm: n must be < 2^31";
  const bool shared = pre && pre->c;
  if (shared && (pre->stride < n || (size_t)pre->W * pre->stride >= (size_t(1) << 31) || pre->narrow >= pre->W ||
                 (size_t)pre->c * pre->W - pre->narrow < (size_t)fr_bits + 1))
    return "msm: precomputed point set does not cover this MSM";
  const uint32_t c = shared ? pre->c : (c_override ? (uint32_t)c_override : (uint32_t)choose_window(n, g.bits));
  // ceil((bits+1)/c): the top signed digit never carries
  const uint32_t W = shared ? pre->W : (uint32_t)(g.bits + 1 + c - 1) / c;
  g.c = c;
  g.W = W;
  g.nb = 1u << (c - 1);
  g.Wred = shared ? 1 : W;
  g.total = g.Wred * g.nb;
  g.npts = shared ? (size_t)W * pre->stride : n;
  const size_t M = (size_t)W * n;  // upper bound on the entries: zero digits are dropped
  g.M = M;
  if (M >= (size_t(1) << 31)) return "msm: n * windows must be < 2^31";
  // Sort geometry: ~2K entries per coarse bin for uniform digits (the final pass
  // sorts a bin of up to S2_STAGE entries in LDS; the narrow top window's bins
  // are ~2x fuller).  Pass-1 bins (b >> (F + G)) are coarsened by G until one
  // pass-1 block (one window of S1 points in the plain layout) touches at most
  // 512 of them (long write runs) and there are at most 8192; G > 0 adds the
  // middle pass (msm_sort.hip).
  SortGeom& sg = g.sg;
  sg.T = g.total;
  sg.M = M;
  sg.F = 4;
  // A GLV plan's windows are full width (|k1|, |k2| < 0.87 * 2^127: no narrow top
  // window) with twice the entries per bucket: ~4K-entry bins keep one pass-1
  // block within 512 bins (no middle pass) and still fit S2_STAGE.
  // The shared-bucket (precomputed) layout takes ~1.5K-entry bins: its 2^24 sort 3.78 -> 3.34 ms, 2^20 0.28 ->
  // 0.19 ms against ~0.75K, while ~3K are slower again (profiles/r06v_shared_sort_bins_ab.txt); the plain
  // layout's 2^24 sort is slower with ~2K bins than ~1K (3.29 -> 3.51 ms, r06u_sort_bins_ab.txt) and with ~0.5K
  // (3.35 -> 3.83 ms, r06w_plain_sort_bins_ab.txt).
  const double bin_entries = glv || shared ? 4096.0 : 2048.0;
  while (sg.F < 13 && (double)M * std::ldexp(1.0, (int)sg.F + 1) <= bin_entries * sg.T) sg.F++;
  auto bins = [&](uint32_t sh) { return (uint32_t)(((uint64_t)sg.T + (1ull << sh) - 1) >> sh); };
  auto touched = [&](uint32_t sh) { return shared ? bins(sh) : std::max(1u, g.nb >> sh); };
  // GM_MSM_SORT_MING: minimum G (tests exercise the middle pass at small sizes)
  const char* ming = getenv("GM_MSM_SORT_MING");
  sg.G = ming ? (uint32_t)std::min(10, std::max(0, atoi(ming))) : 0u;
  // (shared layout at 2^20: 8192 pass-1 bins with G = 0 measured 0.285 ms vs
  // 0.315 with the middle pass -- its 109 MB of entries stay in the caches, which
  // merge the short write runs; at 2^24, 1.6 GB, they do not: 2.4 ms per sort)
  const uint32_t max_touched = (shared && M < (size_t(1) << 24)) ? 8192u : 512u;
  while (sg.G < 10 && (touched(sg.F + sg.G) > max_touched || bins(sg.F + sg.G) > 8192)) sg.G++;
  while (sg.G && sg.F + sg.G > 31) sg.G--;
  sg.NC = bins(sg.F);
  sg.NS = bins(sg.F + sg.G);
  if (sg.NS > 8192) return "msm: too many buckets for the sort";
  // 4-byte entries between the sort passes when the key bits below the pass-1
  // bin, the sign and the largest point index fit (SortGeom);
  // GM_MSM_SORT_WIDE=1 keeps 8 bytes (tests, A/B runs)
  const char* wide = getenv("GM_MSM_SORT_WIDE");
  sg.compact = !(wide && atoi(wide) > 0) && sort_compact_fits(sg.F, sg.G, g.npts);
  g.wn = shared ? W - pre->narrow : W;
  if (!shared && !glv) {
    // plain layout: balance the windows (see DigitGeom, msm_impl.hpp)
    const uint32_t narrow = c * W - (uint32_t)(g.bits + 1);
    if (narrow < W) g.wn = W - narrow;
  }
  return nullptr;
}

// Level-1 segment length (buckets) of the bucket reduction and the segments per
// window.  Measured at 2^20 (BN254 G1 / G2 / BLS12-377 G2 reduction ms): L = 1:
// 0.83 / 4.2 / 16.9, L = 2: 0.51 / 2.6 / 9.6, L = 4: 0.36 / 1.74 / 6.05 -- the LDS
// bit-sum trees cost more per add than the running sums.  So L grows (to 32) as
// long as k_msm_seg keeps >= 128K threads (two waves per SIMD): 4 for 2^20 plain,
// 16 for the one-window 2^21 buckets of a precomputed 2^24 key (segment lengths
// 4 / 8 re-measured in the pipelined loop, profiles/r05ai_segl_ab.txt).
inline void msm_seg_geom(uint32_t Wred, uint32_t nb, uint32_t& L, uint32_t& nseg) {
  uint32_t Lwant = 4;
  while (Lwant < 32 && (size_t)Wred * nb / (2 * Lwant) >= (size_t(1) << 17)) Lwant *= 2;
  L = nb >= Lwant ? Lwant : nb;
  nseg = nb / L;
}

// LDS tree levels of the bucket reduction over nseg segment nodes of xyzz_bytes
// per point (sizeof(XYZZ<DF>)): level i merges groups of 2^lg[i] nodes; Q is the
// points per node after the last level, [G, U, Y_0..Y_{Q-3}].  At most 512 tree
// tasks (adds) per level: two per thread of a BS_THREADS block.  (A 512-thread
// block with one task per thread measured no faster at 2^20: the tree's tail
// is short of blocks, not of threads.)
constexpr uint32_t BS_THREADS = 256;
struct MsmTreeGeom {
  static constexpr uint32_t MAX_LEVELS = 24;  // a level at least halves nseg <= 2^23
  uint32_t levels = 0, lg[MAX_LEVELS] = {}, Q = 2;
};
// false: a level does not fit LDS
inline bool msm_tree_geom(uint32_t nseg, size_t xyzz_bytes, MsmTreeGeom& g) {
  g = MsmTreeGeom();
  const size_t slot_budget = (96u << 10) / xyzz_bytes;
  uint32_t m = nseg, Q = 2;
  while (m > 1) {
    uint32_t lg = 0;
    // largest power-of-two group with NT*Q slots in budget and <= 2 tasks per thread
    while ((2u << lg) <= m && (size_t)(2u << lg) * Q <= slot_budget && (1u << lg) * (Q + 1) <= 2 * BS_THREADS) lg++;
    if (lg == 0 || g.levels == MsmTreeGeom::MAX_LEVELS) return false;
    g.lg[g.levels++] = lg;
    Q += lg;
    m >>= lg;
  }
  g.Q = Q;
  return true;
}

// Host wire-map sentinel "this wire has no point" (groth16.hip, the shared wire
// plan): k_expand_points writes an all-zero (infinity) point into the expanded
// array's slot for such a wire.  It is never an entry value of a plan -- the
// accumulation kernels have no skip branch, so an entry carrying it would fail
// the bounds check (err = 2).  Valid point indices stay below 2^31 - 1
// (msm_plan bounds n and W * stride by 2^31).
constexpr uint32_t MSM_SKIP = 0x7fffffffu;

// Sorted signed-digit plan of one scalar vector: depends only on the scalars
// and the point layout, so MSMs that share scalars and layout (Groth16's G1 and
// G2 B-MSMs, prove.go:217,293) sort once.  Buffers live in the caller's Arena.
struct MsmPlan {
  uint32_t c = 0, W = 0, nb = 0, total = 0;
  uint32_t Wred = 0;  // windows reduced separately: W (plain) or 1 (shared buckets)
  size_t n = 0, M = 0;  // M: upper bound on the sorted entries (n * W); offsets[total] = actual
  size_t npts = 0;    // points addressable through the plan (bounds check)
  int bits = 0;       // scalar bits the digits cover (FR_BITS; 127 for a GLV split)
  uint32_t wn = 0;    // first narrow window (window_geom; W when all are c bits)
  // sorted bucket keys (window-major bucket index), offsets[total] entries; null
  // for a plan built without them (only the lane-pair G2 kernels read keys)
  uint32_t* keys = nullptr;
  uint32_t* vals = nullptr;     // point index | sign << 31
  uint32_t* offsets = nullptr;  // total + 1 bucket start offsets
  // Piece plan (G1 accumulation, msm_piece_plan): every non-empty bucket of len
  // entries is cut into ceil(len / T) pieces of nearly equal length, and the
  // pieces are counting-sorted by length, longest first, so that the lanes of a
  // wave run the same number of adds.  A piece is {first entry, length,
  // destination, 0}: the destination is the bucket itself when the bucket is one
  // piece, else PIECE_PART | part slot; a cut bucket b owns the contiguous part
  // slots pbase[b] .. pbase[b] + ceil(len / T).
  uint32_t T = 0;                   // piece length cap (0: no piece plan, G2-only plans)
  size_t max_pieces = 0, max_parts = 0;  // bounds for allocation and launch
  uint4* pieces = nullptr;          // pcount[0] descriptors
  uint32_t* pcount = nullptr;       // [0] pieces, [1] part slots
  uint32_t* pbase = nullptr;        // per bucket: first part slot (cut buckets only)
  uint32_t* partb = nullptr;        // per part slot: its bucket
};
constexpr uint32_t PIECE_PART = 0x80000000u;
constexpr uint32_t PIECE_MAX_LEN = 128;  // length classes of the counting sort
// Piece length for a plan of M entries at most (gm_set_msm_piece_len overrides it)
uint32_t msm_piece_len(const gm_ctx* ctx, size_t M);
// Builds the piece plan of `plan` (offsets must be queued on ctx->stream).
int msm_piece_plan(gm_ctx* ctx, Arena& arena, MsmPlan& plan, uint32_t T);
// glv (plain layout, all three curves): each scalar k is split
// k = k1 + k2 lambda with |k1|, |k2| < 2^127, over 2n points
// [P_0..P_{n-1}, phi(P_0)..phi(P_{n-1})] (msm_device_launch builds them): half
// the windows, so half the buckets to reduce, for the same number of bucket adds.
// pieces: build the G1 piece plan; keys: write the sorted keys (needed by
// msm_launch<C, true>; a plan that only G1 MSMs use can drop them).
template <class C>
int msm_plan(gm_ctx* ctx, Arena& arena, const void* scalars_dev, size_t n, const MsmPrecomp* pre,
             MsmPlan& plan, bool glv = false, bool pieces = true, bool keys = true);
// GLV for an MSM of n points on ctx: the context's setting (gm_set_msm_glv)
// or, by default, on for n up to 2^21 (G1 and G2)
bool msm_glv_on(const gm_ctx* ctx, bool g2, size_t n);
template <class C, bool G2>
int msm_run(gm_ctx* ctx, const MsmPlan& plan, const void* points_internal,
            typename GroupSel<C, G2>::HF (&jac_out)[3]);

// An MSM whose device work is queued and whose host tail (consistency and
// long-span checks, host Horner) is deferred to msm_finish, so that the tail of
// one MSM overlaps the device work of the next.  Its buffers live in the Arena
// given to msm_launch, which must outlive msm_finish.
struct MsmTail {
  size_t n = 0, M = 0;
  uint32_t c = 0, W = 0, Wr = 0, nb = 0, total = 0, L = 0, nseg = 0, K = 0, Q = 2;
  uint32_t wn = 0;  // first narrow (c - 1 bit) window of the plan (window_geom)
  const uint32_t* keys = nullptr;
  const uint32_t* offsets = nullptr;
  // G1: the plan's piece length and part tables; `pfirst` holds the part slots
  uint32_t T = 0;
  size_t max_parts = 0;
  const uint32_t *pcount = nullptr, *pbase = nullptr, *partb = nullptr;
  void *buckets = nullptr, *pfirst = nullptr, *plast = nullptr, *nodes_a = nullptr, *nodes_b = nullptr;
  void *wsum = nullptr, *errw = nullptr;
  uint8_t* stage = nullptr;  // pinned readback: 16 B (error, max span) + the exported nodes
  gm_ctx* stage_ctx = nullptr;  // owner of `stage` (tail_pinned_acquire), released by msm_finish
  int stage_idx = -1;
  hipEvent_t done = nullptr;
  void release_stage();  // runtime.hpp: returns `stage` to the context
  MsmTail() = default;
  MsmTail(const MsmTail&) = delete;
  MsmTail& operator=(const MsmTail&) = delete;
  ~MsmTail() {
    if (done) hipEventDestroy(done);
    release_stage();
  }
};
template <class C, bool G2>
int msm_launch(gm_ctx* ctx, Arena& arena, const MsmPlan& plan, const void* points_internal, MsmTail& t);
template <class C, bool G2>
int msm_finish(gm_ctx* ctx, MsmTail& t, typename GroupSel<C, G2>::HF (&jac_out)[3]);
// plan + launch (points converted into `arena` first unless points_internal)
template <class C, bool G2>
// inputs_read (optional) is recorded on ctx->stream once the caller's scalars
// and points have been read for the last time (after the digits / conversion).
int msm_device_launch(gm_ctx* ctx, Arena& arena, const void* scalars_dev, const void* points_dev, size_t n,
                      bool points_internal, const MsmPrecomp* pre, MsmTail& t,
                      hipEvent_t inputs_read = nullptr);

// out = sum_i int(scalars[i]) * points[i] as a host Jacobian triple (X, Y, Z).
// points_dev is gnark-layout affine points, or (points_internal) an array of
// device-internal points prepared by msm_prepare_points /
// msm_precompute_points (e.g. a device-resident proving key); `pre` describes a
// precomputed set.
template <class C, bool G2>
int msm_device(gm_ctx* ctx, const void* scalars_dev, const void* points_dev, size_t n,
               typename GroupSel<C, G2>::HF (&jac_out)[3], bool points_internal = false,
               const MsmPrecomp* pre = nullptr);
// Converts n gnark-layout affine points into the internal layout (dst holds
// n * msm_internal_point_bytes<C, G2>() bytes).
template <class C, bool G2>
int msm_prepare_points(gm_ctx* ctx, const void* gnark_points, size_t n, void* dst);
// Same, plus the W - 1 shifted copies of `pre` (dst holds
// pre.W * pre.stride * msm_internal_point_bytes<C, G2>() bytes, stride >= n).
template <class C, bool G2>
int msm_precompute_points(gm_ctx* ctx, const void* gnark_points, size_t n, const MsmPrecomp& pre, void* dst);
template <class C, bool G2>
size_t msm_internal_point_bytes();
// gm_msm_async (include/gnark_mi355x.h) with the choice of the point layout:
// prepared = a prepared set (gm_points_upload), not gnark-layout points.  Finished by gm_msm_wait.
int msm_async_queue(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* points_dev, size_t n,
                    bool prepared, gm_msm_pending** out);
}  // namespace gm
