// gnark's trace.S from the wire tables resident on the device.  buildPermutation
// (backend/plonk/bls12-377/setup.go:271-325) walks lro = xa | xb | xc, position ->
// wire id, and links every position to the previous position of the same wire,
// the first one of a wire to the last one.  lro is gm_plonk_wires::tab as it
// lies (3n u32, every id < nb_wires), so with N = 3n:
//
//  1. Sort the positions 0 .. N-1 by wire id, stably: positions ascend inside a
//     wire's run.  Least-significant-digit radix sort, 8-bit digits, as many
//     passes as nb_wires - 1 has bytes (none for nb_wires = 1).  A pass is
//       k_wp_hist     per tile of 2048 entries, the count of every digit;
//       the scan      exclusive, device-wide (scan.hpp), over (digit, tile);
//       k_wp_scatter  every entry to scan[digit][tile] + its rank among the
//                     tile's entries of that digit.
//     The rank is what makes the sort stable.  A tile is dealt out so that (wave,
//     round, lane) order is position order: wave w takes the tile's entries
//     [512 w, 512 (w + 1)), 64 per round.  Inside a round the lanes holding the
//     same digit are found with eight ballots (one per digit bit); an entry's
//     rank in the round is the number of such lanes below it, and the lowest of
//     them adds the group's size to the wave's counter of that digit in LDS and
//     hands the old value to the group.  A round whose 64 entries share one
//     digit (the padding rows all hold wire 0) is therefore one LDS atomic, not
//     64 on one address.  The four waves' counters are then prefixed per digit,
//     the digits' totals scanned, and the tile written out through LDS in sorted
//     order, so that a digit's entries leave as one contiguous run.
//     The first pass reads its keys from tab in place (the position is the index).
//     Later passes carry the key beside the position: re-gathering it from tab
//     through the position halves the workspace and doubles the time (DESIGN.md
//     §3.7 has the measurement).
//
//  2. Link.  In the sorted order, entry i is a head if its key differs from entry
//     i - 1's, a tail if it differs from entry i + 1's.  An interior entry's
//     position maps to its left neighbour's position.  A head's position maps to
//     its run's tail: the tail does that write, having found its head as the
//     largest head index <= i, by a max-scan inside the tile (k_wp_link).  The one
//     tail per tile whose head lies in an earlier tile is set aside; a max-scan
//     over the tiles' last heads (one block) then tells it where its head is
//     (k_wp_link_fix).  No scratch is indexed by wire id: nb_wires may be 2^32 - 1.
//
// Every counter is written before it is read, so stale workspace does no harm.
#include <string>

#include "plonk_wires_perm.hpp"
#include "scan.hpp"
#include "sort_util.hpp"

namespace gm {

namespace {

constexpr unsigned WP_TPB = 256, WP_WAVES = WP_TPB / 64;
constexpr unsigned WP_ROUNDS = 8;
constexpr unsigned WP_TILE = WP_TPB * WP_ROUNDS;       // 2048 entries
constexpr unsigned WP_WAVE_SPAN = 64 * WP_ROUNDS;      // consecutive entries of one wave
constexpr unsigned WP_DIGITS = 256;
static_assert(WP_DIGITS == WP_TPB, "thread d owns digit d");
constexpr unsigned WP_LINK_TPB = 1024;                 // the link's tile: one entry per thread

// the valid lanes of the wave that hold the same 8-bit digit as this lane
__device__ __forceinline__ uint64_t wp_match(uint32_t d, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (d >> b) & 1;
    const uint64_t bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// the key of sorted entry i as a pass reads it
template <bool FIRST>
__device__ __forceinline__ void wp_load(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ pos_in,
                                        const uint32_t* __restrict__ key_in, uint32_t i, uint32_t& pos,
                                        uint32_t& key) {
  if constexpr (FIRST) {
    pos = i;
    key = tab[i];
  } else {
    pos = pos_in[i];
    key = key_in[i];
  }
}

// hist[d * tiles + tile] = entries of the tile whose digit is d
template <bool FIRST>
__global__ void __launch_bounds__(WP_TPB)
    k_wp_hist(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ pos_in,
              const uint32_t* __restrict__ key_in, uint32_t N, uint32_t shift, uint32_t tiles,
              uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[WP_DIGITS];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, tile = blockIdx.x;
  h[tid] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)tile * WP_TILE + wave * WP_WAVE_SPAN + lane;
#pragma unroll
  for (unsigned r = 0; r < WP_ROUNDS; r++) {
    const uint64_t i = base + r * 64;
    const bool valid = i < N;
    uint32_t pos = 0, key = 0;
    if (valid) wp_load<FIRST>(tab, pos_in, key_in, (uint32_t)i, pos, key);
    const uint32_t d = (key >> shift) & 255u;
    const uint64_t m = wp_match(d, valid);
    if (valid && (m & __lanemask_lt()) == 0) atomicAdd(&h[d], (uint32_t)__popcll(m));
  }
  __syncthreads();
  hist[(size_t)tid * tiles + tile] = h[tid];
}

// ofs: the exclusive scan of hist over (digit, tile)
template <bool FIRST>
__global__ void __launch_bounds__(WP_TPB)
    k_wp_scatter(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ pos_in,
                 const uint32_t* __restrict__ key_in, uint32_t N, uint32_t shift, uint32_t tiles,
                 const uint32_t* __restrict__ ofs, uint32_t* __restrict__ pos_out, uint32_t* __restrict__ key_out) {
  __shared__ uint32_t cnt[WP_WAVES][WP_DIGITS];  // a wave's entries per digit, then the waves before it
  __shared__ uint32_t dbase[WP_DIGITS];          // the tile's entries of smaller digits
  __shared__ uint32_t gdst[WP_DIGITS];           // ofs[d][tile] - dbase[d]
  __shared__ uint32_t wsum[WP_WAVES];
  __shared__ uint32_t spos[WP_TILE];
  __shared__ uint32_t skey[WP_TILE];
  __shared__ uint8_t sdig[WP_TILE];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, tile = blockIdx.x;
#pragma unroll
  for (unsigned w = 0; w < WP_WAVES; w++) cnt[w][tid] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)tile * WP_TILE + wave * WP_WAVE_SPAN + lane;
  uint32_t pos[WP_ROUNDS], key[WP_ROUNDS], rnk[WP_ROUNDS];
#pragma unroll
  for (unsigned r = 0; r < WP_ROUNDS; r++) {
    const uint64_t i = base + r * 64;
    const bool valid = i < N;
    pos[r] = 0;
    key[r] = 0;
    if (valid) wp_load<FIRST>(tab, pos_in, key_in, (uint32_t)i, pos[r], key[r]);
    const uint32_t d = (key[r] >> shift) & 255u;
    const uint64_t m = wp_match(d, valid);
    const uint32_t below = (uint32_t)__popcll(m & __lanemask_lt());
    uint32_t old = 0;
    if (valid && below == 0) old = atomicAdd(&cnt[wave][d], (uint32_t)__popcll(m));
    // the group's lowest lane did the add; an invalid lane reads its own
    const int leader = valid ? __ffsll((unsigned long long)m) - 1 : (int)lane;
    old = __shfl(old, leader, 64);
    rnk[r] = old + below;
  }
  __syncthreads();
  // thread d: the waves' counts of digit d become what the waves before hold
  uint32_t total = 0;
#pragma unroll
  for (unsigned w = 0; w < WP_WAVES; w++) {
    const uint32_t c = cnt[w][tid];
    cnt[w][tid] = total;
    total += c;
  }
  const uint32_t inc = wave_incl_scan(total);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (unsigned w = 0; w < WP_WAVES; w++)
    if (w < wave) before += wsum[w];
  const uint32_t db = before + inc - total;
  dbase[tid] = db;
  gdst[tid] = ofs[(size_t)tid * tiles + tile] - db;
  __syncthreads();
#pragma unroll
  for (unsigned r = 0; r < WP_ROUNDS; r++) {
    const uint64_t i = base + r * 64;
    if (i < N) {
      const uint32_t d = (key[r] >> shift) & 255u;
      const uint32_t lr = dbase[d] + cnt[wave][d] + rnk[r];  // < the tile's entry count
      spos[lr] = pos[r];
      sdig[lr] = (uint8_t)d;
      skey[lr] = key[r];
    }
  }
  __syncthreads();
  const uint64_t first = (uint64_t)tile * WP_TILE;
  const uint32_t count = (uint32_t)min((uint64_t)WP_TILE, (uint64_t)N - first);
  for (uint32_t j = tid; j < count; j += WP_TPB) {
    const uint32_t dst = gdst[sdig[j]] + j;  // < N: the scan's offset plus the rank in the digit
    pos_out[dst] = spos[j];
    key_out[dst] = skey[j];
  }
}

// the sorted order of a single wire: the identity
__global__ void __launch_bounds__(256) k_wp_iota(uint32_t* __restrict__ pos, uint32_t N) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) pos[i] = (uint32_t)i;
}

template <class OUT>
__global__ void __launch_bounds__(256) k_wp_widen(const uint32_t* __restrict__ in, uint32_t N, OUT* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) out[i] = (OUT)in[i];
}

// Sorted entry i = blockIdx.x * 1024 + threadIdx.x.  last_head[tile]: 1 + the
// largest head index of the tile, 0 without one.  deferred[tile]: 1 + the index
// of the tail whose head lies in an earlier tile, 0 without one.
template <class OUT>
__global__ void __launch_bounds__(WP_LINK_TPB)
    k_wp_link(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ keys, uint32_t N, OUT* __restrict__ out,
              uint32_t* __restrict__ last_head, uint32_t* __restrict__ deferred) {
  __shared__ uint32_t sp[WP_LINK_TPB + 1], sk[WP_LINK_TPB + 2], ws[17];
  __shared__ uint32_t sdef;
  const uint32_t t = threadIdx.x;
  const uint64_t first = (uint64_t)blockIdx.x * WP_LINK_TPB;
  const uint64_t i = first + t;
  const bool valid = i < N;
  if (t == 0) sdef = 0;
  // sp[t + 1], sk[t + 1]: entry i; sp[0], sk[0]: entry first - 1; sk[t + 2] of the
  // tile's last entry: entry i + 1
  uint32_t p = 0, k = 0;
  if (valid) {
    p = pos[i];
    k = keys[i];
    sp[t + 1] = p;
    sk[t + 1] = k;
    if (t == 0 && i > 0) {
      sp[0] = pos[i - 1];
      sk[0] = keys[i - 1];
    }
    if ((t == WP_LINK_TPB - 1 || i + 1 == N) && i + 1 < N) sk[t + 2] = keys[i + 1];
  }
  __syncthreads();
  const bool head = valid && (i == 0 || sk[t] != k);
  const bool tail = valid && (i + 1 == N || sk[t + 2] != k);
  uint32_t total;
  const uint32_t v = head ? (uint32_t)i + 1 : 0u;
  const uint32_t hd = max(block_excl<true>(v, ws, &total), v);  // 1 + my run's head, 0: before the tile
  if (valid && !head) out[p] = (OUT)sp[t];
  if (tail) {
    if (hd)
      out[sp[hd - (uint32_t)first]] = (OUT)p;  // sp[(hd - 1 - first) + 1]
    else
      sdef = (uint32_t)i + 1;  // at most one per tile: the first tail
  }
  __syncthreads();
  if (t == 0) {
    last_head[blockIdx.x] = total;
    deferred[blockIdx.x] = sdef;
  }
}

// carry: the exclusive max-scan of last_head over the tiles
template <class OUT>
__global__ void __launch_bounds__(256)
    k_wp_link_fix(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ carry,
                  const uint32_t* __restrict__ deferred, uint32_t tiles, OUT* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < tiles; b += stride) {
    const uint32_t d = deferred[b], h = carry[b];
    // entry 0 is a head, so every tile after the first has one before it
    if (d && h) out[pos[h - 1]] = (OUT)pos[d - 1];
  }
}

int refuse(const std::string& msg) {
  set_error("plonk wires permutation: " + msg);
  return GM_ERR_INVALID;
}

const char* const HIST_NAMES[4] = {"wires_perm_hist_0", "wires_perm_hist_1", "wires_perm_hist_2",
                                   "wires_perm_hist_3"};
const char* const SCAN_NAMES[4] = {"wires_perm_scan_0", "wires_perm_scan_1", "wires_perm_scan_2",
                                   "wires_perm_scan_3"};
const char* const SCATTER_NAMES[4] = {"wires_perm_scatter_0", "wires_perm_scatter_1", "wires_perm_scatter_2",
                                      "wires_perm_scatter_3"};

int sort_pass(gm_ctx* ctx, int pass, const uint32_t* tab, const uint32_t* pos_in, const uint32_t* key_in, uint32_t N,
              uint32_t tiles, uint32_t* hist, uint32_t* bsum, uint32_t* pos_out, uint32_t* key_out) {
  const uint32_t shift = 8u * (uint32_t)pass;
  const size_t cells = (size_t)WP_DIGITS * tiles;
  int rc;
  {
    ProfScope ps(ctx, HIST_NAMES[pass]);
    auto k = pass == 0 ? k_wp_hist<true> : k_wp_hist<false>;
    hipLaunchKernelGGL(k, dim3(tiles), dim3(WP_TPB), 0, ctx->stream, tab, pos_in, key_in, N, shift, tiles, hist);
  }
  {
    ProfScope ps(ctx, SCAN_NAMES[pass]);
    if ((rc = device_excl_scan(ctx, hist, cells, hist, bsum))) return rc;  // hist[cells]: the total, unused
  }
  {
    ProfScope ps(ctx, SCATTER_NAMES[pass]);
    auto k = pass == 0 ? k_wp_scatter<true> : k_wp_scatter<false>;
    hipLaunchKernelGGL(k, dim3(tiles), dim3(WP_TPB), 0, ctx->stream, tab, pos_in, key_in, N, shift, tiles,
                       (const uint32_t*)hist, pos_out, key_out);
  }
  GM_HIP(hipGetLastError());
  return GM_OK;
}

template <class OUT>
int link(gm_ctx* ctx, const uint32_t* pos, const uint32_t* keys, uint32_t N, OUT* out, uint32_t* last_head,
         uint32_t* deferred) {
  const uint32_t ltiles = (N + WP_LINK_TPB - 1) / WP_LINK_TPB;
  ProfScope ps(ctx, "wires_perm_link");
  hipLaunchKernelGGL(k_wp_link<OUT>, dim3(ltiles), dim3(WP_LINK_TPB), 0, ctx->stream, pos, keys, N, out,
                     last_head, deferred);
  int rc;
  if ((rc = block_scan_inplace(ctx, last_head, ltiles, true))) return rc;
  hipLaunchKernelGGL(k_wp_link_fix<OUT>, dim3(grid_for(ltiles)), dim3(256), 0, ctx->stream, pos,
                     (const uint32_t*)last_head, (const uint32_t*)deferred, ltiles, out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // namespace

int plonk_wires_perm_queue(gm_ctx* ctx, Arena& arena, const gm_plonk_wires* w, int64_t* out64,
                           const uint32_t** out32) {
  if (w->n > WIRES_PERM_MAX_N) return refuse("n must be at most 2^30 (positions are 32-bit)");
  // bytes of nb_wires - 1: the ids lie in [0, nb_wires)
  int passes = 0;
  for (uint64_t top = w->nb_wires - 1; top; top >>= 8) passes++;
  const uint32_t N = (uint32_t)(3 * w->n);
  const uint32_t tiles = (N + WP_TILE - 1) / WP_TILE;
  const uint32_t ltiles = (N + WP_LINK_TPB - 1) / WP_LINK_TPB;
  const size_t cells = (size_t)WP_DIGITS * tiles;
  int rc;
  DevBuf pos[2], key[2], hist, bsum, lh, df;
  for (int k = 0; k < 2; k++) {
    if ((rc = pos[k].alloc(arena, sizeof(uint32_t) * N))) return rc;
    if ((rc = key[k].alloc(arena, sizeof(uint32_t) * N))) return rc;
  }
  if ((rc = hist.alloc(arena, sizeof(uint32_t) * (cells + 1)))) return rc;
  if ((rc = bsum.alloc(arena, sizeof(uint32_t) * scan_ws_words(cells)))) return rc;
  if ((rc = lh.alloc(arena, sizeof(uint32_t) * ltiles))) return rc;
  if ((rc = df.alloc(arena, sizeof(uint32_t) * ltiles))) return rc;
  int cur = 0;  // pos[cur] holds the sorted order
  if (passes == 0) {
    hipLaunchKernelGGL(k_wp_iota, dim3(grid_for(N)), dim3(256), 0, ctx->stream, pos[0].as<uint32_t>(), N);
    GM_HIP(hipMemsetAsync(key[0].p, 0, sizeof(uint32_t) * N, ctx->stream));  // the one wire is 0
    GM_HIP(hipGetLastError());
  }
  for (int p = 0; p < passes; p++) {
    // the first pass reads the tables in place and has no input buffers
    const int dst = p == 0 ? 0 : cur ^ 1;
    const uint32_t* const pin = p == 0 ? nullptr : pos[cur].as<uint32_t>();
    const uint32_t* const kin = p == 0 ? nullptr : key[cur].as<uint32_t>();
    if ((rc = sort_pass(ctx, p, w->tab, pin, kin, N, tiles, hist.as<uint32_t>(), bsum.as<uint32_t>(),
                        pos[dst].as<uint32_t>(), key[dst].as<uint32_t>())))
      return rc;
    cur = dst;
  }
  const uint32_t* const sorted = pos[cur].as<uint32_t>();
  const uint32_t* const skeys = key[cur].as<uint32_t>();
  if (out32) {
    uint32_t* const o = pos[cur ^ 1].as<uint32_t>();
    if ((rc = link<uint32_t>(ctx, sorted, skeys, N, o, lh.as<uint32_t>(), df.as<uint32_t>()))) return rc;
    *out32 = o;
    if (out64) {
      hipLaunchKernelGGL(k_wp_widen<int64_t>, dim3(grid_for(N)), dim3(256), 0, ctx->stream, (const uint32_t*)o, N,
                         out64);
      GM_HIP(hipGetLastError());
    }
    return GM_OK;
  }
  return link<int64_t>(ctx, sorted, skeys, N, out64, lh.as<uint32_t>(), df.as<uint32_t>());
}

int plonk_wires_permutation(gm_ctx* ctx, const gm_plonk_wires* w, int64_t* perm_dev) {
  if (w->ctx != ctx) return refuse("the tables were uploaded on another context");
  if (w->n > WIRES_PERM_MAX_N) return refuse("n must be at most 2^30 (positions are 32-bit)");
  if ((uintptr_t)perm_dev % sizeof(int64_t)) return refuse("perm_dev must be 8-byte aligned");
  const uintptr_t a = (uintptr_t)perm_dev, b = (uintptr_t)w->tab;
  if (a < b + 3 * w->n * sizeof(uint32_t) && b < a + 3 * w->n * sizeof(int64_t))
    return refuse("perm_dev overlaps the tables");
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  int rc;
  {
    ProfScope ps(ctx, "plonk_wires_permutation");
    rc = plonk_wires_perm_queue(ctx, arena, w, perm_dev, nullptr);
  }
  // nothing queued may outlive the workspace, also after a failure
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  prof_collect(ctx);
  if (rc) return rc;
  if (e != hipSuccess) {
    set_error(std::string("plonk wires permutation: ") + hipGetErrorString(e));
    return GM_ERR_DEVICE;
  }
  return GM_OK;
}

}  // namespace gm
