// Bucket sort of the MSM digits.  The digits themselves (and the coarse
// histogram) come from k_msm_digits in msm_impl.hpp, which decodes scalars.
//
// The sort only has to GROUP entries by bucket: the accumulation adds every
// point of a bucket exactly, so the order inside a bucket does not matter and no
// pass needs to be stable.  That makes each level a plain counting sort with
// LDS-atomic cursors:
//   k_msm_s1_scan     one block: exclusive scan of the NC coarse counts, and the
//                     part table -- a coarse bin above S2_BIG entries (skewed
//                     scalars, e.g. boolean witness wires) is split into parts.
//   k_msm_s1_scatter  digits -> coarse bins (entries: SortEnt below).
//   k_msm_s2_local    one block per part.  A single-part bin is finished here:
//                     LDS histogram of its 2^F buckets, LDS scan, offsets[];
//                     a bin of <= S2_STAGE entries (the usual case: ~4K) is held
//                     in registers, sorted into LDS and copied out coalesced,
//                     a larger one is read twice and scattered.  A part of a
//                     split bin only adds its LDS histogram into fcount
//                     (global atomics, <= 2^F each).
//   k_msm_s2_scan     split bins: scan of fcount -> offsets and cursors.
//   k_msm_s2_scatter  split bins: per part, one global range reservation per
//                     bucket, then the scatter.
// An entry between the passes sits in its pass-1 bin, so its position already
// gives the key bits above kb = F + G; the final pass rebuilds a bucket from its
// coarse bin and the low F bits.  When kb + vb <= 32 (vb = value bits: sign +
// point index, SortGeom::compact) an entry is one 32-bit word, else 8 bytes.
// The sorted keys are written only for plans a lane-pair (G2) kernel reads.
// Traffic per entry: 4 or 8 B written in pass 1; the same read here, 4 B of
// values (+ 4 B of keys) written (staged bins).
#include "msm.hpp"
#include "runtime.hpp"
#include "scan.hpp"
#include "sort_util.hpp"

namespace gm {

// Entry between the passes, by its word type.  kb = F + G key bits survive in
// the compact form; `low` holds at least those; `val` is index | sign << 31.
template <class E>
struct SortEnt;
template <>
struct SortEnt<uint64_t> {  // bucket | value << 32
  __device__ __forceinline__ static uint64_t make(uint32_t b, uint32_t v, uint32_t) { return ((uint64_t)v << 32) | b; }
  __device__ __forceinline__ static uint32_t low(uint64_t e) { return (uint32_t)e; }
  __device__ __forceinline__ static uint32_t val(uint64_t e, uint32_t) { return (uint32_t)(e >> 32); }
};
template <>
struct SortEnt<uint32_t> {  // bucket's low kb bits | index << kb | sign << 31 (index < 2^(31 - kb))
  __device__ __forceinline__ static uint32_t make(uint32_t b, uint32_t v, uint32_t kb) {
    return (b & ((1u << kb) - 1)) | ((v & 0x7fffffffu) << kb) | (v & 0x80000000u);
  }
  __device__ __forceinline__ static uint32_t low(uint32_t e) { return e; }
  __device__ __forceinline__ static uint32_t val(uint32_t e, uint32_t kb) {
    return ((e & 0x7fffffffu) >> kb) | (e & 0x80000000u);
  }
};

// LDS bytes one workgroup may allocate on `device` (queried once per device)
static size_t device_lds_per_block(int device) {
  static std::mutex mu;
  static std::map<int, size_t> cache;
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find(device);
  if (it != cache.end()) return it->second;
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) {
    (void)hipGetLastError();
    v = 64 << 10;
  }
  return cache[device] = (size_t)v;
}

static __global__ void __launch_bounds__(1024) k_msm_s1_scan(const uint32_t* __restrict__ ccount, uint32_t NC,
                                                             uint32_t T, uint32_t psz, uint32_t* __restrict__ cbase,
                                                             uint32_t* __restrict__ ccursor,
                                                             uint32_t* __restrict__ pbase,
                                                             uint32_t* __restrict__ offsets) {
  __shared__ uint32_t a[8192];
  __shared__ uint32_t wsum[17];
  const uint32_t t = threadIdx.x;
  for (uint32_t q = t; q < NC; q += S_THREADS) a[q] = ccount[q];
  const uint32_t total = block_excl_scan(a, NC, wsum);
  for (uint32_t q = t; q < NC; q += S_THREADS) {
    cbase[q] = a[q];
    ccursor[q] = a[q];
    const uint32_t cnt = ccount[q];
    a[q] = cnt > psz ? (cnt + psz - 1) / psz : 1u;
  }
  if (t == 0) {
    cbase[NC] = total;
    offsets[T] = total;
  }
  const uint32_t parts = block_excl_scan(a, NC, wsum);
  for (uint32_t q = t; q < NC; q += S_THREADS) pbase[q] = a[q];
  if (t == 0) pbase[NC] = parts;
}

// Pass-1 partition: block (chunk, w) moves the non-zero digits of window w of
// S1_PTS points into the coarse bins: LDS histogram with ranks, one global range
// reservation per touched bin, then the entries (SortEnt<E>; F here is the
// pass-1 shift, kb).  In the plain layout with 2^F <= nb the block touches only
// window w's bins [h0, h0 + nh), so its LDS is small and its write runs long
// (S1_PTS / nh entries per bin on average).
constexpr uint32_t S1_PPT = 8, S1_PTS = S_THREADS * S1_PPT;
template <class E>
static __global__ void __launch_bounds__(1024) k_msm_s1_scatter(const uint32_t* __restrict__ dig, uint32_t n,
                                                                uint32_t nb, uint32_t shared_stride, uint32_t F,
                                                                uint32_t NC, uint32_t nh,
                                                                uint32_t* __restrict__ ccursor,
                                                                E* __restrict__ tmp) {
  extern __shared__ uint32_t s1_lds[];
  uint32_t* hist = s1_lds;
  uint32_t* cur = s1_lds + nh;
  const uint32_t t = threadIdx.x, w = blockIdx.y, base = blockIdx.x * S1_PTS;
  const uint32_t wb = shared_stride ? 0u : w * nb;     // window's first bucket
  const uint32_t h0 = nh == NC ? 0u : wb >> F;          // first coarse bin in LDS
  for (uint32_t q = t; q < nh; q += S_THREADS) hist[q] = 0;
  __syncthreads();
  uint32_t dv[S1_PPT], rk[S1_PPT];
#pragma unroll
  for (uint32_t r = 0; r < S1_PPT; r++) {
    const uint32_t i = base + r * S_THREADS + t;
    dv[r] = i < n ? dig[(size_t)w * n + i] : 0xffffffffu;
    if (dv[r] != 0xffffffffu) rk[r] = lds_rank_add(hist, (((dv[r] & 0x7fffffffu) + wb) >> F) - h0);
  }
  __syncthreads();
  for (uint32_t q = t; q < nh; q += S_THREADS)
    if (hist[q]) cur[q] = atomicAdd(&ccursor[h0 + q], hist[q]);
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < S1_PPT; r++) {
    if (dv[r] == 0xffffffffu) continue;
    const uint32_t i = base + r * S_THREADS + t;
    const uint32_t b = (dv[r] & 0x7fffffffu) + wb;
    const uint32_t v = (shared_stride ? w * shared_stride + i : i) | (dv[r] & 0x80000000u);
    tmp[cur[(b >> F) - h0] + rk[r]] = SortEnt<E>::make(b, v, F);
  }
}

// The same partition with coalesced writes: the block's entries are first
// sorted by bin into an LDS stage (rank + the bin's local base), then written out
// in stage order, so consecutive lanes store consecutive entries of one
// bin's run instead of 64 scattered stores per wave instruction.  PPT points
// per thread (S_THREADS * PPT entries staged).  The stage always holds the
// 8-B form: the copy loop finds an entry's bin in its full key, and narrows the
// entry to E on the global store.  (A 4-B entry staged beside a 16-bit bin id,
// at 8 and at 16 points per thread, measured slower: profiles/sort_compact_ab.txt.)
template <class E, uint32_t PPT>
static __global__ void __launch_bounds__(1024) k_msm_s1_scatter_st(const uint32_t* __restrict__ dig, uint32_t n,
                                                                   uint32_t nb, uint32_t shared_stride, uint32_t F,
                                                                   uint32_t NC, uint32_t nh,
                                                                   uint32_t* __restrict__ ccursor,
                                                                   E* __restrict__ tmp) {
  constexpr uint32_t PTS = S_THREADS * PPT;
  extern __shared__ uint64_t s1s_lds[];
  uint64_t* stage = s1s_lds;
  uint32_t* hist = reinterpret_cast<uint32_t*>(s1s_lds + PTS);
  uint32_t* cur = hist + nh;   // global base of the block's run in bin q
  uint32_t* lb = cur + nh;     // local base of bin q in the stage
  uint32_t* wsum = lb + nh;    // 17 words
  const uint32_t t = threadIdx.x, w = blockIdx.y, base = blockIdx.x * PTS;
  const uint32_t wb = shared_stride ? 0u : w * nb;
  const uint32_t h0 = nh == NC ? 0u : wb >> F;
  for (uint32_t q = t; q < nh; q += S_THREADS) hist[q] = 0;
  __syncthreads();
  uint32_t dv[PPT], rk[PPT];
#pragma unroll
  for (uint32_t r = 0; r < PPT; r++) {
    const uint32_t i = base + r * S_THREADS + t;
    dv[r] = i < n ? dig[(size_t)w * n + i] : 0xffffffffu;
    if (dv[r] != 0xffffffffu) rk[r] = lds_rank_add(hist, (((dv[r] & 0x7fffffffu) + wb) >> F) - h0);
  }
  __syncthreads();
  for (uint32_t q = t; q < nh; q += S_THREADS) {
    const uint32_t h = hist[q];
    cur[q] = h ? atomicAdd(&ccursor[h0 + q], h) : 0u;
    lb[q] = h;
  }
  const uint32_t total = block_excl_scan(lb, nh, wsum);  // synchronises
#pragma unroll
  for (uint32_t r = 0; r < PPT; r++) {
    if (dv[r] == 0xffffffffu) continue;
    const uint32_t i = base + r * S_THREADS + t;
    const uint32_t b = (dv[r] & 0x7fffffffu) + wb;
    const uint32_t v = (shared_stride ? w * shared_stride + i : i) | (dv[r] & 0x80000000u);
    stage[lb[(b >> F) - h0] + rk[r]] = ((uint64_t)v << 32) | b;
  }
  __syncthreads();
  for (uint32_t q = t; q < total; q += S_THREADS) {
    const uint64_t e = stage[q];
    const uint32_t b = (uint32_t)e, h = (b >> F) - h0;
    tmp[cur[h] + (q - lb[h])] = SortEnt<E>::make(b, (uint32_t)(e >> 32), F);
  }
}

// block j -> (coarse bin, part): largest H with pbase[H] <= j
// (no split bins, the usual case: part j is bin j)
__device__ __forceinline__ void s2_locate(const uint32_t* __restrict__ pbase, uint32_t NC, uint32_t j, uint32_t* sh) {
  if (threadIdx.x == 0) {
    uint32_t lo = 0, hi = NC;  // pbase[lo] <= j < pbase[hi]
    if (pbase[NC] == NC) lo = j, hi = j + 1;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (pbase[mid] <= j) lo = mid;
      else hi = mid;
    }
    sh[0] = lo;
    sh[1] = j - pbase[lo];
  }
  __syncthreads();
}

// ---- middle pass of a three-level sort (large MSMs) ------------------------
// Pass 1 then partitions into super-bins s = b >> (F + G) (few enough that a
// pass-1 block writes long runs), and this pass splits every super-bin into its
// 2^G coarse bins H = b >> F, part by part (SM_PART entries): an LDS histogram
// per part and global atomics give the coarse counts, a per-super-bin scan the
// coarse bases (super-bin base + local prefix -- no device-wide scan), and the
// scatter reserves one range per touched coarse bin (SM_PART / 2^G entries per
// run on average).
constexpr uint32_t SM_PART = 16384, SM_IPT = SM_PART / S_THREADS;

template <class E>
static __global__ void __launch_bounds__(1024) k_msm_sm_count(const E* __restrict__ tmp,
                                                              const uint32_t* __restrict__ sbase,
                                                              const uint32_t* __restrict__ spbase, uint32_t NS,
                                                              uint32_t F, uint32_t G, uint32_t* __restrict__ ccount) {
  __shared__ uint32_t hist[1024], sh[2];
  const uint32_t j = blockIdx.x, t = threadIdx.x;
  if (j >= spbase[NS]) return;
  s2_locate(spbase, NS, j, sh);
  const uint32_t s = sh[0], p = sh[1];
  const uint32_t start = sbase[s], cnt = sbase[s + 1] - start;
  const uint32_t lo = p * SM_PART, hi = min(lo + SM_PART, cnt), ng = 1u << G;
  for (uint32_t q = t; q < ng; q += S_THREADS) hist[q] = 0;
  __syncthreads();
  for (uint32_t e = lo + t; e < hi; e += S_THREADS) lds_rank_add(hist, (SortEnt<E>::low(tmp[start + e]) >> F) & (ng - 1));
  __syncthreads();
  for (uint32_t q = t; q < ng; q += S_THREADS)
    if (hist[q]) atomicAdd(&ccount[(s << G) + q], hist[q]);
}

// block s: coarse bases / cursors of super-bin s's 2^G coarse bins, and the
// number of final-pass parts of each (cparts; > 1 only above S2_BIG entries)
static __global__ void __launch_bounds__(1024) k_msm_sm_scan(const uint32_t* __restrict__ ccount,
                                                             const uint32_t* __restrict__ sbase, uint32_t G,
                                                             uint32_t NC, uint32_t* __restrict__ cbase,
                                                             uint32_t* __restrict__ ccursor,
                                                             uint32_t* __restrict__ cparts) {
  __shared__ uint32_t a[1024], wsum[17];
  const uint32_t s = blockIdx.x, t = threadIdx.x, H0 = s << G;
  const uint32_t nh = min(1u << G, NC - H0);
  for (uint32_t q = t; q < nh; q += S_THREADS) a[q] = ccount[H0 + q];
  block_excl_scan(a, nh, wsum);
  for (uint32_t q = t; q < nh; q += S_THREADS) {
    const uint32_t c = ccount[H0 + q];
    cbase[H0 + q] = sbase[s] + a[q];
    ccursor[H0 + q] = sbase[s] + a[q];
    cparts[H0 + q] = c > S2_BIG ? (c + S2_BIG - 1) / S2_BIG : 1u;
  }
  if (t == 0 && H0 + nh == NC) cbase[NC] = sbase[s + 1];
}

template <class E>
static __global__ void __launch_bounds__(1024) k_msm_sm_scatter(const E* __restrict__ tmp,
                                                                const uint32_t* __restrict__ sbase,
                                                                const uint32_t* __restrict__ spbase, uint32_t NS,
                                                                uint32_t F, uint32_t G,
                                                                uint32_t* __restrict__ ccursor,
                                                                E* __restrict__ tmp2) {
  __shared__ uint32_t hist[1024], cur[1024], sh[2];
  const uint32_t j = blockIdx.x, t = threadIdx.x;
  if (j >= spbase[NS]) return;
  s2_locate(spbase, NS, j, sh);
  const uint32_t s = sh[0], p = sh[1];
  const uint32_t start = sbase[s], cnt = sbase[s + 1] - start;
  const uint32_t lo = p * SM_PART, hi = min(lo + SM_PART, cnt), ng = 1u << G;
  for (uint32_t q = t; q < ng; q += S_THREADS) hist[q] = 0;
  __syncthreads();
  E x[SM_IPT];
  uint32_t rk[SM_IPT];
#pragma unroll
  for (uint32_t it = 0; it < SM_IPT; it++) {
    const uint32_t e = lo + it * S_THREADS + t;
    if (e < hi) {
      x[it] = tmp[start + e];
      rk[it] = lds_rank_add(hist, (SortEnt<E>::low(x[it]) >> F) & (ng - 1));
    }
  }
  __syncthreads();
  for (uint32_t q = t; q < ng; q += S_THREADS)
    if (hist[q]) cur[q] = atomicAdd(&ccursor[(s << G) + q], hist[q]);
  __syncthreads();
#pragma unroll
  for (uint32_t it = 0; it < SM_IPT; it++) {
    const uint32_t e = lo + it * S_THREADS + t;
    if (e < hi) tmp2[cur[(SortEnt<E>::low(x[it]) >> F) & (ng - 1)] + rk[it]] = x[it];
  }
}

// LDS layout: hist[2^F] | staged values[S2_STAGE] | (KEYS) staged keys[S2_STAGE].
// kb = F + G: the key bits a compact entry carries (SortEnt); an entry's bucket
// is its coarse bin's first bucket + its low F bits.  KEYS false: keys_out is
// neither staged nor stored (it may be null).
template <bool KEYS>
constexpr size_t s2_local_lds(uint32_t nf) {
  return sizeof(uint32_t) * (nf + (KEYS ? 2 : 1) * (size_t)S2_STAGE);
}
template <class E, bool KEYS>
static __global__ void __launch_bounds__(1024) k_msm_s2_local(const E* __restrict__ tmp,
                                                              const uint32_t* __restrict__ cbase,
                                                              const uint32_t* __restrict__ pbase, uint32_t NC,
                                                              uint32_t F, uint32_t kb, uint32_t T,
                                                              uint32_t* __restrict__ fcount,
                                                              uint32_t* __restrict__ keys_out,
                                                              uint32_t* __restrict__ vals_out,
                                                              uint32_t* __restrict__ offsets) {
  extern __shared__ uint32_t s2_lds[];
  __shared__ uint32_t sh[2], wsum[17];
  const uint32_t j = blockIdx.x, t = threadIdx.x;
  // no split bins (the usual case): part j is bin j -- the three loads issue together
  const uint32_t parts = pbase[NC];
  const uint32_t cj0 = j < NC ? cbase[j] : 0u, cj1 = j < NC ? cbase[j + 1] : 0u;
  if (j >= parts) return;
  uint32_t H, p, start, cnt;
  if (parts == NC) {
    H = j;
    p = 0;
    start = cj0;
    cnt = cj1 - cj0;
  } else {
    s2_locate(pbase, NC, j, sh);
    H = sh[0];
    p = sh[1];
    start = cbase[H];
    cnt = cbase[H + 1] - start;
  }
  const uint32_t b0 = H << F, nf = min(1u << F, T - b0), fmask = (1u << F) - 1;
  uint32_t* hist = s2_lds;
  for (uint32_t q = t; q < nf; q += S_THREADS) hist[q] = 0;
  __syncthreads();
  if (cnt <= S2_STAGE) {
    // whole bin in registers: local counting sort staged in LDS, then one
    // coalesced copy of the bin's sorted keys / values
    constexpr uint32_t IPT = S2_STAGE / S_THREADS;
    E x[IPT];
    uint32_t rk[IPT];
#pragma unroll
    for (uint32_t it = 0; it < IPT; it++) {
      const uint32_t e = it * S_THREADS + t;
      if (e < cnt) {
        x[it] = tmp[start + e];
        rk[it] = lds_rank_add(hist, SortEnt<E>::low(x[it]) & fmask);
      }
    }
    block_excl_scan(hist, nf, wsum);
    for (uint32_t f = t; f < nf; f += S_THREADS) offsets[b0 + f] = start + hist[f];
    uint32_t* sv = s2_lds + nf;
    uint32_t* sk = sv + S2_STAGE;  // KEYS only
#pragma unroll
    for (uint32_t it = 0; it < IPT; it++) {
      const uint32_t e = it * S_THREADS + t;
      if (e < cnt) {
        const uint32_t f = SortEnt<E>::low(x[it]) & fmask;
        const uint32_t pos = hist[f] + rk[it];
        if constexpr (KEYS) sk[pos] = b0 + f;
        sv[pos] = SortEnt<E>::val(x[it], kb);
      }
    }
    __syncthreads();
    for (uint32_t q = t; q < cnt; q += S_THREADS) {
      if constexpr (KEYS) keys_out[start + q] = sk[q];
      vals_out[start + q] = sv[q];
    }
  } else if (cnt <= S2_BIG) {
    // too large to stage: two reads, scattered writes
    for (uint32_t e = t; e < cnt; e += S_THREADS) lds_rank_add(hist, SortEnt<E>::low(tmp[start + e]) & fmask);
    block_excl_scan(hist, nf, wsum);
    for (uint32_t f = t; f < nf; f += S_THREADS) offsets[b0 + f] = start + hist[f];
    __syncthreads();
    for (uint32_t e = t; e < cnt; e += S_THREADS) {
      const E x = tmp[start + e];
      const uint32_t f = SortEnt<E>::low(x) & fmask;
      const uint32_t pos = start + lds_rank_add(hist, f);
      if constexpr (KEYS) keys_out[pos] = b0 + f;
      vals_out[pos] = SortEnt<E>::val(x, kb);
    }
  } else {
    const uint32_t lo = p * S2_BIG, hi = min(lo + S2_BIG, cnt);
    for (uint32_t e = lo + t; e < hi; e += S_THREADS) lds_rank_add(hist, SortEnt<E>::low(tmp[start + e]) & fmask);
    __syncthreads();
    for (uint32_t f = t; f < nf; f += S_THREADS)
      if (hist[f]) atomicAdd(&fcount[b0 + f], hist[f]);
  }
}

// The split-bin kernels below run on a capped grid, block-strided over the bins /
// parts: with no split bin (uniform digits) every block returns at once, where a
// block per bin cost ~0.2 ms per launch at 2^24 (213K empty blocks).
constexpr uint32_t S2_SPLIT_GRID = 2048;
static __global__ void __launch_bounds__(1024) k_msm_s2_scan(const uint32_t* __restrict__ cbase,
                                                             const uint32_t* __restrict__ pbase, uint32_t NC,
                                                             uint32_t F, uint32_t T, uint32_t* __restrict__ fcount,
                                                             uint32_t* __restrict__ offsets) {
  extern __shared__ uint32_t hist[];
  __shared__ uint32_t wsum[17];
  if (pbase[NC] == NC) return;  // no split bins
  const uint32_t t = threadIdx.x;
  for (uint32_t H = blockIdx.x; H < NC; H += gridDim.x) {
    const uint32_t start = cbase[H], cnt = cbase[H + 1] - start;
    if (cnt <= S2_BIG) continue;
    const uint32_t b0 = H << F, nf = min(1u << F, T - b0);
    for (uint32_t f = t; f < nf; f += S_THREADS) hist[f] = fcount[b0 + f];
    block_excl_scan(hist, nf, wsum);
    for (uint32_t f = t; f < nf; f += S_THREADS) {
      offsets[b0 + f] = start + hist[f];
      fcount[b0 + f] = start + hist[f];  // now the bucket's write cursor
    }
    __syncthreads();
  }
}

template <class E, bool KEYS>
static __global__ void __launch_bounds__(1024) k_msm_s2_scatter(const E* __restrict__ tmp,
                                                                const uint32_t* __restrict__ cbase,
                                                                const uint32_t* __restrict__ pbase, uint32_t NC,
                                                                uint32_t F, uint32_t kb, uint32_t T,
                                                                uint32_t* __restrict__ fcursor,
                                                                uint32_t* __restrict__ keys_out,
                                                                uint32_t* __restrict__ vals_out) {
  extern __shared__ uint32_t s2_lds[];
  __shared__ uint32_t sh[2];
  const uint32_t t = threadIdx.x, parts = pbase[NC];
  if (parts == NC) return;  // no split bins: nothing to do
  for (uint32_t j = blockIdx.x; j < parts; j += gridDim.x) {
    s2_locate(pbase, NC, j, sh);
    const uint32_t H = sh[0], p = sh[1];
    const uint32_t start = cbase[H], cnt = cbase[H + 1] - start;
    __syncthreads();  // every thread has read sh before the next part's s2_locate
    if (cnt <= S2_BIG) continue;
    const uint32_t b0 = H << F, nf = min(1u << F, T - b0), fmask = (1u << F) - 1;
    uint32_t* hist = s2_lds;
    uint32_t* cur = s2_lds + nf;
    for (uint32_t q = t; q < nf; q += S_THREADS) hist[q] = 0;
    __syncthreads();
    const uint32_t lo = p * S2_BIG, hi = min(lo + S2_BIG, cnt);
    for (uint32_t e = lo + t; e < hi; e += S_THREADS) lds_rank_add(hist, SortEnt<E>::low(tmp[start + e]) & fmask);
    __syncthreads();
    for (uint32_t f = t; f < nf; f += S_THREADS)
      if (hist[f]) cur[f] = atomicAdd(&fcursor[b0 + f], hist[f]);
    __syncthreads();
    for (uint32_t e = lo + t; e < hi; e += S_THREADS) {
      const E x = tmp[start + e];
      const uint32_t f = SortEnt<E>::low(x) & fmask;
      const uint32_t pos = lds_rank_add(cur, f);
      if constexpr (KEYS) keys_out[pos] = b0 + f;
      vals_out[pos] = SortEnt<E>::val(x, kb);
    }
    __syncthreads();  // the LDS is reused by the next part
  }
}

// The passes for one entry width E and with (KEYS) or without the sorted keys.
template <class E, bool KEYS>
static int sort_passes(gm_ctx* ctx, Arena& arena, const SortGeom& g, size_t n, uint32_t W, uint32_t nb,
                       uint32_t shared_stride, const uint32_t* dig, const uint32_t* scount, uint32_t* keys_out,
                       uint32_t* vals_out, uint32_t* offsets) {
  hipStream_t st = ctx->stream;
  const uint32_t shift = g.F + g.G;  // pass-1 bin = b >> shift (super-bin, or coarse bin when G = 0)
  int rc;
  DevBuf sbase, scursor, spbase, tmp;
  if ((rc = sbase.alloc(arena, 4 * ((size_t)g.NS + 1))) || (rc = scursor.alloc(arena, 4 * (size_t)g.NS)) ||
      (rc = spbase.alloc(arena, 4 * ((size_t)g.NS + 1))) || (rc = tmp.alloc(arena, sizeof(E) * g.M)))
    return rc;
  hipLaunchKernelGGL(k_msm_s1_scan, dim3(1), dim3(S_THREADS), 0, st, scount, g.NS, g.T, g.G ? SM_PART : S2_BIG,
                     sbase.as<uint32_t>(), scursor.as<uint32_t>(), spbase.as<uint32_t>(), offsets);
  // bins one pass-1 block touches: its window's own nb >> shift in the plain layout
  const uint32_t nh = (!shared_stride && (1u << shift) <= nb) ? nb >> shift : g.NS;
  // staged (coalesced-write) pass 1 while its LDS fits: 64 KB of entries plus
  // three words per touched bin (up to ~112 KB at 4,096 bins: gfx950 has 160 KB
  // per workgroup; a device with less takes the direct scatter)
  const size_t lds = 8 * (size_t)S1_PTS + sizeof(uint32_t) * (3 * (size_t)nh + 17);
  if (nh <= 4096 && lds <= device_lds_per_block(ctx->device)) {
    hipLaunchKernelGGL((k_msm_s1_scatter_st<E, S1_PPT>), dim3(blocks_for(n, S1_PTS), W), dim3(S_THREADS), lds, st, dig,
                       (uint32_t)n, nb, shared_stride, shift, g.NS, nh, scursor.as<uint32_t>(), tmp.as<E>());
    GM_HIP(hipGetLastError());
  } else {
    hipLaunchKernelGGL(k_msm_s1_scatter<E>, dim3(blocks_for(n, S1_PTS), W), dim3(S_THREADS),
                       2 * sizeof(uint32_t) * nh, st, dig, (uint32_t)n, nb, shared_stride, shift, g.NS, nh,
                       scursor.as<uint32_t>(), tmp.as<E>());
  }
  // final pass input: coarse-binned entries with their bases / part table
  const E* fin = tmp.as<E>();
  const uint32_t *cbase = sbase.as<uint32_t>(), *pbase = spbase.as<uint32_t>();
  if (g.G) {
    DevBuf ccount, cb, ccur, cparts, pb, bsum, tmp2;
    if ((rc = ccount.alloc(arena, 4 * (size_t)g.NC)) || (rc = cb.alloc(arena, 4 * ((size_t)g.NC + 1))) ||
        (rc = ccur.alloc(arena, 4 * (size_t)g.NC)) || (rc = cparts.alloc(arena, 4 * (size_t)g.NC)) ||
        (rc = pb.alloc(arena, 4 * ((size_t)g.NC + 1))) || (rc = bsum.alloc(arena, 4 * scan_ws_words(g.NC))) ||
        (rc = tmp2.alloc(arena, sizeof(E) * g.M)))
      return rc;
    const size_t mparts = (size_t)g.NS + g.M / SM_PART + 1;
    GM_HIP(hipMemsetAsync(ccount.p, 0, 4 * (size_t)g.NC, st));
    hipLaunchKernelGGL(k_msm_sm_count<E>, dim3((unsigned)mparts), dim3(S_THREADS), 0, st, tmp.as<E>(),
                       sbase.as<uint32_t>(), spbase.as<uint32_t>(), g.NS, g.F, g.G, ccount.as<uint32_t>());
    hipLaunchKernelGGL(k_msm_sm_scan, dim3(g.NS), dim3(S_THREADS), 0, st, ccount.as<uint32_t>(), sbase.as<uint32_t>(),
                       g.G, g.NC, cb.as<uint32_t>(), ccur.as<uint32_t>(), cparts.as<uint32_t>());
    // NC <= NS << G <= 2^23 coarse bins (msm_sort_digits checks NS <= 8192, G <= 10)
    if ((rc = device_excl_scan(ctx, cparts.as<uint32_t>(), g.NC, pb.as<uint32_t>(), bsum.as<uint32_t>()))) return rc;
    hipLaunchKernelGGL(k_msm_sm_scatter<E>, dim3((unsigned)mparts), dim3(S_THREADS), 0, st, tmp.as<E>(),
                       sbase.as<uint32_t>(), spbase.as<uint32_t>(), g.NS, g.F, g.G, ccur.as<uint32_t>(),
                       tmp2.as<E>());
    fin = tmp2.as<E>();
    cbase = cb.as<uint32_t>();
    pbase = pb.as<uint32_t>();
  }
  DevBuf fcount;
  if ((rc = fcount.alloc(arena, 4 * (size_t)g.T))) return rc;
  const uint32_t nfmax = std::min<uint32_t>(1u << g.F, g.T);
  // every coarse bin has >= 1 part; split bins add at most M / S2_BIG more
  const size_t maxparts = (size_t)g.NC + g.M / S2_BIG + 1;
  GM_HIP(hipMemsetAsync(fcount.p, 0, sizeof(uint32_t) * g.T, st));
  hipLaunchKernelGGL((k_msm_s2_local<E, KEYS>), dim3((unsigned)maxparts), dim3(S_THREADS), s2_local_lds<KEYS>(nfmax),
                     st, fin, cbase, pbase, g.NC, g.F, shift, g.T, fcount.as<uint32_t>(), keys_out, vals_out, offsets);
  hipLaunchKernelGGL(k_msm_s2_scan, dim3(std::min<uint32_t>(g.NC, S2_SPLIT_GRID)), dim3(S_THREADS),
                     sizeof(uint32_t) * nfmax, st, cbase, pbase, g.NC, g.F, g.T, fcount.as<uint32_t>(), offsets);
  hipLaunchKernelGGL((k_msm_s2_scatter<E, KEYS>), dim3((unsigned)std::min<size_t>(maxparts, S2_SPLIT_GRID)),
                     dim3(S_THREADS), 2 * sizeof(uint32_t) * nfmax, st, fin, cbase, pbase, g.NC, g.F, shift, g.T,
                     fcount.as<uint32_t>(), keys_out, vals_out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int msm_sort_digits(gm_ctx* ctx, Arena& arena, const SortGeom& g, size_t n, uint32_t W, uint32_t nb,
                    uint32_t shared_stride, const uint32_t* dig, const uint32_t* scount, uint32_t* keys_out,
                    uint32_t* vals_out, uint32_t* offsets) {
  if (g.NS == 0 || g.NS > 8192 || g.F > 13 || g.G > 10 || g.NC != (g.T + (1u << g.F) - 1) >> g.F ||
      g.NS != (g.T + (1u << (g.F + g.G)) - 1) >> (g.F + g.G)) {
    set_error("msm sort: bad geometry");
    return GM_ERR_INVALID;
  }
  // compact entries hold F + G key bits, the sign, and an index below 2^(31 - F - G)
  const size_t vmax = shared_stride ? (size_t)W * shared_stride : n;
  if (g.compact && (vmax - 1) >> (31 - g.F - g.G)) {
    set_error("msm sort: values do not fit a compact entry");
    return GM_ERR_INVALID;
  }
  auto run = g.compact ? (keys_out ? sort_passes<uint32_t, true> : sort_passes<uint32_t, false>)
                       : (keys_out ? sort_passes<uint64_t, true> : sort_passes<uint64_t, false>);
  return run(ctx, arena, g, n, W, nb, shared_stride, dig, scount, keys_out, vals_out, offsets);
}

// ---------------------------------------------------------------------------
// Piece plan of the G1 accumulation (MsmPlan, msm.hpp): buckets cut into
// ceil(len / T) pieces of nearly equal length, the pieces counting-sorted by
// length, longest first.  Three small kernels over the bucket offsets:
//   k_msm_pp_hist     pieces per length class (LDS histogram, then one global
//                     atomic per class per block)
//   k_msm_pp_scan     one block: class bases, longest class first; piece count
//   k_msm_pp_scatter  the descriptors, the part slots of the cut buckets
//                     (pbase, one global reservation per block) and the bucket
//                     of every part slot.  A bucket of more than PP_COOP pieces
//                     (skewed scalars) is written by the whole block.
// The order of the pieces inside a class, and of the cut buckets' part ranges,
// follows the atomics: the group law makes the result independent of it.
// ---------------------------------------------------------------------------
constexpr uint32_t PP_THREADS = 256, PP_PER = 2, PP_CLASSES = PIECE_MAX_LEN + 1, PP_COOP = 32, PP_BIG = 256;

// bucket of len entries -> p pieces: r of q + 1 entries first, then p - r of q
__device__ __forceinline__ void pp_split(uint32_t len, uint32_t T, uint32_t& p, uint32_t& q, uint32_t& r) {
  p = (len + T - 1) / T;
  q = len / p;
  r = len - q * p;
}
__device__ __forceinline__ void pp_write(uint32_t b, uint32_t bs, uint32_t p, uint32_t q, uint32_t r, uint32_t i,
                                         uint32_t s0, uint32_t s1, uint32_t pb, uint4* __restrict__ pieces,
                                         uint32_t* __restrict__ partb) {
  const bool big = i < r;
  const uint32_t start = big ? bs + i * (q + 1) : bs + r * (q + 1) + (i - r) * q;
  pieces[big ? s1 + i : s0 + (i - r)] = make_uint4(start, big ? q + 1 : q, p == 1 ? b : PIECE_PART | (pb + i), 0u);
  if (p > 1) partb[pb + i] = b;
}

static __global__ void __launch_bounds__(PP_THREADS) k_msm_pp_hist(const uint32_t* __restrict__ offsets,
                                                                   uint32_t total, uint32_t T,
                                                                   uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[PP_CLASSES];
  const uint32_t t = threadIdx.x;
  if (t < PP_CLASSES) h[t] = 0;
  __syncthreads();
  for (uint32_t k = 0; k < PP_PER; k++) {
    const uint32_t b = (blockIdx.x * PP_PER + k) * PP_THREADS + t;
    if (b >= total) break;
    const uint32_t len = offsets[b + 1] - offsets[b];
    if (!len) continue;
    uint32_t p, q, r;
    pp_split(len, T, p, q, r);
    atomicAdd(&h[q], p - r);
    if (r) atomicAdd(&h[q + 1], r);
  }
  __syncthreads();
  if (t < PP_CLASSES && h[t]) atomicAdd(&hist[t], h[t]);
}

// cursor[l] = pieces longer than l; pcount[0] = all pieces, pcount[1] = 0
static __global__ void __launch_bounds__(PP_THREADS) k_msm_pp_scan(const uint32_t* __restrict__ hist,
                                                                   uint32_t* __restrict__ cursor,
                                                                   uint32_t* __restrict__ pcount) {
  __shared__ uint32_t h[PP_CLASSES];
  const uint32_t t = threadIdx.x;
  if (t < PP_CLASSES) h[t] = hist[t];
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (int l = (int)PP_CLASSES - 1; l >= 0; l--) {
      const uint32_t c = h[l];
      h[l] = run;
      run += c;
    }
    pcount[0] = run;
    pcount[1] = 0;
  }
  __syncthreads();
  if (t < PP_CLASSES) cursor[t] = h[t];
}

static __global__ void __launch_bounds__(PP_THREADS) k_msm_pp_scatter(const uint32_t* __restrict__ offsets,
                                                                      uint32_t total, uint32_t T,
                                                                      uint32_t* __restrict__ cursor,
                                                                      uint32_t* __restrict__ pcount,
                                                                      uint4* __restrict__ pieces,
                                                                      uint32_t* __restrict__ pbase,
                                                                      uint32_t* __restrict__ partb) {
  __shared__ uint32_t cnt[PP_CLASSES], base[PP_CLASSES];
  __shared__ uint32_t nparts, part0, nbig;
  __shared__ uint32_t bigb[PP_BIG], bigs0[PP_BIG], bigs1[PP_BIG], bigpb[PP_BIG];
  const uint32_t t = threadIdx.x;
  if (t < PP_CLASSES) cnt[t] = 0;
  if (t == 0) {
    nparts = 0;
    nbig = 0;
  }
  __syncthreads();
  uint32_t loc[PP_PER];  // the bucket's first part slot inside the block
#pragma unroll
  for (uint32_t k = 0; k < PP_PER; k++) {
    const uint32_t b = (blockIdx.x * PP_PER + k) * PP_THREADS + t;
    loc[k] = 0;
    if (b >= total) continue;
    const uint32_t len = offsets[b + 1] - offsets[b];
    if (!len) continue;
    uint32_t p, q, r;
    pp_split(len, T, p, q, r);
    atomicAdd(&cnt[q], p - r);
    if (r) atomicAdd(&cnt[q + 1], r);
    if (p > 1) loc[k] = atomicAdd(&nparts, p);
  }
  __syncthreads();
  if (t < PP_CLASSES) {
    if (cnt[t]) base[t] = atomicAdd(&cursor[t], cnt[t]);
    cnt[t] = 0;
  }
  if (t == 0 && nparts) part0 = atomicAdd(&pcount[1], nparts);
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < PP_PER; k++) {
    const uint32_t b = (blockIdx.x * PP_PER + k) * PP_THREADS + t;
    if (b >= total) continue;
    const uint32_t bs = offsets[b], len = offsets[b + 1] - bs;
    if (!len) continue;
    uint32_t p, q, r;
    pp_split(len, T, p, q, r);
    const uint32_t s0 = base[q] + atomicAdd(&cnt[q], p - r);
    const uint32_t s1 = r ? base[q + 1] + atomicAdd(&cnt[q + 1], r) : 0u;
    const uint32_t pb = p > 1 ? part0 + loc[k] : 0u;
    if (p > 1) pbase[b] = pb;
    if (p > PP_COOP) {
      const uint32_t e = atomicAdd(&nbig, 1u);
      if (e < PP_BIG) {
        bigb[e] = b;
        bigs0[e] = s0;
        bigs1[e] = s1;
        bigpb[e] = pb;
        continue;
      }
    }
    for (uint32_t i = 0; i < p; i++) pp_write(b, bs, p, q, r, i, s0, s1, pb, pieces, partb);
  }
  __syncthreads();
  const uint32_t nb = min(nbig, PP_BIG);
  for (uint32_t e = 0; e < nb; e++) {
    const uint32_t b = bigb[e], bs = offsets[b], len = offsets[b + 1] - bs;
    uint32_t p, q, r;
    pp_split(len, T, p, q, r);
    for (uint32_t i = t; i < p; i += PP_THREADS) pp_write(b, bs, p, q, r, i, bigs0[e], bigs1[e], bigpb[e], pieces, partb);
  }
}

int msm_piece_plan(gm_ctx* ctx, Arena& arena, MsmPlan& plan, uint32_t T) {
  if (T == 0 || T > PIECE_MAX_LEN) {
    set_error("msm piece plan: bad piece length");
    return GM_ERR_INVALID;
  }
  hipStream_t st = ctx->stream;
  const size_t M = plan.M, total = plan.total;
  plan.T = T;
  // one piece per T entries plus one per non-empty bucket; a cut bucket (len > T)
  // has at most 2 len / T parts
  plan.max_pieces = M / T + std::min(total, M) + 1;
  plan.max_parts = std::min(2 * M / T, M / T + total) + 1;
  if (plan.max_pieces >= (size_t(1) << 31)) {
    set_error("msm piece plan: too many pieces");
    return GM_ERR_INVALID;
  }
  int rc;
  DevBuf pieces, pcount, pbase, partb, hist;
  if ((rc = pieces.alloc(arena, sizeof(uint4) * plan.max_pieces)) || (rc = pcount.alloc(arena, 16)) ||
      (rc = pbase.alloc(arena, sizeof(uint32_t) * total)) ||
      (rc = partb.alloc(arena, sizeof(uint32_t) * plan.max_parts)) ||
      (rc = hist.alloc(arena, sizeof(uint32_t) * 2 * PP_CLASSES)))
    return rc;
  uint32_t* h = hist.as<uint32_t>();
  const unsigned blocks = blocks_for(total, PP_THREADS * PP_PER);
  GM_HIP(hipMemsetAsync(h, 0, sizeof(uint32_t) * PP_CLASSES, st));
  hipLaunchKernelGGL(k_msm_pp_hist, dim3(blocks), dim3(PP_THREADS), 0, st, plan.offsets, plan.total, T, h);
  hipLaunchKernelGGL(k_msm_pp_scan, dim3(1), dim3(PP_THREADS), 0, st, h, h + PP_CLASSES, pcount.as<uint32_t>());
  hipLaunchKernelGGL(k_msm_pp_scatter, dim3(blocks), dim3(PP_THREADS), 0, st, plan.offsets, plan.total, T,
                     h + PP_CLASSES, pcount.as<uint32_t>(), pieces.as<uint4>(), pbase.as<uint32_t>(),
                     partb.as<uint32_t>());
  GM_HIP(hipGetLastError());
  plan.pieces = pieces.as<uint4>();
  plan.pcount = pcount.as<uint32_t>();
  plan.pbase = pbase.as<uint32_t>();
  plan.partb = partb.as<uint32_t>();
  return GM_OK;
}

// Shared-bucket cost model: n*W accumulation adds + ~3 reduction adds per
// bucket, paid once (not per window).  Picks c = 20 / W = 13 for 2^20 BN254
// points and c = 22 / W = 12 for 2^24.
MsmPrecomp msm_choose_precomp(size_t n, int bits) {
  MsmPrecomp best;
  double best_cost = 1e300;
  for (uint32_t c = 8; c <= 24; c++) {
    const uint32_t W = (uint32_t)((bits + 1 + c - 1) / c);
    const double cost = (double)n * W + 3.0 * (double)(1u << (c - 1));
    if (cost < best_cost) {
      best_cost = cost;
      best.c = c;
      best.W = W;
    }
  }
  best.stride = n;
  best.narrow = precomp_narrow(best.c, best.W, bits);
  return best;
}

}  // namespace gm
