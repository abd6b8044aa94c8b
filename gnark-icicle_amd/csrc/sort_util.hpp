// Block-level building blocks of the counting sorts and scans (the MSM bucket
// sort in msm_impl.hpp and msm_sort.hip, the wires permutation's radix sort and
// link, the device-wide scan in scan.hip): wave / block scans of u32, by sum or
// by max, and an LDS counter increment that returns the entry's rank.  All
// assume 1024-thread blocks of wave64 unless they say otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gm {

constexpr uint32_t S_THREADS = 1024;

// the scans' operator: sum mod 2^32, or max (identity 0 for both)
template <bool MAX>
__device__ __forceinline__ uint32_t scan_op(uint32_t a, uint32_t b) {
  return MAX ? max(a, b) : a + b;
}

// inclusive scan over the wave (any block size)
template <bool MAX>
__device__ __forceinline__ uint32_t wave_incl(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if (lane >= (uint32_t)d) v = scan_op<MAX>(v, u);
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) { return wave_incl<false>(v); }

// Exclusive scan (sum, or max with identity 0) of one value per thread over a
// 1024-thread block; *total receives the block's result.  ws: 17 words of LDS.
// Synchronises on entry and exit.
template <bool MAX>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* ws, uint32_t* total) {
  __syncthreads();
  const uint32_t t = threadIdx.x, lane = t & 63;
  const uint32_t inc = wave_incl<MAX>(v);
  uint32_t exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = 0;
  if (lane == 63) ws[t >> 6] = inc;
  __syncthreads();
  if (t < 64) {
    const uint32_t x = t < 16 ? ws[t] : 0u;
    const uint32_t xi = wave_incl<MAX>(x);
    uint32_t xe = __shfl_up(xi, 1, 64);
    if (t == 0) xe = 0;
    if (t < 16) ws[t] = xe;
    if (t == 15) ws[16] = xi;
  }
  __syncthreads();
  const uint32_t r = scan_op<MAX>(ws[t >> 6], exc);
  *total = ws[16];
  __syncthreads();
  return r;
}

// Exclusive sum scan of a[0, len) (LDS) by a 1024-thread block; returns the total.
// wsum: 17 words of LDS.  Synchronises on entry and exit.  (Not written over
// block_excl: the MSM sort's kernels would change their register use.)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t* a, uint32_t len, uint32_t* wsum) {
  __syncthreads();
  const uint32_t t = threadIdx.x;
  const uint32_t per = (len + S_THREADS - 1) / S_THREADS;
  const uint32_t lo = min(t * per, len), hi = min(lo + per, len);
  uint32_t s = 0;
  for (uint32_t q = lo; q < hi; q++) s += a[q];
  const uint32_t inc = wave_incl_scan(s);
  if ((t & 63) == 63) wsum[t >> 6] = inc;
  __syncthreads();
  if (t < 64) {
    const uint32_t v = t < S_THREADS / 64 ? wsum[t] : 0u;
    const uint32_t vi = wave_incl_scan(v);
    if (t < S_THREADS / 64) wsum[t] = vi - v;
    if (t == S_THREADS / 64 - 1) wsum[S_THREADS / 64] = vi;
  }
  __syncthreads();
  uint32_t run = wsum[t >> 6] + inc - s;
  for (uint32_t q = lo; q < hi; q++) {
    const uint32_t x = a[q];
    a[q] = run;
    run += x;
  }
  const uint32_t total = wsum[S_THREADS / 64];
  __syncthreads();
  return total;
}

// rank = hist[key]++ for the active lanes.  When every active lane of the wave
// has the same key (skewed scalars: one huge bucket) the wave does ONE atomic
// instead of 64 serialised same-address LDS atomics.
__device__ __forceinline__ uint32_t lds_rank_add(uint32_t* hist, uint32_t key) {
  const uint32_t k0 = __builtin_amdgcn_readfirstlane(key);
  const uint64_t active = __ballot(1);
  if (__ballot(key == k0) == active) {
    const uint32_t below = (uint32_t)__popcll(active & __lanemask_lt());
    uint32_t old = 0;
    if (below == 0) old = atomicAdd(&hist[k0], (uint32_t)__popcll(active));
    return __builtin_amdgcn_readfirstlane(old) + below;
  }
  return atomicAdd(&hist[key], 1u);
}

}  // namespace gm
