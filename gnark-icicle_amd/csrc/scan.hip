// Device-wide exclusive scan of u32: blocks of SCAN_BLK words scan themselves
// through LDS and leave their totals in the workspace, one block scans the
// totals (in slices, so any number of them) and writes the grand total, and a
// grid-stride pass adds every block's offset.
#include "scan.hpp"
#include "sort_util.hpp"

namespace gm {

namespace {

constexpr uint32_t SCAN_BLK = 4096;

// in and out may be the same array: a block reads its words before it writes them
__global__ void __launch_bounds__(S_THREADS)
    k_scan_local(const uint32_t* in, size_t n, uint32_t* out, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t a[SCAN_BLK], wsum[17];
  const size_t base = (size_t)blockIdx.x * SCAN_BLK;
  const uint32_t len = (uint32_t)min((size_t)SCAN_BLK, n - base);
  for (uint32_t q = threadIdx.x; q < len; q += S_THREADS) a[q] = in[base + q];
  const uint32_t tot = block_excl_scan(a, len, wsum);
  for (uint32_t q = threadIdx.x; q < len; q += S_THREADS) out[base + q] = a[q];
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
// one block, any length: thread t scans the t-th slice of a in place (sum, or max
// with identity 0); *total (unless null) receives the result over all of a
template <bool MAX>
__global__ void __launch_bounds__(S_THREADS)
    k_scan_one(uint32_t* __restrict__ a, uint32_t len, uint32_t* __restrict__ total) {
  __shared__ uint32_t ws[17];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (len + S_THREADS - 1) / S_THREADS;
  const uint32_t lo = min(t * per, len), hi = min(lo + per, len);
  uint32_t acc = 0;
  for (uint32_t q = lo; q < hi; q++) acc = scan_op<MAX>(acc, a[q]);
  uint32_t tot;
  uint32_t run = block_excl<MAX>(acc, ws, &tot);
  for (uint32_t q = lo; q < hi; q++) {
    const uint32_t x = a[q];
    a[q] = run;
    run = scan_op<MAX>(run, x);
  }
  if (total && t == 0) *total = tot;
}
__global__ void __launch_bounds__(256)
    k_scan_add(uint32_t* __restrict__ out, size_t n, const uint32_t* __restrict__ bsum) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] += bsum[i / SCAN_BLK];
}

}  // namespace

size_t scan_ws_words(size_t n) { return (n + SCAN_BLK - 1) / SCAN_BLK; }

int device_excl_scan(gm_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out, uint32_t* ws) {
  if (n == 0) {
    GM_HIP(hipMemsetAsync(out, 0, sizeof(uint32_t), ctx->stream));
    return GM_OK;
  }
  const size_t nblk = scan_ws_words(n);
  if (nblk > 0x7fffffffu) {  // the grid's limit; 2^43 words
    set_error("scan: too long");
    return GM_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_scan_local, dim3((unsigned)nblk), dim3(S_THREADS), 0, ctx->stream, in, n, out, ws);
  hipLaunchKernelGGL(k_scan_one<false>, dim3(1), dim3(S_THREADS), 0, ctx->stream, ws, (uint32_t)nblk, out + n);
  hipLaunchKernelGGL(k_scan_add, dim3(grid_for(n)), dim3(256), 0, ctx->stream, out, n, (const uint32_t*)ws);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int block_scan_inplace(gm_ctx* ctx, uint32_t* a, uint32_t len, bool max) {
  auto k = max ? k_scan_one<true> : k_scan_one<false>;
  hipLaunchKernelGGL(k, dim3(1), dim3(S_THREADS), 0, ctx->stream, a, len, (uint32_t*)nullptr);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // namespace gm
