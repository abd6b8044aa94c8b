// The device-wide exclusive scan of u32 (scan.hip): the offsets of the MSM
// sort's parts, of the Groth16 setup's columns and compactions, and of the
// wires permutation's radix passes.
#pragma once
#include <cstddef>
#include <cstdint>
#include "runtime.hpp"

namespace gm {
// out[i] = in[0] + .. + in[i-1] for i <= n (out has n + 1 words; out[n] is the total),
// sums mod 2^32.  out may be in (in place).  ws: scan_ws_words(n) u32 of workspace,
// need not be initialised.  Any n that fits the allocation; n == 0 writes out[0] = 0.
// Queued on ctx->stream; nothing synchronises.
size_t scan_ws_words(size_t n);
int device_excl_scan(gm_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out, uint32_t* ws);
// a[i] = a[0] op .. op a[i-1] in place by one block, op the sum mod 2^32 or (max)
// the maximum, both from 0.  For short arrays: the block walks a in 1024 slices.
int block_scan_inplace(gm_ctx* ctx, uint32_t* a, uint32_t len, bool max);
}  // namespace gm
