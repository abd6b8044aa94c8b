// Test hook for the pairing's layers (include/gnark_mi355x_testhooks.h,
// gm_test_pairing_op): each operation of pairing_impl.hpp element-wise, one lane
// per element.  Not in the product library.
#include "pairing_impl.hpp"
#include "../../include/gnark_mi355x_testhooks.h"

namespace gm {

template <class C, int OP>
__global__ void __launch_bounds__(PR_TPB)
    k_pairing_op(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n, uint32_t* __restrict__ out) {
  using T = Pr<C>;
  using F12 = typename T::F12;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const F12 x = T::load12(a, i);
  F12 r;
  if constexpr (OP == GM_TPAIR_MUL) {
    r = T::mul12(x, T::load12(b, i));
  } else if constexpr (OP == GM_TPAIR_SQR) {
    r = T::sqr12(x);
  } else if constexpr (OP == GM_TPAIR_INV) {
    r = T::inv12(x);
  } else if constexpr (OP == GM_TPAIR_CONJ) {
    r = T::conj12(x);
  } else if constexpr (OP == GM_TPAIR_FROB1) {
    r = T::template frob12<1>(x);
  } else if constexpr (OP == GM_TPAIR_FROB2) {
    r = T::template frob12<2>(x);
  } else if constexpr (OP == GM_TPAIR_CYC_SQR) {
    r = T::cyc_sqr12(x);
  } else if constexpr (OP == GM_TPAIR_LINE_MUL) {
    const F12 y = T::load12(b, i);
    typename T::Line l;
    if constexpr (!T::K::M_TWIST) {
      l.ly = y.c0.b0;  // w^0
      l.lx = y.c1.b0;  // w^1
      l.lc = y.c1.b1;  // w^3
    } else {
      l.lc = y.c0.b0;  // w^0
      l.lx = y.c0.b1;  // w^2
      l.ly = y.c1.b1;  // w^3
    }
    r = T::line_mul12(x, l);
  } else if constexpr (OP == GM_TPAIR_EXP_U) {
    r = T::exp_abs_u12(x);
  } else {
    static_assert(OP == GM_TPAIR_FINAL_EXP, "unknown pairing test op");
    r = T::final_exp(x);
  }
  T::store12(out, i, r);
}

template <class C, int OP>
static void launch_op(gm_ctx* ctx, const void* a, const void* b, size_t n, void* out) {
  hipLaunchKernelGGL((k_pairing_op<C, OP>), dim3(blocks_for(n, PR_TPB)), dim3(PR_TPB), 0, ctx->stream,
                     (const uint32_t*)a, (const uint32_t*)b, n, (uint32_t*)out);
}

template <class C>
static int pairing_op_t(gm_ctx* ctx, int op, const void* a, const void* b, size_t n, void* out) {
  switch (op) {
    case GM_TPAIR_MUL: launch_op<C, GM_TPAIR_MUL>(ctx, a, b, n, out); break;
    case GM_TPAIR_SQR: launch_op<C, GM_TPAIR_SQR>(ctx, a, b, n, out); break;
    case GM_TPAIR_INV: launch_op<C, GM_TPAIR_INV>(ctx, a, b, n, out); break;
    case GM_TPAIR_CONJ: launch_op<C, GM_TPAIR_CONJ>(ctx, a, b, n, out); break;
    case GM_TPAIR_FROB1: launch_op<C, GM_TPAIR_FROB1>(ctx, a, b, n, out); break;
    case GM_TPAIR_FROB2: launch_op<C, GM_TPAIR_FROB2>(ctx, a, b, n, out); break;
    case GM_TPAIR_CYC_SQR: launch_op<C, GM_TPAIR_CYC_SQR>(ctx, a, b, n, out); break;
    case GM_TPAIR_LINE_MUL: launch_op<C, GM_TPAIR_LINE_MUL>(ctx, a, b, n, out); break;
    case GM_TPAIR_EXP_U: launch_op<C, GM_TPAIR_EXP_U>(ctx, a, b, n, out); break;
    case GM_TPAIR_FINAL_EXP: launch_op<C, GM_TPAIR_FINAL_EXP>(ctx, a, b, n, out); break;
    case GM_TPAIR_MILLER:
      hipLaunchKernelGGL((k_pairing_miller<C>), dim3(blocks_for(n, PR_TPB)), dim3(PR_TPB), 0, ctx->stream,
                         (const uint32_t*)a, (const uint32_t*)b, n, (uint32_t*)out);
      break;
    default: return GM_ERR_INVALID;
  }
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

}  // namespace gm

using namespace gm;

extern "C" int gm_test_pairing_op(gm_ctx* ctx, int curve, int op, const void* a_dev, const void* b_dev, size_t n,
                                  void* out_dev) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_test_pairing_op")) return rc;
  const bool needs_b = op == GM_TPAIR_MUL || op == GM_TPAIR_LINE_MUL || op == GM_TPAIR_MILLER;
  if (!ctx || op < 0 || op >= GM_TPAIR_OPS || (n && (!a_dev || !out_dev || (needs_b && !b_dev)))) return GM_ERR_INVALID;
  if ((uintptr_t)a_dev % 16 || (uintptr_t)b_dev % 16 || (uintptr_t)out_dev % 16) return GM_ERR_INVALID;
  if (n == 0) return GM_OK;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE(curve, pairing_op_t<C>(ctx, op, a_dev, b_dev, n, out_dev));
}
