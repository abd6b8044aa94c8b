// The wire tables of a PLONK circuit resident on the device, and l, r, o as a
// gather through them.  gnark's evaluateLROSmallDomain
// (constraint/bls12-377/system.go) fills solution.L / R / O row by row from the
// solver's values through three wire ids that are fixed when the circuit is
// compiled:
//   l[i] = values[xa[i]]   r[i] = values[xb[i]]   o[i] = values[xc[i]]
// With the ids uploaded once per circuit only the values cross PCIe per proof
// (the PLONK twin of r1cs.hip).  The rows come complete from the caller,
// placeholder and padding rows included; every id is checked against nb_wires
// before the upload, so the kernel reads inside the witness without a check of
// its own.
//
// Elements are 32-byte gnark words moved as they are: no field arithmetic, one
// kernel for both curves.  Two lanes share an element, one per 16-byte half, so
// a wave's stores are 1 KiB contiguous per output and every access is 16 bytes
// wide; the ids are read as coalesced u32 (both lanes of a pair read the same
// word).  The scatter behind the sparse BSB22 input is the same kernel turned
// round.
#include <algorithm>

#include "plonk_wires.hpp"
#include "runtime.hpp"

namespace gm {

void plonk_wires_release(gm_plonk_wires* w) {
  if (!w) return;
  if (w->ctx) {
    auto& v = w->ctx->plonk_wires;
    v.erase(std::remove(v.begin(), v.end(), w), v.end());
    hipSetDevice(w->ctx->device);
  }
  if (w->tab) hipFree(w->tab);
  delete w;
}

namespace {

constexpr unsigned WIRES_TPB = 256;  // the block of grid_for (runtime.hpp)

// lane t: half t & 1 of row t >> 1 of all three outputs
__global__ void __launch_bounds__(WIRES_TPB)
    k_gather_lro(const uint32_t* __restrict__ tab, size_t n, const uint4* __restrict__ witness,
                 uint4* __restrict__ l, uint4* __restrict__ r, uint4* __restrict__ o) {
  const size_t stride = (size_t)gridDim.x * WIRES_TPB;
  for (size_t t = (size_t)blockIdx.x * WIRES_TPB + threadIdx.x; t < 2 * n; t += stride) {
    const size_t row = t >> 1, half = t & 1;
    const size_t a = tab[row], b = tab[n + row], c = tab[2 * n + row];
    const uint4 va = witness[2 * a + half];
    const uint4 vb = witness[2 * b + half];
    const uint4 vc = witness[2 * c + half];
    l[t] = va;
    r[t] = vb;
    o[t] = vc;
  }
}

// lane t: half t & 1 of pair t >> 1
__global__ void __launch_bounds__(WIRES_TPB)
    k_scatter_rows(uint4* __restrict__ dst, const uint32_t* __restrict__ rows, const uint4* __restrict__ values,
                   size_t count) {
  const size_t stride = (size_t)gridDim.x * WIRES_TPB;
  for (size_t t = (size_t)blockIdx.x * WIRES_TPB + threadIdx.x; t < 2 * count; t += stride) {
    const size_t row = rows[t >> 1];
    dst[2 * row + (t & 1)] = values[t];
  }
}

int refuse(const std::string& msg) {
  set_error("plonk wires: " + msg);
  return GM_ERR_INVALID;
}

}  // namespace

int plonk_wires_upload(gm_ctx* ctx, size_t n, size_t nb_wires, const uint32_t* xa, const uint32_t* xb,
                       const uint32_t* xc, gm_plonk_wires** out) {
  if (n < 8 || (n & (n - 1))) return refuse("n must be a power of two >= 8");
  if (nb_wires == 0 || nb_wires > 0xffffffffull) return refuse("nb_wires must lie in [1, 2^32 - 1]");
  const uint32_t* const tabs[3] = {xa, xb, xc};
  static const char* const names[3] = {"xa", "xb", "xc"};
  for (int k = 0; k < 3; k++)
    for (size_t i = 0; i < n; i++)
      if (tabs[k][i] >= nb_wires)
        return refuse(std::string(names[k]) + "[" + std::to_string(i) + "] = " + std::to_string(tabs[k][i]) +
                      " is not below nb_wires = " + std::to_string(nb_wires));
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  gm_plonk_wires* w = new gm_plonk_wires;
  w->n = n;
  w->nb_wires = nb_wires;
  const hipError_t e = hipMalloc((void**)&w->tab, 3 * n * sizeof(uint32_t));
  if (e != hipSuccess) {
    delete w;
    set_error(std::string("plonk wires: hipMalloc(") + std::to_string(3 * n * sizeof(uint32_t)) +
              "): " + hipGetErrorString(e));
    return GM_ERR_OOM;
  }
  for (int k = 0; k < 3; k++) {
    // synchronous: no host pointer is read after the call returns
    const hipError_t c = hipMemcpy(w->tab + k * n, tabs[k], n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (c != hipSuccess) {
      plonk_wires_release(w);
      set_error(std::string("plonk wires: upload of ") + names[k] + ": " + hipGetErrorString(c));
      return GM_ERR_DEVICE;
    }
  }
  w->ctx = ctx;
  ctx->plonk_wires.push_back(w);
  *out = w;
  return GM_OK;
}

int plonk_gather_lro_device(gm_ctx* ctx, const gm_plonk_wires* w, const void* witness, void* l, void* r, void* o) {
  hipLaunchKernelGGL(k_gather_lro, dim3(grid_for(2 * w->n)), dim3(WIRES_TPB), 0, ctx->stream, w->tab, w->n,
                     (const uint4*)witness, (uint4*)l, (uint4*)r, (uint4*)o);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int plonk_scatter_rows_device(gm_ctx* ctx, void* dst, const uint32_t* rows, const void* values, size_t count) {
  if (count == 0) return GM_OK;
  hipLaunchKernelGGL(k_scatter_rows, dim3(grid_for(2 * count)), dim3(WIRES_TPB), 0, ctx->stream, (uint4*)dst, rows,
                     (const uint4*)values, count);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // namespace gm
