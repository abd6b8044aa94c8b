// Groth16 setup on the device (g16_setup.hip): the fixed-base batch scalar
// multiplication behind gnark's Setup (curve.BatchScalarMultiplicationG1/G2,
// backend/groth16/bn254/setup.go:239-275, 318-330), the block-wise batch inversion
// it normalises its sums with, and the scalar side of Setup over a resident R1CS.
#pragma once
#include "curves.hpp"
#include "runtime.hpp"

namespace gm {

// window bounds of the fixed-base table (gm_set_fixed_base_window)
constexpr int FIXED_BASE_C_MIN = 2, FIXED_BASE_C_MAX = 16;

// Window width c for n scalars of `bits` bits: the context's override, or the
// cost model's minimum (g16_setup.hip, "Window model").
int fixed_base_window(const gm_ctx* ctx, size_t n, int bits);

// out_dev[i] = [k_i] base as gnark affine points, k_i Montgomery fr.Elements on the
// device; the contract of gm_batch_mul_base.  Drains the stream before it returns.
template <class C, bool G2>
int batch_mul_fixed_device(gm_ctx* ctx, const void* base_affine_host, const void* scalars_dev, size_t n,
                           void* out_dev);

// The scalar side of Setup and the points.  sizes != NULL: the counts nbA, nbB, nbK
// alone (gm_g16_setup_sizes).  Else the arrays go to the non-NULL members of `out`
// (gm_g16_setup; out may be NULL) and, with pk_out, become the resident key
// (gm_g16_pk_setup).  Judges the inputs on the host first; `entry` names the caller
// in refusals.
int g16_setup_run(gm_ctx* ctx, const char* entry, const gm_r1cs* r, const gm_g16_setup_in* in,
                  const gm_g16_setup_out* out, size_t* sizes, unsigned flags, gm_g16_pk** pk_out);

// ---- block-wise batch inversion (Montgomery's trick) --------------------------------
// A block of TPB lanes holds one non-zero element each.  block_product leaves the
// product tree of the block in `tree` (2 TPB elements of LDS: node 1 is the root,
// node TPB + t lane t's element) and returns the root; block_inverse, given the
// root's inverse, walks the tree down and returns 1 / d of the calling lane:
// inv(left child) = inv(parent) * right child, and the mirror image.  3 TPB
// products per block for TPB inverses, plus the one inversion of the root that
// another launch does at full lane occupancy.  Every lane of the block must call
// (a lane without an element passes one).  Templated on the field: Fe<Fp> and
// Fe2 coordinates here, Fe<Fr> scalars alike.
template <class F, unsigned TPB>
GM_DEV F block_product(const F& d, F* __restrict__ tree) {
  const unsigned t = threadIdx.x;
  tree[TPB + t] = d;
  __syncthreads();
  for (unsigned s = TPB / 2; s >= 1; s >>= 1) {
    if (t < s) tree[s + t] = fe_mul(tree[2 * (s + t)], tree[2 * (s + t) + 1]);
    __syncthreads();
  }
  return tree[1];
}

template <class F, unsigned TPB>
GM_DEV F block_inverse(const F& d, const F& root_inv, F* __restrict__ tree) {
  const unsigned t = threadIdx.x;
  block_product<F, TPB>(d, tree);
  if (t == 0) tree[1] = root_inv;
  __syncthreads();
  for (unsigned s = 1; s < TPB; s <<= 1) {
    if (t < s) {
      const unsigned k = s + t;
      const F inv = tree[k], l = tree[2 * k], r = tree[2 * k + 1];
      tree[2 * k] = fe_mul(inv, r);
      tree[2 * k + 1] = fe_mul(inv, l);
    }
    __syncthreads();
  }
  return tree[TPB + t];
}

}  // namespace gm
