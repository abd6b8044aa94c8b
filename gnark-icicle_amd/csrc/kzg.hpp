// KZG opening polynomial work on the device (see kzg.hip): evaluation at a
// point, division by X - z, and the gamma-fold of a batch opening.
#pragma once
#include <cstddef>
#include "curves.hpp"

struct gm_ctx;

namespace gm {
// values_host[i] = f_i(z) for k polynomials resident on the device (lens[i] = 0 -> 0)
template <class C>
int poly_eval_device(gm_ctx* ctx, const void* const* polys, const size_t* lens, size_t k, const void* z_host,
                     void* values_host);
// q[0..m-2] = (f - f(z)) / (X - z), *value_host = f(z); m >= 1, q must not overlap f
template <class C>
int poly_div_linear_device(gm_ctx* ctx, const void* f, size_t m, const void* z_host, void* q, void* value_host);
// out[0..max(lens)-1] = sum_i gamma^i f_i
template <class C>
int poly_fold_device(gm_ctx* ctx, const void* const* polys, const size_t* lens, size_t k, const void* gamma_host,
                     void* out);
}  // namespace gm
