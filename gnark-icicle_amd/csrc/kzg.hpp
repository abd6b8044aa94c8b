// KZG opening polynomial work on the device (see kzg.hip): evaluation at a
// point, division by X - z, and the gamma-fold of a batch opening.
#pragma once
#include <cstddef>
#include <cstring>
#include "curves.hpp"

struct gm_ctx;

namespace gm {
// gnark-form host element -> internal form in gnark's word layout: x 2^(29 N) =
// (x 2^(32 NG)) 2^(29 N - 32 NG), a product with a small power of two
template <class C>
FeG<typename C::Fr> to_internal_words(const host::F<typename C::HFr>& x) {
  using Fr = typename C::Fr;
  static const host::F<typename C::HFr> kin = host::from_u64<typename C::HFr>(1ull << (RADIX * Fr::N - 32 * Fr::NG));
  const host::F<typename C::HFr> y = x * kin;
  FeG<Fr> r;
  static_assert(sizeof(r.w) == sizeof(y.v), "gnark layout");
  memcpy(r.w, y.v, sizeof(r.w));
  return r;
}

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
