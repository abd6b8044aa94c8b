// PLONK quotient on the device (see plonk.hip): resident polynomials in, h out.
#pragma once
#include <cstddef>
#include "../../include/gnark_mi355x.h"
#include "curves.hpp"

namespace gm {
// h_dev[0..4n) = the polynomial of degree < 4n that is T / Z_H on g <w_4n>
// (include/gnark_mi355x.h, gm_plonk_quotient).  Queues on ctx->stream; the caller
// synchronises.
template <class C>
int plonk_quotient_device(gm_ctx* ctx, const gm_plonk_quotient_in* in, void* h_dev);
}  // namespace gm
