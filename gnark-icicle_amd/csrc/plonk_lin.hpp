// PLONK linearized polynomial on the device (see plonk_lin.hip): resident
// selectors, permutation values, Z and h in, r(X) and the blinded wires out.
#pragma once
#include <cstddef>
#include "../../include/gnark_mi355x.h"
#include "curves.hpp"

namespace gm {
// geometry of the combination pass: a lane owns one coefficient, a block
// LIN_BLOCK consecutive ones; ceil((n + 3) / LIN_BLOCK) blocks: the grid is
// not capped, so no lane loops
constexpr int LIN_TPB_LOG = 8;
constexpr int LIN_BLOCK = 1 << LIN_TPB_LOG;  // coefficients per block (256)

// out->lin[0..n+3) = the linearized polynomial, out->evals = the six (+ nb_bsb)
// evaluations, the blinded copies where asked for (include/gnark_mi355x.h,
// gm_plonk_linearize).  Checks every argument on the host before the first
// launch.  The evaluations synchronise; the combination is queued on ctx->stream
// and the caller synchronises.
template <class C>
int plonk_linearize_device(gm_ctx* ctx, const gm_plonk_linearize_in* in, const gm_plonk_linearize_out* out);
}  // namespace gm
