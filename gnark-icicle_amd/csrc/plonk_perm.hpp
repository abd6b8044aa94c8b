// PLONK permutation polynomial Z on the device (see plonk_perm.hip): resident
// wires and permutation values in, Z in Lagrange form out.
#pragma once
#include <cstddef>
#include "../../include/gnark_mi355x.h"
#include "curves.hpp"

namespace gm {
// geometry of the scan: a chunk is PERM_TPB * PERM_E consecutive rows, a thread
// owns a run of PERM_E of them; the carry scan takes PERM_CT chunks per tile
constexpr int PERM_TPB_LOG = 7;
constexpr int PERM_TPB = 1 << PERM_TPB_LOG;
constexpr int PERM_E_LOG = 2;
constexpr int PERM_E = 1 << PERM_E_LOG;
constexpr int PERM_C = PERM_TPB * PERM_E;  // rows per chunk (512)
constexpr int PERM_CT_LOG = 6;
constexpr int PERM_CT = 1 << PERM_CT_LOG;  // chunks per tile of the carry scan (64)

// z_lagrange[0..n) = the copy-constraint accumulator (include/gnark_mi355x.h,
// gm_plonk_perm_z), Lagrange regular.  Checks every argument on the host before
// the first launch.  Queues on ctx->stream; the caller synchronises.
template <class C>
int plonk_perm_z_device(gm_ctx* ctx, const gm_plonk_perm_in* in, void* z_lagrange, void* z_canonical);
}  // namespace gm
