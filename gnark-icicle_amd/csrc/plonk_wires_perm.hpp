// gnark's trace.S from the resident wire tables (see plonk_wires_perm.hip): a
// stable radix sort of the 3n positions by wire id, then every position linked
// to its predecessor in its wire's run.
#pragma once
#include <cstddef>
#include <cstdint>
#include "plonk_wires.hpp"
#include "runtime.hpp"

namespace gm {
// positions are 32-bit: 3 * 2^30 < 2^32
constexpr size_t WIRES_PERM_MAX_N = (size_t)1 << 30;
// Queues the sort and the link on ctx->stream and does not wait.  Scratch comes
// from `arena` (the caller's scope, which must outlive the queued work): two
// buffers of 3n u32 positions (24n bytes), two more for the keys carried beside
// them, and about 1.5n bytes of counters; nothing is sized by nb_wires and nothing is
// expected to be zero.  out64 (device, 3n int64, may be NULL) receives the permutation in
// gnark's element type.  out32 (may be NULL) receives a pointer to the permutation
// as 3n u32 inside the arena.  The tables are only read.
int plonk_wires_perm_queue(gm_ctx* ctx, Arena& arena, const gm_plonk_wires* w, int64_t* out64,
                           const uint32_t** out32);
// the stage call behind gm_plonk_wires_permutation: returns with the stream drained
int plonk_wires_permutation(gm_ctx* ctx, const gm_plonk_wires* w, int64_t* perm_dev);
}  // namespace gm
