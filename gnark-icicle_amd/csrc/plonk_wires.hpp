// The wire tables of a PLONK circuit resident on the device (see plonk_wires.hip):
// per row the ids of its three wires, from which l, r, o are a gather of the
// solver's values.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/gnark_mi355x.h"

struct gm_plonk_wires {
  gm_ctx* ctx = nullptr;
  size_t n = 0, nb_wires = 0;
  uint32_t* tab = nullptr;  // one allocation: xa, xb, xc, n ids each, every id < nb_wires
  // the tables lie inside a gm_plonk_scs (plonk_scs.hpp), which frees them:
  // gm_plonk_wires_free refuses the object, and it is on no context's list
  bool borrowed = false;
};

namespace gm {
// Every argument is checked on the host before the first device call.
int plonk_wires_upload(gm_ctx* ctx, size_t n, size_t nb_wires, const uint32_t* xa, const uint32_t* xb,
                       const uint32_t* xc, gm_plonk_wires** out);
// frees the tables and takes the object off its context's list
void plonk_wires_release(gm_plonk_wires* w);
// l[i] = witness[xa[i]], r[i] = witness[xb[i]], o[i] = witness[xc[i]], queued on
// ctx->stream; the caller has checked that no output overlaps the witness
int plonk_gather_lro_device(gm_ctx* ctx, const gm_plonk_wires* w, const void* witness, void* l, void* r, void* o);
// dst[rows[i]] = values[i] for i < count (32-byte elements, all three on the
// device), queued on ctx->stream; the caller has checked that the rows are
// distinct and inside dst
int plonk_scatter_rows_device(gm_ctx* ctx, void* dst, const uint32_t* rows, const void* values, size_t count);
}  // namespace gm
