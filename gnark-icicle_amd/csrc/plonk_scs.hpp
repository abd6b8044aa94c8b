// A PLONK constraint system resident on the device (see plonk_scs.hip): gnark's
// SparseR1C records split into columns, from which the wire tables, the
// selectors, the proving key and a check of a witness are made on the device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/gnark_mi355x.h"
#include "plonk_wires.hpp"

struct gm_plonk_scs {
  gm_ctx* ctx = nullptr;
  int curve = 0;
  size_t n = 0, nb_public = 0, nb_constraints = 0, nb_wires = 0, ncoeffs = 0, nb_bsb = 0;
  // One allocation, every part 256-byte aligned:
  //   tab        xa | xb | xc, n ids each: gm_plonk_wires' layout, which `wires` points at
  //   cid        five columns of `stride` coefficient ids in the selectors' order
  //              QL QR QM QO QK, entry i of a column belongs to constraint i
  //   coeffs     ncoeffs elements, gnark form: the CoeffTable
  //   committed  the committed rows of all gates, gate after gate, offset by
  //              nb_public, ascending inside a gate (the selector kernel searches them)
  //   commitment one byte per constraint: SparseR1C.Commitment
  char* buf = nullptr;
  size_t bytes = 0, stride = 0;
  uint32_t* cid = nullptr;
  void* coeffs = nullptr;
  uint32_t* committed = nullptr;
  uint8_t* commitment = nullptr;
  std::vector<size_t> committed_off;   // nb_bsb + 1 offsets into `committed`
  std::vector<size_t> commitment_row;  // nb_bsb rows of Qk: nb_public + CommitmentIndex
  gm_plonk_wires wires;                // borrowed view of `tab`; on no context's list
};

namespace gm {
// column source of plonk_pk_finish (plonk_pk.hpp): GM_SCS_* -> n elements at out_dev
int plonk_scs_column(gm_ctx* ctx, const void* scs, unsigned which, void* out_dev);
// Every argument is checked on the host before the first device call.
int plonk_scs_upload(gm_ctx* ctx, int curve, const gm_plonk_scs_host* h, gm_plonk_scs** out);
// frees the object and takes it off its context's list
void plonk_scs_release(gm_plonk_scs* s);
// selector `which` (checked by the caller) as n elements, Lagrange regular, queued
// on ctx->stream
int plonk_scs_selector_device(gm_ctx* ctx, const gm_plonk_scs* s, unsigned which, void* out_dev);
int plonk_scs_selector(gm_ctx* ctx, const gm_plonk_scs* s, unsigned which, void* out_dev);
// The gate equation on every constraint row whose Commitment is NOT, witness on
// the device (nb_wires elements); result_dev: two u64, {failures, smallest failing
// constraint}, initialised here to {0, ~0}.  Queued on ctx->stream.
int plonk_scs_check_device(gm_ctx* ctx, const gm_plonk_scs* s, const void* witness_dev,
                           unsigned long long* result_dev);
int plonk_scs_check(gm_ctx* ctx, const gm_plonk_scs* s, const void* witness_host, size_t* nb_unsatisfied,
                    size_t* first_unsatisfied);
}  // namespace gm
