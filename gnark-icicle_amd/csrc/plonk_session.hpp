// One PLONK proof on a resident key (see plonk_session.hip): the prover's five
// rounds as a state machine over buffers the session owns.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/gnark_mi355x.h"
#include "plonk_pk.hpp"

struct gm_plonk_session {
  gm_ctx* ctx = nullptr;
  gm_plonk_pk* pk = nullptr;
  int state = 0;  // the last round that ran; bsb22 calls belong to state 0
  std::vector<char> bsb_done;
  void* buf = nullptr;  // one allocation (or the key's parked one); the members below point into it
  size_t buf_bytes = 0;
  void *l_lag = nullptr, *r_lag = nullptr, *o_lag = nullptr;  // Lagrange regular, n each
  void *l = nullptr, *r = nullptr, *o = nullptr, *qk = nullptr;  // canonical, n each (qk completed)
  void *z_lag = nullptr, *z = nullptr;  // n each
  void* h = nullptr;  // 4n; before round 3 also staging of n elements
  void* lin = nullptr;  // n + 3
  void *l_bl = nullptr, *r_bl = nullptr, *o_bl = nullptr, *z_bl = nullptr;  // n + 2 each, z n + 3
  std::vector<void*> pi2_lag, pi2;  // nb_bsb of n each
  // the proof's host scalars (gnark words), kept from the round that brought them
  uint64_t bl[2][4], br[2][4], bo[2][4], bz[3][4], h_rand[2][4];
  bool has_h_rand = false;
  uint64_t alpha[4], beta[4], gamma[4], zeta[4];
};

namespace gm {
int plonk_session_begin(gm_ctx* ctx, gm_plonk_pk* pk, gm_plonk_session** out);
int plonk_session_bsb22(gm_plonk_session* s, size_t j, const void* committed_host, void* digest_affine);
int plonk_session_round1(gm_plonk_session* s, const gm_plonk_round1_in* in, void* lro_affine);
int plonk_session_bsb22_sparse(gm_plonk_session* s, size_t j, const uint32_t* rows, const void* values, size_t count,
                               void* digest_affine);
int plonk_session_round1_witness(gm_plonk_session* s, const gm_plonk_wires* w, const gm_plonk_round1_witness_in* in,
                                 void* lro_affine);
int plonk_session_round2(gm_plonk_session* s, const void* beta, const void* gamma, void* z_affine);
int plonk_session_round3(gm_plonk_session* s, const void* alpha, void* h_affine);
int plonk_session_round4(gm_plonk_session* s, const void* zeta, void* lin_affine, void* claimed,
                         void* z_shifted_value, void* z_shifted_h_affine);
int plonk_session_round5(gm_plonk_session* s, const void* kzg_gamma, void* batch_h_affine);
void plonk_session_release(gm_plonk_session* s);
}  // namespace gm
