// One PLONK proof on a resident key -- the five rounds of gnark's prover
// (backend/plonk/bls12-377/prove.go) as calls on buffers that stay on the device
// from one round to the next.  Per proof the solver's L, R, O and the public
// inputs (or, with resident wire tables, the witness they are gathered from),
// the blinding scalars and the challenges go in; digests, claimed values and
// opening proofs come out.  The Fiat-Shamir transcript is the caller's.
//
// The stages are the library's own device functions (plonk_perm_z_device,
// plonk_quotient_device, plonk_linearize_device, the kzg.hip polynomial work, the
// MSM, the gather and scatter of plonk_wires.hip): this file holds no kernel.
// What it adds is the data flow between them:
//   * l, r, o and the BSB22 polynomials are kept in both bases, Qk is completed
//     from the key's Lagrange Qk and taken to canonical form;
//   * wires and Z are committed where they lie, as Lagrange values over the
//     Lagrange SRS, and the blinding P~ = P + (X^n - 1) b enters the digest as
//     sum_k b_k (G_n+k - G_k), host scalar multiplications on six points of the
//     canonical SRS that the key copied at upload;
//   * the StatisticalZK edits of the quotient shards enter their digests the same
//     way (rho X^m -> rho G_m, -rho at [0] -> -rho G_0), so h stays as
//     gm_plonk_linearize reads it: unedited, with h_rand beside it;
//   * round 3 hands the key's coset cache to the quotient.
// Every digest is a sum of group elements converted to affine once, so its bytes
// are those of the commit of the edited coefficient list.
#include <algorithm>
#include <cstring>

#include "curves.hpp"
#include "kzg.hpp"
#include "msm.hpp"
#include "ntt.hpp"
#include "plonk.hpp"
#include "plonk_lin.hpp"
#include "plonk_perm.hpp"
#include "plonk_session.hpp"
#include "plonk_wires.hpp"
#include "runtime.hpp"

namespace gm {

// The buffer goes to the key for the next session on it (gm_plonk_pk::spare_buf),
// unless the key already holds one.
void plonk_session_release(gm_plonk_session* s) {
  if (!s) return;
  if (s->buf) {
    gm_plonk_pk* pk = s->pk;
    if (!pk->spare_buf) {
      pk->spare_buf = s->buf;
      pk->spare_bytes = s->buf_bytes;
      s->ctx->plonk_spare_keys.push_back(pk);
    } else {
      hipSetDevice(s->ctx->device);
      hipFree(s->buf);
    }
  }
  delete s;
}

namespace {

template <class C>
struct G1 {
  using HP = typename GroupSel<C, false>::HF;
  using Jac = host::Jac<HP>;
  using Aff = host::Aff<HP>;
  using HFr = host::F<typename C::HFr>;
};

// [k] (+-E_idx), E = the key's six canonical SRS points, k one gnark element
template <class C>
typename G1<C>::Jac edge_mul(const gm_plonk_pk* pk, int idx, const uint64_t* k_gnark, bool neg) {
  typename G1<C>::Aff a;
  static_assert(sizeof(a) == 2 * sizeof(typename G1<C>::HP), "gnark affine layout");
  memcpy(&a, &pk->edge[idx * sizeof(a)], sizeof(a));
  if (neg && !a.is_inf()) a.y = -a.y;
  typename G1<C>::HFr k;
  memcpy(k.v, k_gnark, sizeof(k.v));
  k = host::from_mont(k);
  return host::jmul(host::to_jac(a), k.v, 4);
}

// the digest's share of the blinding (X^n - 1) b, b of nc coefficients
template <class C>
typename G1<C>::Jac blind_term(const gm_plonk_pk* pk, const uint64_t (*b)[4], int nc) {
  typename G1<C>::Jac acc = G1<C>::Jac::inf();
  for (int k = 0; k < nc; k++) {
    acc = host::jadd(acc, edge_mul<C>(pk, 3 + k, b[k], false));
    acc = host::jadd(acc, edge_mul<C>(pk, k, b[k], true));
  }
  return acc;
}

template <class C>
void store_affine(const typename G1<C>::Jac& j, void* out) {
  const typename G1<C>::Aff a = host::to_aff(j);
  memcpy(out, &a, sizeof(a));
}

// Lagrange regular -> canonical regular: reversal, then the inverse DIT (as Z in
// plonk_perm_z_device)
template <class C>
int canonical_from(gm_ctx* ctx, void* dst, const void* lag, size_t n) {
  if (int rc = bitrev_copy_device<C>(ctx, dst, lag, n)) return rc;
  return ntt_device<C>(ctx, dst, n, true, true, false);
}

// commit of m resident scalars over a prepared SRS, as a host Jacobian
template <class C>
int commit(gm_ctx* ctx, const void* scalars, const void* srs, size_t m, typename G1<C>::Jac* out) {
  typename G1<C>::HP j[3];
  if (int rc = msm_device<C, false>(ctx, scalars, srs, m, j, true)) return rc;
  *out = {j[0], j[1], j[2]};
  return GM_OK;
}

// three commits in flight (the slots of gm_msm_async); every handle is waited for
template <class C>
int commit3(gm_ctx* ctx, int curve, const void* const* scalars, const void* srs, size_t m,
            typename G1<C>::Jac* out) {
  gm_msm_pending* pend[3] = {};
  int rc = GM_OK;
  for (int i = 0; i < 3 && !rc; i++) rc = msm_async_queue(ctx, curve, 0, scalars[i], srs, m, true, &pend[i]);
  for (int i = 0; i < 3; i++) {
    if (!pend[i]) continue;
    typename G1<C>::HP j[3];
    const int r = gm_msm_wait(pend[i], j, nullptr);
    if (r && !rc) rc = r;
    out[i] = {j[0], j[1], j[2]};
  }
  return rc;
}

int refuse(const char* msg) {
  set_error(std::string("plonk session: ") + msg);
  return GM_ERR_INVALID;
}

// every stage function queues on ctx->stream with scratch from the workspace:
// nothing queued may outlive the call's workspace, also after a failure.  A
// round that takes workspace of its own declares its Arena BEFORE the drain,
// so that the drain (destroyed first) waits while the workspace is still held.
struct StreamDrain {
  gm_ctx* ctx;
  ~StreamDrain() {
    hipStreamSynchronize(ctx->stream);
    prof_collect(ctx);
  }
};

// the committed values lie in pi2_lag[j]: their canonical form and their digest
template <class C>
int bsb22_tail(gm_plonk_session* s, size_t j, void* digest) {
  gm_ctx* ctx = s->ctx;
  const gm_plonk_pk* pk = s->pk;
  const size_t n = pk->n;
  int rc;
  if ((rc = canonical_from<C>(ctx, s->pi2[j], s->pi2_lag[j], n))) return rc;
  typename G1<C>::Jac d;
  if ((rc = commit<C>(ctx, s->pi2_lag[j], pk->srs_lagrange, n, &d))) return rc;
  store_affine<C>(d, digest);
  return GM_OK;
}

template <class C>
int bsb22_t(gm_plonk_session* s, size_t j, const void* committed, void* digest) {
  gm_ctx* ctx = s->ctx;
  StreamDrain drain{ctx};
  GM_HIP(hipMemcpyAsync(s->pi2_lag[j], committed, 32 * s->pk->n, hipMemcpyHostToDevice, ctx->stream));
  return bsb22_tail<C>(s, j, digest);
}

// the vector by its nonzero rows: zero-filled on the device, then one scatter of
// the (row, value) pairs (the rows were checked on the host)
template <class C>
int bsb22_sparse_t(gm_plonk_session* s, size_t j, const uint32_t* rows, const void* values, size_t count,
                   void* digest) {
  gm_ctx* ctx = s->ctx;
  Arena arena(ctx);  // before the drain (StreamDrain)
  DevBuf drows, dvals;
  int rc;
  if ((rc = dvals.alloc(arena, 32 * count))) return rc;
  if ((rc = drows.alloc(arena, sizeof(uint32_t) * count))) return rc;
  StreamDrain drain{ctx};
  GM_HIP(hipMemsetAsync(s->pi2_lag[j], 0, 32 * s->pk->n, ctx->stream));
  if (count) {
    GM_HIP(hipMemcpyAsync(dvals.p, values, 32 * count, hipMemcpyHostToDevice, ctx->stream));
    GM_HIP(hipMemcpyAsync(drows.p, rows, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = plonk_scatter_rows_device(ctx, s->pi2_lag[j], drows.as<uint32_t>(), dvals.p, count))) return rc;
  }
  return bsb22_tail<C>(s, j, digest);
}

// Round 1 once l, r, o lie in their Lagrange buffers and Qk's copy in h carries
// the public inputs: the commitment values on their rows, the three commits, the
// canonical forms, the blinding, the scalars kept.  `in` is either input struct
// (they share these members).
template <class C, class In>
int round1_tail(gm_plonk_session* s, const In* in, void* lro_affine) {
  gm_ctx* ctx = s->ctx;
  const gm_plonk_pk* pk = s->pk;
  const size_t n = pk->n, nb = pk->nb_bsb;
  void* const lag[3] = {s->l_lag, s->r_lag, s->o_lag};
  void* const can[3] = {s->l, s->r, s->o};
  for (size_t j = 0; j < nb; j++)
    GM_HIP(hipMemcpyAsync((char*)s->h + 32 * pk->commitment_row[j], (const char*)in->commitment_vals + 32 * j, 32,
                          hipMemcpyHostToDevice, ctx->stream));
  // the three commits start behind the copies and run beside the transforms
  typename G1<C>::Jac d[3];
  gm_msm_pending* pend[3] = {};
  int rc = GM_OK;
  for (int i = 0; i < 3 && !rc; i++)
    rc = msm_async_queue(ctx, pk->curve, 0, lag[i], pk->srs_lagrange, n, true, &pend[i]);
  if (!rc) rc = canonical_from<C>(ctx, s->qk, s->h, n);
  for (int i = 0; i < 3 && !rc; i++) rc = canonical_from<C>(ctx, can[i], lag[i], n);
  // the blinding's share, on the host while the device works
  uint64_t b[3][2][4];
  memcpy(b[0], in->bl, sizeof(b[0]));
  memcpy(b[1], in->br, sizeof(b[1]));
  memcpy(b[2], in->bo, sizeof(b[2]));
  typename G1<C>::Jac bt[3];
  if (!rc)
    for (int i = 0; i < 3; i++) bt[i] = blind_term<C>(pk, b[i], 2);
  for (int i = 0; i < 3; i++) {
    if (!pend[i]) continue;
    typename G1<C>::HP j[3];
    const int r = gm_msm_wait(pend[i], j, nullptr);
    if (r && !rc) rc = r;
    d[i] = {j[0], j[1], j[2]};
  }
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  const size_t pb = sizeof(typename G1<C>::Aff);
  for (int i = 0; i < 3; i++) store_affine<C>(host::jadd(d[i], bt[i]), (char*)lro_affine + pb * i);
  memcpy(s->bl, in->bl, sizeof(s->bl));
  memcpy(s->br, in->br, sizeof(s->br));
  memcpy(s->bo, in->bo, sizeof(s->bo));
  memcpy(s->bz, in->bz, sizeof(s->bz));
  s->has_h_rand = in->h_rand != nullptr;
  if (in->h_rand) memcpy(s->h_rand, in->h_rand, sizeof(s->h_rand));
  return GM_OK;
}

template <class C>
int round1_t(gm_plonk_session* s, const gm_plonk_round1_in* in, void* lro_affine) {
  gm_ctx* ctx = s->ctx;
  const gm_plonk_pk* pk = s->pk;
  const size_t n = pk->n;
  StreamDrain drain{ctx};
  void* const lag[3] = {s->l_lag, s->r_lag, s->o_lag};
  const void* const host[3] = {in->l, in->r, in->o};
  for (int i = 0; i < 3; i++)
    GM_HIP(hipMemcpyAsync(lag[i], host[i], 32 * n, hipMemcpyHostToDevice, ctx->stream));
  // Qk: the key's Lagrange values, the public inputs on the first rows, the
  // commitment values on theirs (prove.go:363-389); completed in h, which is free
  // until round 3
  GM_HIP(hipMemcpyAsync(s->h, pk->lagrange(gm_plonk_pk::LAG_QK), 32 * n, hipMemcpyDeviceToDevice, ctx->stream));
  if (pk->nb_public)
    GM_HIP(hipMemcpyAsync(s->h, in->public_inputs, 32 * pk->nb_public, hipMemcpyHostToDevice, ctx->stream));
  return round1_tail<C>(s, in, lro_affine);
}

// Round 1 from the solver's values: one upload, l, r, o gathered through the
// resident wire tables, Qk's public rows from the witness' first nb_public
// elements (solver.values[:nbPublic] is the public witness)
template <class C>
int round1_witness_t(gm_plonk_session* s, const gm_plonk_wires* w, const gm_plonk_round1_witness_in* in,
                     void* lro_affine) {
  gm_ctx* ctx = s->ctx;
  const gm_plonk_pk* pk = s->pk;
  const size_t n = pk->n;
  Arena arena(ctx);  // before the drain (StreamDrain)
  DevBuf wit;
  int rc;
  if ((rc = wit.alloc(arena, 32 * w->nb_wires))) return rc;
  StreamDrain drain{ctx};
  GM_HIP(hipMemcpyAsync(wit.p, in->witness, 32 * w->nb_wires, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = plonk_gather_lro_device(ctx, w, wit.p, s->l_lag, s->r_lag, s->o_lag))) return rc;
  GM_HIP(hipMemcpyAsync(s->h, pk->lagrange(gm_plonk_pk::LAG_QK), 32 * n, hipMemcpyDeviceToDevice, ctx->stream));
  if (pk->nb_public)
    GM_HIP(hipMemcpyAsync(s->h, wit.p, 32 * pk->nb_public, hipMemcpyDeviceToDevice, ctx->stream));
  return round1_tail<C>(s, in, lro_affine);
}

template <class C>
int round2_t(gm_plonk_session* s, const void* beta, const void* gamma, void* z_affine) {
  gm_ctx* ctx = s->ctx;
  const gm_plonk_pk* pk = s->pk;
  StreamDrain drain{ctx};
  gm_plonk_perm_in in;
  in.n = pk->n;
  in.l = s->l_lag;
  in.r = s->r_lag;
  in.o = s->o_lag;
  in.s1 = pk->lagrange(gm_plonk_pk::LAG_S1);
  in.s2 = pk->lagrange(gm_plonk_pk::LAG_S2);
  in.s3 = pk->lagrange(gm_plonk_pk::LAG_S3);
  in.beta = beta;
  in.gamma = gamma;
  int rc;
  if ((rc = plonk_perm_z_device<C>(ctx, &in, s->z_lag, s->z))) return rc;
  typename G1<C>::Jac d;
  if ((rc = commit<C>(ctx, s->z_lag, pk->srs_lagrange, pk->n, &d))) return rc;
  store_affine<C>(host::jadd(d, blind_term<C>(pk, s->bz, 3)), z_affine);
  memcpy(s->beta, beta, 32);
  memcpy(s->gamma, gamma, 32);
  return GM_OK;
}

// the members the quotient and the linearization share (the first twenty of both structs)
template <class In>
void fill_stage_in(const gm_plonk_session* s, In* in, std::vector<const void*>* qcp, std::vector<const void*>* pi2) {
  const gm_plonk_pk* pk = s->pk;
  in->n = pk->n;
  in->ql = pk->canonical(gm_plonk_pk::QL);
  in->qr = pk->canonical(gm_plonk_pk::QR);
  in->qm = pk->canonical(gm_plonk_pk::QM);
  in->qo = pk->canonical(gm_plonk_pk::QO);
  in->qk = s->qk;
  in->s1 = pk->canonical(gm_plonk_pk::S1);
  in->s2 = pk->canonical(gm_plonk_pk::S2);
  in->s3 = pk->canonical(gm_plonk_pk::S3);
  in->l = s->l;
  in->r = s->r;
  in->o = s->o;
  in->z = s->z;
  in->nb_bsb = pk->nb_bsb;
  for (size_t j = 0; j < pk->nb_bsb; j++) {
    qcp->push_back(pk->qcp(j));
    pi2->push_back(s->pi2[j]);
  }
  in->qcp = pk->nb_bsb ? qcp->data() : nullptr;
  in->pi2 = pk->nb_bsb ? pi2->data() : nullptr;
  in->bl = s->bl;
  in->br = s->br;
  in->bo = s->bo;
  in->bz = s->bz;
}

template <class C>
int round3_t(gm_plonk_session* s, const void* alpha, void* h_affine) {
  gm_ctx* ctx = s->ctx;
  const gm_plonk_pk* pk = s->pk;
  const size_t n = pk->n, m = n + 2;
  StreamDrain drain{ctx};
  gm_plonk_quotient_in in;
  std::vector<const void*> qcp, pi2;
  fill_stage_in(s, &in, &qcp, &pi2);
  in.alpha = alpha;
  in.beta = s->beta;
  in.gamma = s->gamma;
  const PlonkCosetCache cache = pk->coset_cache();
  int rc;
  {
    // device-event bracket of the quotient alone, one name per kernel variant
    ProfScope ps(ctx, pk->cache ? "plonk_session_quotient_cached" : "plonk_session_quotient");
    rc = plonk_quotient_device<C>(ctx, &in, s->h, pk->cache ? &cache : nullptr);
  }
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  // h1, h2, h3 where they lie (prove.go:1154-1173)
  const void* shard[3] = {s->h, (const char*)s->h + 32 * m, (const char*)s->h + 32 * 2 * m};
  typename G1<C>::Jac d[3];
  if ((rc = commit3<C>(ctx, pk->curve, shard, pk->srs_canonical, m, d))) return rc;
  if (s->has_h_rand) {
    // h1 || rho0;  h2 with [0] -= rho0, then rho1;  h3 with [0] -= rho1 (prove.go:619-654)
    d[0] = host::jadd(d[0], edge_mul<C>(pk, 5, s->h_rand[0], false));
    d[1] = host::jadd(d[1], edge_mul<C>(pk, 0, s->h_rand[0], true));
    d[1] = host::jadd(d[1], edge_mul<C>(pk, 5, s->h_rand[1], false));
    d[2] = host::jadd(d[2], edge_mul<C>(pk, 0, s->h_rand[1], true));
  }
  const size_t pb = sizeof(typename G1<C>::Aff);
  for (int i = 0; i < 3; i++) store_affine<C>(d[i], (char*)h_affine + pb * i);
  memcpy(s->alpha, alpha, 32);
  return GM_OK;
}

template <class C>
int round4_t(gm_plonk_session* s, const void* zeta, void* lin_affine, void* claimed, void* z_shifted_value,
             void* z_shifted_h_affine) {
  using HFr = typename G1<C>::HFr;
  gm_ctx* ctx = s->ctx;
  const gm_plonk_pk* pk = s->pk;
  const size_t n = pk->n, nb = pk->nb_bsb;
  Arena arena(ctx);  // before the drain (StreamDrain)
  DevBuf q;          // the quotient of the opening of Z~
  DevBuf key_qk;     // GM_PLONK_PK_LIN_KEY_QK: the key's Qk in the canonical basis
  int rc;
  if ((rc = q.alloc(arena, 32 * (n + 2)))) return rc;
  if (pk->lin_key_qk && (rc = key_qk.alloc(arena, 32 * n))) return rc;
  StreamDrain drain{ctx};
  gm_plonk_linearize_in in;
  std::vector<const void*> qcp, pi2;
  fill_stage_in(s, &in, &qcp, &pi2);
  if (pk->lin_key_qk) {
    // gnark's innerComputeLinearizedPoly reads trace.Qk, not the completed copy the quotient took
    // (prove.go:1301-1337): the public inputs reach the verifier through PI(zeta) alone
    if ((rc = canonical_from<C>(ctx, key_qk.p, pk->lagrange(gm_plonk_pk::LAG_QK), n))) return rc;
    in.qk = key_qk.p;
  }
  in.h = s->h;
  in.h_rand = s->has_h_rand ? s->h_rand : nullptr;
  in.alpha = s->alpha;
  in.beta = s->beta;
  in.gamma = s->gamma;
  in.zeta = zeta;
  std::vector<HFr> ev(6 + nb);
  gm_plonk_linearize_out out;
  out.lin = s->lin;
  out.l_blinded = s->l_bl;
  out.r_blinded = s->r_bl;
  out.o_blinded = s->o_bl;
  out.z_blinded = s->z_bl;
  out.evals = ev.data();
  if ((rc = plonk_linearize_device<C>(ctx, &in, &out))) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  typename G1<C>::Jac d;
  if ((rc = commit<C>(ctx, s->lin, pk->srs_canonical, n + 3, &d))) return rc;
  // lin(zeta): the first of the claimed values (polysToOpen, prove.go:736-744)
  HFr lin_zeta;
  const void* lp = s->lin;
  const size_t ll = n + 3;
  if ((rc = poly_eval_device<C>(ctx, &lp, &ll, 1, zeta, lin_zeta.v))) return rc;
  // kzg.Open of Z~ at w zeta (prove.go:600-617); w as plonk_linearize_device has it
  HFr w, z;
  memcpy(z.v, zeta, sizeof(z.v));
  if ((rc = coset4_shift<C>(n / 4, 1, w.v))) return rc;
  w = w * host::finv(host::from_u64<typename C::HFr>(C::COSET_GEN));
  const HFr wzeta = w * z;
  typename G1<C>::Jac hq;
  HFr zu;
  if ((rc = poly_div_linear_device<C>(ctx, s->z_bl, n + 3, wzeta.v, q.p, zu.v))) return rc;
  if ((rc = commit<C>(ctx, q.p, pk->srs_canonical, n + 2, &hq))) return rc;
  store_affine<C>(d, lin_affine);
  store_affine<C>(hq, z_shifted_h_affine);
  // lin, l~, r~, o~, s1, s2, qcp_j: the evaluations' order but for z~(w zeta)
  memcpy(claimed, lin_zeta.v, 32);
  memcpy((char*)claimed + 32, ev.data(), 32 * 5);
  if (nb) memcpy((char*)claimed + 32 * 6, ev.data() + 6, 32 * nb);
  memcpy(z_shifted_value, ev[5].v, 32);
  memcpy(s->zeta, zeta, 32);
  return GM_OK;
}

template <class C>
int round5_t(gm_plonk_session* s, const void* kzg_gamma, void* batch_h_affine) {
  using HFr = typename G1<C>::HFr;
  gm_ctx* ctx = s->ctx;
  const gm_plonk_pk* pk = s->pk;
  const size_t n = pk->n, nb = pk->nb_bsb;
  Arena arena(ctx);  // before the drain (StreamDrain)
  DevBuf folded, q;
  int rc;
  if ((rc = folded.alloc(arena, 32 * (n + 3)))) return rc;
  if ((rc = q.alloc(arena, 32 * (n + 2)))) return rc;
  StreamDrain drain{ctx};
  // kzg.BatchOpenSinglePoint over polysToOpen at zeta (prove.go:726-767)
  std::vector<const void*> polys = {s->lin,  s->l_bl, s->r_bl, s->o_bl, pk->canonical(gm_plonk_pk::S1),
                                    pk->canonical(gm_plonk_pk::S2)};
  std::vector<size_t> lens = {n + 3, n + 2, n + 2, n + 2, n, n};
  for (size_t j = 0; j < nb; j++) {
    polys.push_back(pk->qcp(j));
    lens.push_back(n);
  }
  if ((rc = poly_fold_device<C>(ctx, polys.data(), lens.data(), polys.size(), kzg_gamma, folded.p))) return rc;
  HFr value;
  if ((rc = poly_div_linear_device<C>(ctx, folded.p, n + 3, s->zeta, q.p, value.v))) return rc;
  typename G1<C>::Jac d;
  if ((rc = commit<C>(ctx, q.p, pk->srs_canonical, n + 2, &d))) return rc;
  store_affine<C>(d, batch_h_affine);
  return GM_OK;
}

}  // namespace

#define GM_PLONK_DISPATCH(s, call) ((s)->pk->curve == GM_BN254 ? call<CurveBN254> : call<CurveBLS12377>)

int plonk_session_begin(gm_ctx* ctx, gm_plonk_pk* pk, gm_plonk_session** out) {
  if (pk->ctx != ctx) return refuse("the key was uploaded on another context");
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const size_t n = pk->n, nb = pk->nb_bsb;
  // sizes in elements, each region rounded to 8 elements (256 bytes)
  auto up = [](size_t e) { return (e + 7) & ~size_t(7); };
  const size_t sizes[] = {n, n, n, n, n, n, n, n, n, 4 * n, up(n + 3), up(n + 2), up(n + 2), up(n + 2), up(n + 3)};
  size_t total = 2 * nb * n;
  for (size_t e : sizes) total += e;
  gm_plonk_session* s = new gm_plonk_session;
  s->ctx = ctx;
  s->pk = pk;
  s->buf_bytes = 32 * total;
  if (pk->spare_buf && pk->spare_bytes == s->buf_bytes) {
    // the buffer of the session before (a session's size depends on the key alone)
    s->buf = pk->spare_buf;
    pk->spare_buf = nullptr;
    plonk_spare_release(pk);
  } else {
    const hipError_t e = hipMalloc(&s->buf, s->buf_bytes);
    if (e != hipSuccess) {
      delete s;
      set_error(std::string("plonk session: hipMalloc(") + std::to_string(32 * total) + "): " + hipGetErrorString(e));
      return GM_ERR_OOM;
    }
  }
  char* p = (char*)s->buf;
  void** const slots[] = {&s->l_lag, &s->r_lag, &s->o_lag, &s->l,    &s->r,    &s->o,    &s->qk,  &s->z_lag,
                          &s->z,     &s->h,     &s->lin,   &s->l_bl, &s->r_bl, &s->o_bl, &s->z_bl};
  for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); k++) {
    *slots[k] = p;
    p += 32 * sizes[k];
  }
  for (size_t j = 0; j < nb; j++) {
    s->pi2_lag.push_back(p);
    s->pi2.push_back(p + 32 * n);
    p += 64 * n;
  }
  s->bsb_done.assign(nb, 0);
  *out = s;
  return GM_OK;
}

int plonk_session_bsb22(gm_plonk_session* s, size_t j, const void* committed_host, void* digest_affine) {
  if (s->state != 0) return refuse("bsb22 belongs before round 1");
  if (j >= s->pk->nb_bsb) return refuse("bsb22: j is not below the key's nb_bsb");
  if (!committed_host || !digest_affine) return refuse("bsb22: the values and the digest must be non-null");
  CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  const int rc = GM_PLONK_DISPATCH(s, bsb22_t)(s, j, committed_host, digest_affine);
  if (!rc) s->bsb_done[j] = 1;
  return rc;
}

int plonk_session_round1(gm_plonk_session* s, const gm_plonk_round1_in* in, void* lro_affine) {
  if (s->state != 0) return refuse("round 1 was already run");
  for (char done : s->bsb_done)
    if (!done) return refuse("round 1 needs the bsb22 call of every commitment first");
  if (!in->l || !in->r || !in->o || !in->bl || !in->br || !in->bo || !in->bz || !lro_affine)
    return refuse("round 1: l, r, o, the blinding scalars and the output must be non-null");
  if (s->pk->nb_public && !in->public_inputs) return refuse("round 1: the public inputs must be non-null");
  if ((s->pk->nb_bsb != 0) != (in->commitment_vals != nullptr))
    return refuse("round 1: commitment_vals must be given exactly when the key has commitments");
  CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  const int rc = GM_PLONK_DISPATCH(s, round1_t)(s, in, lro_affine);
  if (!rc) s->state = 1;
  return rc;
}

int plonk_session_bsb22_sparse(gm_plonk_session* s, size_t j, const uint32_t* rows, const void* values, size_t count,
                               void* digest_affine) {
  if (s->state != 0) return refuse("bsb22 belongs before round 1");
  const size_t n = s->pk->n;
  if (j >= s->pk->nb_bsb) return refuse("bsb22: j is not below the key's nb_bsb");
  if (!digest_affine || (count && (!rows || !values)))
    return refuse("bsb22 sparse: the rows, the values and the digest must be non-null");
  if (count > n) return refuse("bsb22 sparse: more rows than the domain has");
  std::vector<uint32_t> sorted(rows, rows + count);
  std::sort(sorted.begin(), sorted.end());
  if (count && sorted.back() >= n) {
    set_error("plonk session: bsb22 sparse: row " + std::to_string(sorted.back()) + " lies outside the domain");
    return GM_ERR_INVALID;
  }
  const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
  if (dup != sorted.end()) {
    set_error("plonk session: bsb22 sparse: row " + std::to_string(*dup) + " is given twice");
    return GM_ERR_INVALID;
  }
  CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  const int rc = GM_PLONK_DISPATCH(s, bsb22_sparse_t)(s, j, rows, values, count, digest_affine);
  if (!rc) s->bsb_done[j] = 1;
  return rc;
}

int plonk_session_round1_witness(gm_plonk_session* s, const gm_plonk_wires* w, const gm_plonk_round1_witness_in* in,
                                 void* lro_affine) {
  if (s->state != 0) return refuse("round 1 was already run");
  for (char done : s->bsb_done)
    if (!done) return refuse("round 1 needs the bsb22 call of every commitment first");
  if (!in->witness || !in->bl || !in->br || !in->bo || !in->bz || !lro_affine)
    return refuse("round 1: the witness, the blinding scalars and the output must be non-null");
  if ((s->pk->nb_bsb != 0) != (in->commitment_vals != nullptr))
    return refuse("round 1: commitment_vals must be given exactly when the key has commitments");
  if (w->ctx != s->ctx) return refuse("round 1: the wire tables were uploaded on another context");
  if (w->n != s->pk->n) return refuse("round 1: the wire tables have another n than the key");
  if (w->nb_wires < s->pk->nb_public) return refuse("round 1: fewer wires than the key has public inputs");
  CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  const int rc = GM_PLONK_DISPATCH(s, round1_witness_t)(s, w, in, lro_affine);
  if (!rc) s->state = 1;
  return rc;
}

int plonk_session_round2(gm_plonk_session* s, const void* beta, const void* gamma, void* z_affine) {
  if (s->state != 1) return refuse("round 2 follows round 1");
  if (!beta || !gamma || !z_affine) return refuse("round 2: beta, gamma and the output must be non-null");
  CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  const int rc = GM_PLONK_DISPATCH(s, round2_t)(s, beta, gamma, z_affine);
  if (!rc) s->state = 2;
  return rc;
}

int plonk_session_round3(gm_plonk_session* s, const void* alpha, void* h_affine) {
  if (s->state != 2) return refuse("round 3 follows round 2");
  if (!alpha || !h_affine) return refuse("round 3: alpha and the output must be non-null");
  CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  const int rc = GM_PLONK_DISPATCH(s, round3_t)(s, alpha, h_affine);
  if (!rc) s->state = 3;
  return rc;
}

int plonk_session_round4(gm_plonk_session* s, const void* zeta, void* lin_affine, void* claimed,
                         void* z_shifted_value, void* z_shifted_h_affine) {
  if (s->state != 3) return refuse("round 4 follows round 3");
  if (!zeta || !lin_affine || !claimed || !z_shifted_value || !z_shifted_h_affine)
    return refuse("round 4: zeta and the outputs must be non-null");
  CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  const int rc = GM_PLONK_DISPATCH(s, round4_t)(s, zeta, lin_affine, claimed, z_shifted_value, z_shifted_h_affine);
  if (!rc) s->state = 4;
  return rc;
}

int plonk_session_round5(gm_plonk_session* s, const void* kzg_gamma, void* batch_h_affine) {
  if (s->state != 4) return refuse("round 5 follows round 4");
  if (!kzg_gamma || !batch_h_affine) return refuse("round 5: the folding challenge and the output must be non-null");
  CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  const int rc = GM_PLONK_DISPATCH(s, round5_t)(s, kzg_gamma, batch_h_affine);
  if (!rc) s->state = 5;
  return rc;
}

}  // namespace gm
