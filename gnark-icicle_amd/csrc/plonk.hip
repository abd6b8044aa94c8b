// PLONK quotient on gfx950 -- replaces computeNumerator + divideByZH of gnark's
// PLONK prover (backend/plonk/bls12-377/prove.go:771-1034, :1178-1231) for
// polynomials that are resident on the device.  The result is defined in
// include/gnark_mi355x.h (gm_plonk_quotient): h of degree < 4n with h = T / Z_H on
// the 4n coset g <w1>.
//
// The 4n coset is the union of the four cosets c_i <w0>, c_i = g w1^i, w0 = w1^4,
// and point g w1^(4j + i) = c_i w0^j.  Per coset:
//   * every input polynomial is copied into workspace and taken to its n values
//     on c_i <w0> by a size-n forward DIF with c_i^k multiplied in on load
//     (coset4_ntt_device): position p holds the value at x = c_i w0^brev(p);
//   * L1 = Z_H / (n (X - 1)) = (1/n) sum_k X^k goes the same way from the
//     constant coefficient vector 1/n (exact, no inversion per point);
//   * k_plonk_constraint evaluates T / Z_H, one thread per position p.  x comes
//     from the domain's table w0^brev(p) times c_i; Z~(w0 x) is position
//     brev(brev(p) + 1 mod n) of the same coset; the blinding terms are
//     Z_H(c_i) b(x) with Z_H(c_i) = c_i^n - 1 one constant per coset, computed
//     and inverted on the host.
// The value of point 4j + i belongs at bit-reversed position brev2(i) n + brev(j)
// of the 4n vector, i.e. coset i fills the contiguous block brev2(i) n + p: the
// constraint kernel's stores are as consecutive as its loads, and one inverse
// coset DIT of size 4n (bit-reversed in, natural out, g^-k / 4n on store) leaves h
// in regular order.
//
// Number forms (field.hpp): mul(a, b) = a b / 2^(29 N).  Stored values are gnark
// Montgomery elements (v 2^256), tables and most constants internal (v 2^(29 N)):
// mul(gnark, internal) is gnark, mul(internal, internal) is internal, and a
// product of two gnark elements carries the factor 2^(256 - 29 N), which the
// constant that multiplies it next takes out again (k_bsb, k_lag).  The wires are
// converted to internal form once, so every gate and permutation product is one
// multiplication.  Every sum and product is fully reduced: whatever the order
// of the products, the stored words are gnark-crypto's.
#include <cstring>

#include "curves.hpp"
#include "kzg.hpp"
#include "ntt.hpp"
#include "plonk.hpp"
#include "runtime.hpp"

namespace gm {

constexpr int PLONK_TPB = 256;
// workspace slots (n elements each); the BSB22 pairs follow
enum { PQ_QL, PQ_QR, PQ_QM, PQ_QO, PQ_QK, PQ_S1, PQ_S2, PQ_S3, PQ_L, PQ_R, PQ_O, PQ_Z, PQ_L1, PQ_FIXED };
// With a key's coset cache (PlonkCosetCache, plonk.hpp) only the per-proof
// polynomials go through workspace; the PI2_j follow.  The fixed ones are read
// from the cache's block of the coset, slots PC_* (plonk.hpp), the Qcp_j last.
enum { PW_QK, PW_L, PW_R, PW_O, PW_Z, PW_FIXED };

// the constants of one coset, by value
template <class P>
struct QuotCoset {
  FeG<P> c;                    // internal: the shift c_i
  FeG<P> bl[2], br[2], bo[2];  // internal: Z_H(c_i) times the blinding coefficients
  FeG<P> bz[3];                // gnark: Z_H(c_i) bz_k
  FeG<P> bzs[2];               // gnark: Z_H(c_i) bz_k w0^k, k = 1, 2 (bz at w0 x)
  FeG<P> beta_s;               // beta 2^(29 N - 256), internal: mul(S gnark, beta_s) = beta S internal
  FeG<P> beta[3];              // internal: beta, beta g, beta g^2
  FeG<P> gamma;                // internal
  FeG<P> one;                  // gnark
  FeG<P> k_gate;               // internal: 1 / Z_H(c_i)
  FeG<P> k_bsb;                // internal: 2^(29 N - 256) / Z_H(c_i)
  FeG<P> k_perm;               // internal: alpha / Z_H(c_i)
  FeG<P> k_lag;                // internal: alpha^2 2^(29 N - 256) / Z_H(c_i)
};

// ev: the (PQ_FIXED + 2 nb) coset evaluations, slot k at element k n; out: the
// coset's block of the 4n vector.  Lane p reads element p of every slot (32 B,
// consecutive lanes consecutive) and one element of the Z slot elsewhere.
// CACHED: ev holds the PW_FIXED + nb per-proof slots only and fx, the key's cache
// block of this coset, the PC_FIXED + nb fixed ones.  Which of the two holds slot
// k, and where, is a table of compile-time constants (PQ_WHERE), so either
// variant does the address arithmetic the kernel did before.
struct PqWhere {
  bool fixed;
  int slot;
};
__device__ constexpr PqWhere PQ_WHERE[PQ_FIXED] = {
    {true, PC_QL}, {true, PC_QR}, {true, PC_QM}, {true, PC_QO}, {false, PW_QK}, {true, PC_S1}, {true, PC_S2},
    {true, PC_S3}, {false, PW_L}, {false, PW_R}, {false, PW_O}, {false, PW_Z},  {true, PC_L1}};

template <class P, bool CACHED>
__global__ void __launch_bounds__(PLONK_TPB) k_plonk_constraint(const void* __restrict__ ev,
                                                                const void* __restrict__ fx, size_t n, int logn,
                                                                int nb, const Fe<P>* __restrict__ wbrev,
                                                                QuotCoset<P> q, void* __restrict__ out) {
  const size_t p = (size_t)blockIdx.x * PLONK_TPB + threadIdx.x;
  if (p >= n) return;
  // one of the thirteen named slots
  auto at = [&](int k, size_t idx) {
    if (!CACHED) return fe_load_g<P>(ev, (size_t)k * n + idx);
    return PQ_WHERE[k].fixed ? fe_load_g<P>(fx, (size_t)PQ_WHERE[k].slot * n + idx)
                             : fe_load_g<P>(ev, (size_t)PQ_WHERE[k].slot * n + idx);
  };
  // the BSB22 pairs behind them
  auto qcp_at = [&](int j, size_t idx) {
    return CACHED ? fe_load_g<P>(fx, (size_t)(PC_FIXED + j) * n + idx)
                  : fe_load_g<P>(ev, (size_t)(PQ_FIXED + j) * n + idx);
  };
  auto pi2_at = [&](int j, size_t idx) {
    return fe_load_g<P>(ev, (size_t)((CACHED ? PW_FIXED : PQ_FIXED + nb) + j) * n + idx);
  };
  auto U = [](const FeG<P>& g) { return fe_unpack<P>(g); };
  // Z(w0 x): evaluation index brev(p) + 1 mod n
  const size_t pn = brev_bits((brev_bits((uint32_t)p, logn) + 1) & (uint32_t)(n - 1), logn);
  const Fe<P> x = fe_mul(wbrev[p], U(q.c));  // internal
  const Fe<P> x2 = fe_sqr(x);
  // blinded wires, internal form: W + Z_H (b0 + b1 x)
  const Fe<P> L = fe_add(fe_to_internal(at(PQ_L, p)), fe_add(U(q.bl[0]), fe_mul(U(q.bl[1]), x)));
  const Fe<P> R = fe_add(fe_to_internal(at(PQ_R, p)), fe_add(U(q.br[0]), fe_mul(U(q.br[1]), x)));
  const Fe<P> O = fe_add(fe_to_internal(at(PQ_O, p)), fe_add(U(q.bo[0]), fe_mul(U(q.bo[1]), x)));
  // Z~(x) and Z~(w0 x), gnark form
  const Fe<P> bz0 = U(q.bz[0]);
  const Fe<P> Z = fe_add(fe_add(at(PQ_Z, p), bz0), fe_add(fe_mul(U(q.bz[1]), x), fe_mul(U(q.bz[2]), x2)));
  const Fe<P> ZS = fe_add(fe_add(at(PQ_Z, pn), bz0), fe_add(fe_mul(U(q.bzs[0]), x), fe_mul(U(q.bzs[1]), x2)));
  // gate: L (Ql + Qm R) + Qr R + Qo O + Qk, gnark
  Fe<P> gate = fe_mul(fe_add(at(PQ_QL, p), fe_mul(at(PQ_QM, p), R)), L);
  gate = fe_add(gate, fe_mul(at(PQ_QR, p), R));
  gate = fe_add(gate, fe_mul(at(PQ_QO, p), O));
  gate = fe_add(gate, at(PQ_QK, p));
  Fe<P> acc = fe_mul(gate, U(q.k_gate));
  if (nb) {
    Fe<P> bsb = fe_zero<P>();  // gnark times 2^(256 - 29 N)
    for (int k = 0; k < nb; k++) bsb = fe_add(bsb, fe_mul(qcp_at(k, p), pi2_at(k, p)));
    acc = fe_add(acc, fe_mul(bsb, U(q.k_bsb)));
  }
  // permutation
  const Fe<P> gam = U(q.gamma), bs = U(q.beta_s);
  const Fe<P> Lg = fe_add(L, gam), Rg = fe_add(R, gam), Og = fe_add(O, gam);
  Fe<P> a = fe_mul(ZS, fe_add(Lg, fe_mul(at(PQ_S1, p), bs)));
  a = fe_mul(a, fe_add(Rg, fe_mul(at(PQ_S2, p), bs)));
  a = fe_mul(a, fe_add(Og, fe_mul(at(PQ_S3, p), bs)));
  Fe<P> b = fe_mul(Z, fe_add(Lg, fe_mul(U(q.beta[0]), x)));
  b = fe_mul(b, fe_add(Rg, fe_mul(U(q.beta[1]), x)));
  b = fe_mul(b, fe_add(Og, fe_mul(U(q.beta[2]), x)));
  acc = fe_add(acc, fe_mul(fe_sub(a, b), U(q.k_perm)));
  // alpha^2 (Z~ - 1) L1
  acc = fe_add(acc, fe_mul(fe_mul(fe_sub(Z, U(q.one)), at(PQ_L1, p)), U(q.k_lag)));
  fe_store_g<P>(out, p, acc);
}

template <class P>
__global__ void __launch_bounds__(PLONK_TPB) k_fill_const(void* __restrict__ dst, size_t n, FeG<P> v) {
  const size_t i = (size_t)blockIdx.x * PLONK_TPB + threadIdx.x;
  if (i < n) feg_store<P>(reinterpret_cast<uint32_t*>(dst) + i * P::NG, v);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <class HF, class Fr>
static FeG<Fr> gnark_words(const HF& h) {
  FeG<Fr> r;
  static_assert(sizeof(r.w) == sizeof(h.v), "gnark layout");
  memcpy(r.w, h.v, sizeof(r.w));
  return r;
}

// The cache of a key: the fixed polynomials' values on the four cosets, exactly
// what the loop below leaves in their workspace slots (same calls, same order of
// operations), block i = coset i, slot k of a block at element (i slots + k) n.
template <class C>
int plonk_coset_cache_build(gm_ctx* ctx, size_t n, const void* const* fixed, size_t nb, void* cache) {
  using Fr = typename C::Fr;
  using HF = host::F<typename C::HFr>;
  const size_t slots = PC_FIXED + nb;
  const FeG<Fr> ninv = gnark_words<HF, Fr>(host::finv(host::from_u64<typename C::HFr>(n)));
  int rc;
  for (int i = 0; i < 4; i++)
    for (size_t k = 0; k < slots; k++) {
      char* slot = (char*)cache + 32 * n * (i * slots + k);
      const size_t f = k < PC_L1 ? k : k - 1;  // fixed[]: ql qr qm qo s1 s2 s3 qcp_0 ..
      if (k == PC_L1) {
        hipLaunchKernelGGL(k_fill_const<Fr>, dim3(blocks_for(n, PLONK_TPB)), dim3(PLONK_TPB), 0, ctx->stream,
                           (void*)slot, n, ninv);
        GM_HIP(hipGetLastError());
      } else {
        GM_HIP(hipMemcpyAsync(slot, fixed[f], 32 * n, hipMemcpyDeviceToDevice, ctx->stream));
      }
      if ((rc = coset4_ntt_device<C>(ctx, slot, n, i))) return rc;
    }
  return GM_OK;
}

template <class C>
int plonk_quotient_device(gm_ctx* ctx, const gm_plonk_quotient_in* in, void* h_dev, const PlonkCosetCache* cache) {
  using Fr = typename C::Fr;
  using HFr = typename C::HFr;
  using HF = host::F<HFr>;
  const size_t n = in->n, nb = in->nb_bsb;
  int logn = 0;
  while (((size_t)1 << logn) < n && logn < 62) logn++;
  if (((size_t)1 << logn) != n || n < 8 || logn + 2 > C::TWO_ADICITY || logn + 2 > 30) {
    set_error("plonk quotient: n must be a power of two >= 8 with 4n within the 2-adicity");
    return GM_ERR_INVALID;
  }
  if (nb > 1024 || (nb && (!in->qcp || !in->pi2))) {
    set_error("plonk quotient: nb_bsb > 0 needs the qcp and pi2 tables (at most 1024 gates)");
    return GM_ERR_INVALID;
  }
  // sources in workspace-slot order
  std::vector<const void*> src = {in->ql, in->qr, in->qm, in->qo, in->qk, in->s1, in->s2,
                                  in->s3, in->l,  in->r,  in->o,  in->z,  nullptr /* L1 */};
  for (size_t k = 0; k < nb; k++) src.push_back(in->qcp[k]);
  for (size_t k = 0; k < nb; k++) src.push_back(in->pi2[k]);
  const void* host_in[] = {in->bl, in->br, in->bo, in->bz, in->alpha, in->beta, in->gamma};
  for (const void* p : host_in)
    if (!p) {
      set_error("plonk quotient: blinding coefficients and challenges must be non-null");
      return GM_ERR_INVALID;
    }
  if (!h_dev || (uintptr_t)h_dev % 16) {
    set_error("plonk quotient: h must be non-null and 16-byte aligned");
    return GM_ERR_INVALID;
  }
  const uintptr_t h0 = (uintptr_t)h_dev, h1 = h0 + 32 * 4 * n;
  for (size_t k = 0; k < src.size(); k++) {
    if (k == PQ_L1) continue;
    const uintptr_t p0 = (uintptr_t)src[k];
    if (!p0 || p0 % 16) {
      set_error("plonk quotient: polynomial pointers must be non-null and 16-byte aligned");
      return GM_ERR_INVALID;
    }
    if (p0 < h1 && h0 < p0 + 32 * n) {
      set_error("plonk quotient: h must not overlap an input");
      return GM_ERR_INVALID;
    }
  }

  auto ld = [](const void* p, int k) {
    HF v;
    memcpy(v.v, (const char*)p + 32 * k, sizeof(v.v));
    return v;
  };
  const HF alpha = ld(in->alpha, 0), beta = ld(in->beta, 0), gamma = ld(in->gamma, 0);
  const HF g = host::from_u64<HFr>(C::COSET_GEN);
  // 2^(29 N - 256): takes the factor of a gnark x gnark product out again
  const HF kin = host::from_u64<HFr>(1ull << (RADIX * Fr::N - 32 * Fr::NG));
  HF shift[4];
  int rc;
  for (int i = 0; i < 4; i++)
    if ((rc = coset4_shift<C>(n, i, shift[i].v))) return rc;
  HF w0 = shift[1] * host::finv(shift[0]);  // w1
  w0 = w0 * w0;
  w0 = w0 * w0;
  const uint64_t en[1] = {n};

  if (cache && (!cache->base || cache->n != n || cache->nb_bsb != nb)) {
    set_error("plonk quotient: the coset cache belongs to another key shape");
    return GM_ERR_INVALID;
  }
  // workspace slot of source k: its own, or with a cache only the per-proof ones
  std::vector<int> ws(src.size());
  size_t nws = 0;
  for (size_t k = 0; k < src.size(); k++) {
    const bool per_proof = k == PQ_QK || (k >= PQ_L && k <= PQ_Z) || k >= PQ_FIXED + nb;
    ws[k] = !cache ? (int)k : per_proof ? (int)nws : -1;
    nws += per_proof;
  }
  if (!cache) nws = src.size();
  Arena arena(ctx);
  DevBuf ev;
  if ((rc = ev.alloc(arena, 32 * n * nws))) return rc;
  const void* wbrev;
  if ((rc = ntt_brev_roots<C>(ctx, n, &wbrev))) return rc;
  const FeG<Fr> ninv = gnark_words<HF, Fr>(host::finv(host::from_u64<HFr>(n)));
  const unsigned grid = blocks_for(n, PLONK_TPB);
  auto I = [](const HF& v) { return to_internal_words<C>(v); };
  auto G = [](const HF& v) { return gnark_words<HF, Fr>(v); };

  for (int i = 0; i < 4; i++) {
    for (size_t k = 0; k < src.size(); k++) {
      if (ws[k] < 0) continue;  // in the key's cache
      char* slot = ev.as<char>() + 32 * n * ws[k];
      if (k == PQ_L1) {
        hipLaunchKernelGGL(k_fill_const<Fr>, dim3(grid), dim3(PLONK_TPB), 0, ctx->stream, (void*)slot, n, ninv);
        GM_HIP(hipGetLastError());
      } else {
        GM_HIP(hipMemcpyAsync(slot, src[k], 32 * n, hipMemcpyDeviceToDevice, ctx->stream));
      }
      if ((rc = coset4_ntt_device<C>(ctx, slot, n, i))) return rc;
    }
    const HF c = shift[i];
    // c^n = g^n times a fourth root of unity; g generates the whole group, so it is never 1
    const HF zh = host::fpow(c, en, 1) - HF::one();
    const HF zhinv = host::finv(zh);
    QuotCoset<Fr> q;
    q.c = I(c);
    for (int k = 0; k < 2; k++) {
      q.bl[k] = I(zh * ld(in->bl, k));
      q.br[k] = I(zh * ld(in->br, k));
      q.bo[k] = I(zh * ld(in->bo, k));
    }
    for (int k = 0; k < 3; k++) q.bz[k] = G(zh * ld(in->bz, k));
    q.bzs[0] = G(zh * ld(in->bz, 1) * w0);
    q.bzs[1] = G(zh * ld(in->bz, 2) * w0 * w0);
    q.beta_s = I(beta * kin);
    q.beta[0] = I(beta);
    q.beta[1] = I(beta * g);
    q.beta[2] = I(beta * g * g);
    q.gamma = I(gamma);
    q.one = G(HF::one());
    q.k_gate = I(zhinv);
    q.k_bsb = I(zhinv * kin);
    q.k_perm = I(alpha * zhinv);
    q.k_lag = I(alpha * alpha * zhinv * kin);
    const size_t block = (size_t)(((i & 1) << 1) | (i >> 1)) * n;  // brev2(i) n
    ProfScope ps(ctx, "plonk_constraint");
    if (cache) {
      const void* fx = (const char*)cache->base + 32 * n * (PC_FIXED + nb) * i;
      hipLaunchKernelGGL((k_plonk_constraint<Fr, true>), dim3(grid), dim3(PLONK_TPB), 0, ctx->stream,
                         (const void*)ev.p, fx, n, logn, (int)nb, (const Fe<Fr>*)wbrev, q,
                         (void*)((char*)h_dev + 32 * block));
    } else {
      hipLaunchKernelGGL((k_plonk_constraint<Fr, false>), dim3(grid), dim3(PLONK_TPB), 0, ctx->stream,
                         (const void*)ev.p, (const void*)nullptr, n, logn, (int)nb, (const Fe<Fr>*)wbrev, q,
                         (void*)((char*)h_dev + 32 * block));
    }
    GM_HIP(hipGetLastError());
  }
  return ntt_device<C>(ctx, h_dev, 4 * n, true, true, true);
}

template int plonk_quotient_device<CurveBN254>(gm_ctx*, const gm_plonk_quotient_in*, void*, const PlonkCosetCache*);
template int plonk_quotient_device<CurveBLS12377>(gm_ctx*, const gm_plonk_quotient_in*, void*,
                                                  const PlonkCosetCache*);
template int plonk_coset_cache_build<CurveBN254>(gm_ctx*, size_t, const void* const*, size_t, void*);
template int plonk_coset_cache_build<CurveBLS12377>(gm_ctx*, size_t, const void* const*, size_t, void*);

}  // namespace gm
