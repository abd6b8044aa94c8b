// PLONK linearized polynomial on gfx950 -- replaces computeLinearizedPolynomial /
// innerComputeLinearizedPoly of gnark's PLONK prover
// (backend/plonk/bls12-377/prove.go:656-724, :1233-1368) for polynomials that are
// resident on the device.  The result is defined in include/gnark_mi355x.h
// (gm_plonk_linearize).
//
//   evaluations   l, r, o, s1, s2, qcp_j at zeta and z at w zeta by poly_eval_device
//                 (kzg.hip); the call returns host values, and the blinding parts
//                 (zeta^n - 1) b(x) and every scalar of the combination are O(1)
//                 host work (host_arith.hpp).
//   k_lin_combine one pass over i in [0, n + 3), a lane per coefficient (32 B as two
//                 16 B loads, consecutive lanes consecutive elements; every stream
//                 starts on an element boundary, the h shards at m and 2m too).
//                 Lanes with i < n take the bulk path: every stream is read, no
//                 length tests.  The three lanes i in [n, n + 3) take the tail
//                 path: Z~'s blinding coefficients (a constant per lane, from the
//                 host) and, for i < m, the three h shards.
//   k_lin_blind   the blinded copies l~, r~, o~, z~: a copy with 2 len(b) edited
//                 coefficients.  A kernel of its own: of the four polynomials the
//                 combination holds only z (l, r, o enter through their
//                 evaluations), and its registers are spent on the product.
//
// Number forms (field.hpp): mul(a, b) = a b / 2^(29 N).  Stored values are gnark
// Montgomery elements, the scalars of the combination are internal
// (to_internal_words): mul(gnark, internal) is gnark, so each term is one product
// and nothing is converted.  Z~[i] = z[i] - bz[i] (i < 3) is not formed: the
// host folds -(c2 + a2L) bz[i] into one added constant per edited coefficient,
// together with the StatisticalZK terms of lin[0] and lin[m].
//
// Lazy accumulation: fe_mul_lz leaves a product below 2p unreduced, fe_add_lz adds
// without a test, and one pass at the store (fe_reduce_k<16>, then fe_canon<4>)
// brings any value below 32p to [0, p).  So up to 15 products below 2p and one
// stored element (< p) may be summed before a reduction.  The fixed part sums 9
// products, qk and at most one host constant: below 20p.  nb_bsb is not capped,
// so the BSB22 loop folds at 16p after every product: below 20p + 2p on entry
// to the fold the first time, below 16p + 2p afterwards, below 16p after it.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage;
// BN254 / BLS12-377 Fr), no scratch, no VGPR spill and no LDS in either:
//   k_lin_combine  62 / 63 VGPRs, 8 waves per SIMD
//   k_lin_blind    22 / 22 VGPRs, 8 waves per SIMD
#include <cstring>
#include <vector>

#include "curves.hpp"
#include "kzg.hpp"
#include "ntt.hpp"
#include "plonk_lin.hpp"
#include "runtime.hpp"

namespace gm {

constexpr int LIN_TPB = LIN_BLOCK;

// the constants of one call, by value
template <class P>
struct LinK {
  FeG<P> cz, cs3, cqm, cql, cqr, cqo;  // internal: c2 + a2L, c1, rl, l~(zeta), r~(zeta), o~(zeta)
  FeG<P> ch[3];                        // internal: -zh, -zh zm, -zh zm^2
  FeG<P> lo[3];                        // gnark: added to lin[i], i < 3
  FeG<P> hi[3];                        // gnark: lin[n + i] before the h shards
};

struct LinIn {
  const void *z, *s3, *qm, *ql, *qr, *qo, *qk, *h;
};

// one BSB22 gate: pi2_j and qcp_j(zeta) (internal)
template <class P>
struct LinBsb {
  const void* pi2;
  FeG<P> q;
};

// f[i] k, below 2p
template <class P>
GM_DEV Fe<P> lin_term(const void* __restrict__ f, size_t i, const FeG<P>& k) {
  return fe_mul_lz(fe_load_g<P>(f, i), fe_unpack<P>(k));
}
// one of three call constants by a lane's own index
template <class P>
GM_DEV Fe<P> lin_pick(const FeG<P> (&c)[3], size_t j) {
  FeG<P> g;
#pragma unroll
  for (int w = 0; w < P::NG; w++) g.w[w] = j == 0 ? c[0].w[w] : (j == 1 ? c[1].w[w] : c[2].w[w]);
  return fe_unpack<P>(g);
}

template <class P>
__global__ void __launch_bounds__(LIN_TPB) k_lin_combine(LinIn in, size_t n, size_t nb,
                                                         const LinBsb<P>* __restrict__ bsb, LinK<P> k,
                                                         void* __restrict__ lin) {
  const size_t i = (size_t)blockIdx.x * LIN_TPB + threadIdx.x;
  const size_t m = n + 2;
  if (i >= n + 3) return;
  Fe<P> acc;
  if (i < n) {
    acc = lin_term<P>(in.z, i, k.cz);
    acc = fe_add_lz(acc, lin_term<P>(in.s3, i, k.cs3));
    acc = fe_add_lz(acc, lin_term<P>(in.qm, i, k.cqm));
    acc = fe_add_lz(acc, lin_term<P>(in.ql, i, k.cql));
    acc = fe_add_lz(acc, lin_term<P>(in.qr, i, k.cqr));
    acc = fe_add_lz(acc, lin_term<P>(in.qo, i, k.cqo));
    acc = fe_add_lz(acc, fe_load_g<P>(in.qk, i));
    acc = fe_add_lz(acc, lin_term<P>(in.h, i, k.ch[0]));
    acc = fe_add_lz(acc, lin_term<P>(in.h, m + i, k.ch[1]));
    acc = fe_add_lz(acc, lin_term<P>(in.h, 2 * m + i, k.ch[2]));  // 9 products and qk: < 19p
    if (i < 3) acc = fe_add_lz(acc, lin_pick<P>(k.lo, i));        // < 20p
    for (size_t j = 0; j < nb; j++) {
      const LinBsb<P> b = bsb[j];
      acc = fe_add_lz(acc, lin_term<P>(b.pi2, i, b.q));  // < 22p
      fe_reduce_k<16>(acc);                              // < 16p
    }
  } else {
    // i = n, n + 1 (both below m) and n + 2 = m
    acc = lin_pick<P>(k.hi, i - n);
    if (i < m) {
      acc = fe_add_lz(acc, lin_term<P>(in.h, i, k.ch[0]));
      acc = fe_add_lz(acc, lin_term<P>(in.h, m + i, k.ch[1]));
      acc = fe_add_lz(acc, lin_term<P>(in.h, 2 * m + i, k.ch[2]));  // < 7p
    }
  }
  fe_reduce_k<16>(acc);
  fe_store_g<P>(lin, i, fe_canon<4>(acc));
}

// the blinded copies: blockIdx.y = polynomial (l, r, o, z)
template <class P>
struct LinBlind {
  const void* src[4];
  void* dst[4];
  FeG<P> b[4][3];  // gnark; l, r, o use two
};

template <class P>
__global__ void __launch_bounds__(LIN_TPB) k_lin_blind(LinBlind<P> a, size_t n) {
  const int q = blockIdx.y;
  const size_t nbl = q == 3 ? 3 : 2;
  const size_t i = (size_t)blockIdx.x * LIN_TPB + threadIdx.x;
  void* dst = q == 0 ? a.dst[0] : (q == 1 ? a.dst[1] : (q == 2 ? a.dst[2] : a.dst[3]));
  const void* src = q == 0 ? a.src[0] : (q == 1 ? a.src[1] : (q == 2 ? a.src[2] : a.src[3]));
  if (!dst || i >= n + nbl) return;
  const size_t e = i < n ? i : i - n;  // the blinding coefficient of an edited element
  FeG<P> g;
  if (i < n) g = feg_load<P>(reinterpret_cast<const uint32_t*>(src) + i * P::NG);
  if (i < nbl || i >= n) {
    FeG<P> b;
#pragma unroll
    for (int w = 0; w < P::NG; w++) {
      const uint32_t b0 = q == 0 ? a.b[0][0].w[w] : (q == 1 ? a.b[1][0].w[w] : (q == 2 ? a.b[2][0].w[w] : a.b[3][0].w[w]));
      const uint32_t b1 = q == 0 ? a.b[0][1].w[w] : (q == 1 ? a.b[1][1].w[w] : (q == 2 ? a.b[2][1].w[w] : a.b[3][1].w[w]));
      b.w[w] = e == 0 ? b0 : (e == 1 ? b1 : a.b[3][2].w[w]);
    }
    g = i < n ? fe_pack(fe_sub(fe_unpack<P>(g), fe_unpack<P>(b))) : b;
  }
  feg_store<P>(reinterpret_cast<uint32_t*>(dst) + i * P::NG, g);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <class C>
int plonk_linearize_device(gm_ctx* ctx, const gm_plonk_linearize_in* in, const gm_plonk_linearize_out* out) {
  using Fr = typename C::Fr;
  using HFr = typename C::HFr;
  using HF = host::F<HFr>;
  const size_t n = in->n, nb = in->nb_bsb;
  int logn = 0;
  while (((size_t)1 << logn) < n && logn < 62) logn++;
  if (((size_t)1 << logn) != n || n < 8 || logn > C::TWO_ADICITY || logn > 30) {
    set_error("plonk linearize: n must be a power of two >= 8 within the 2-adicity");
    return GM_ERR_INVALID;
  }
  if (nb && (!in->qcp || !in->pi2)) {
    set_error("plonk linearize: nb_bsb > 0 needs the qcp and pi2 tables");
    return GM_ERR_INVALID;
  }
  const void* host_in[] = {in->bl, in->br, in->bo, in->bz, in->alpha, in->beta, in->gamma, in->zeta};
  for (const void* p : host_in)
    if (!p) {
      set_error("plonk linearize: blinding coefficients and challenges must be non-null");
      return GM_ERR_INVALID;
    }
  if (!out->lin || !out->evals) {
    set_error("plonk linearize: lin and evals must be non-null");
    return GM_ERR_INVALID;
  }
  // every device range of the call: inputs first, then the outputs that were given
  struct Range {
    uintptr_t p;
    size_t len;
  };
  std::vector<Range> rg;
  const void* polys[] = {in->ql, in->qr, in->qm, in->qo, in->qk, in->s1, in->s2, in->s3, in->l, in->r, in->o, in->z};
  for (const void* p : polys) rg.push_back({(uintptr_t)p, n});
  for (size_t j = 0; j < nb; j++) rg.push_back({(uintptr_t)in->qcp[j], n});
  for (size_t j = 0; j < nb; j++) rg.push_back({(uintptr_t)in->pi2[j], n});
  rg.push_back({(uintptr_t)in->h, 4 * n});
  const size_t nin = rg.size();
  for (const Range& r : rg)
    if (!r.p || r.p % 16) {
      set_error("plonk linearize: polynomial pointers must be non-null and 16-byte aligned");
      return GM_ERR_INVALID;
    }
  void* const blinded[4] = {out->l_blinded, out->r_blinded, out->o_blinded, out->z_blinded};
  rg.push_back({(uintptr_t)out->lin, n + 3});
  for (int q = 0; q < 4; q++)
    if (blinded[q]) rg.push_back({(uintptr_t)blinded[q], n + (q == 3 ? 3 : 2)});
  for (size_t a = nin; a < rg.size(); a++) {
    if (rg[a].p % 16) {
      set_error("plonk linearize: output pointers must be 16-byte aligned");
      return GM_ERR_INVALID;
    }
    for (size_t b = 0; b < a; b++)
      if (rg[b].p < rg[a].p + 32 * rg[a].len && rg[a].p < rg[b].p + 32 * rg[b].len) {
        set_error(b < nin ? "plonk linearize: an output must not overlap an input"
                          : "plonk linearize: the outputs must not overlap each other");
        return GM_ERR_INVALID;
      }
  }

  auto ld = [](const void* p, int k) {
    HF v;
    memcpy(v.v, (const char*)p + 32 * k, sizeof(v.v));
    return v;
  };
  const HF alpha = ld(in->alpha, 0), beta = ld(in->beta, 0), gamma = ld(in->gamma, 0), zeta = ld(in->zeta, 0);
  const HF bl[2] = {ld(in->bl, 0), ld(in->bl, 1)}, br[2] = {ld(in->br, 0), ld(in->br, 1)};
  const HF bo[2] = {ld(in->bo, 0), ld(in->bo, 1)}, bz[3] = {ld(in->bz, 0), ld(in->bz, 1), ld(in->bz, 2)};
  const HF g = host::from_u64<HFr>(C::COSET_GEN), one = HF::one();
  // w, the generator of the n domain: the 4 (n / 4) domain's, (g w) / g
  HF w;
  int rc;
  if ((rc = coset4_shift<C>(n / 4, 1, w.v))) return rc;
  w = w * host::finv(g);
  const HF wzeta = w * zeta;

  // ---- evaluations: l, r, o, s1, s2, qcp_j at zeta; z at w zeta
  std::vector<const void*> ep = {in->l, in->r, in->o, in->s1, in->s2};
  for (size_t j = 0; j < nb; j++) ep.push_back(in->qcp[j]);
  const std::vector<size_t> el(ep.size(), n);
  std::vector<HF> ev(ep.size());
  HF zv;
  if ((rc = poly_eval_device<C>(ctx, ep.data(), el.data(), ep.size(), zeta.v, ev.data()))) return rc;
  if ((rc = poly_eval_device<C>(ctx, &in->z, &n, 1, wzeta.v, zv.v))) return rc;

  // ---- the scalars
  const uint64_t en[1] = {n};
  const HF zn = host::fpow(zeta, en, 1);
  const HF zh = zn - one, zm = zn * zeta * zeta;
  const HF le = ev[0] + zh * (bl[0] + bl[1] * zeta);
  const HF re = ev[1] + zh * (br[0] + br[1] * zeta);
  const HF oe = ev[2] + zh * (bo[0] + bo[1] * zeta);
  const HF s1e = ev[3], s2e = ev[4];
  const HF zue = zv + zh * (bz[0] + (bz[1] + bz[2] * wzeta) * wzeta);  // (w zeta)^n = zeta^n
  const HF rl = le * re;
  const HF c1 = alpha * (le + beta * s1e + gamma) * (re + beta * s2e + gamma) * beta * zue;
  const HF c2 = -(alpha * (le + beta * zeta + gamma) * (re + beta * g * zeta + gamma) *
                  (oe + beta * g * g * zeta + gamma));
  // finv(0) = 0: gnark's Inverse
  const HF a2l = alpha * alpha * zh * host::finv(zeta - one) * host::finv(host::from_u64<HFr>(n));
  const HF cz = c2 + a2l;

  const HF res[6] = {le, re, oe, s1e, s2e, zue};
  memcpy(out->evals, res, sizeof(res));
  if (nb) memcpy((char*)out->evals + sizeof(res), ev.data() + 5, 32 * nb);

  auto I = [](const HF& v) { return to_internal_words<C>(v); };
  auto G = [](const HF& h) {
    FeG<Fr> r;
    static_assert(sizeof(r.w) == sizeof(h.v), "gnark layout");
    memcpy(r.w, h.v, sizeof(r.w));
    return r;
  };
  LinK<Fr> k;
  k.cz = I(cz);
  k.cs3 = I(c1);
  k.cqm = I(rl);
  k.cql = I(le);
  k.cqr = I(re);
  k.cqo = I(oe);
  k.ch[0] = I(-zh);
  k.ch[1] = I(-(zh * zm));
  k.ch[2] = I(-(zh * zm * zm));
  HF lo[3], hi[3];
  for (int i = 0; i < 3; i++) {
    hi[i] = cz * bz[i];
    lo[i] = -hi[i];
  }
  if (in->h_rand) {
    // h1' = h1 + rho0 X^m, h2' = h2 - rho0 + rho1 X^m, h3' = h3 - rho1 (prove.go:619-654)
    const HF r0 = ld(in->h_rand, 0), r1 = ld(in->h_rand, 1);
    lo[0] = lo[0] + zh * (zm * r0 + zm * zm * r1);
    hi[2] = hi[2] - zh * (r0 + zm * r1);
  }
  for (int i = 0; i < 3; i++) {
    k.lo[i] = G(lo[i]);
    k.hi[i] = G(hi[i]);
  }

  Arena arena(ctx);
  DevBuf tab;
  std::vector<LinBsb<Fr>> bsb(nb);
  if (nb) {
    for (size_t j = 0; j < nb; j++) bsb[j] = {in->pi2[j], I(ev[5 + j])};
    if ((rc = tab.alloc(arena, nb * sizeof(LinBsb<Fr>)))) return rc;
    // synchronous: bsb leaves with this frame
    GM_HIP(hipMemcpy(tab.p, bsb.data(), nb * sizeof(LinBsb<Fr>), hipMemcpyHostToDevice));
  }
  const LinIn lin_in = {in->z, in->s3, in->qm, in->ql, in->qr, in->qo, in->qk, in->h};
  {
    ProfScope ps(ctx, "plonk_lin_combine");
    hipLaunchKernelGGL(k_lin_combine<Fr>, dim3(blocks_for(n + 3, LIN_TPB)), dim3(LIN_TPB), 0, ctx->stream, lin_in, n,
                       nb, (const LinBsb<Fr>*)tab.p, k, out->lin);
    GM_HIP(hipGetLastError());
  }
  if (blinded[0] || blinded[1] || blinded[2] || blinded[3]) {
    LinBlind<Fr> a;
    const void* src[4] = {in->l, in->r, in->o, in->z};
    const HF* bs[4] = {bl, br, bo, bz};
    for (int q = 0; q < 4; q++) {
      a.src[q] = src[q];
      a.dst[q] = blinded[q];
      for (int e = 0; e < 3; e++) a.b[q][e] = G(e < (q == 3 ? 3 : 2) ? bs[q][e] : HF::zero());
    }
    ProfScope ps(ctx, "plonk_lin_blind");
    hipLaunchKernelGGL(k_lin_blind<Fr>, dim3(blocks_for(n + 3, LIN_TPB), 4), dim3(LIN_TPB), 0, ctx->stream, a, n);
    GM_HIP(hipGetLastError());
  }
  return GM_OK;
}

template int plonk_linearize_device<CurveBN254>(gm_ctx*, const gm_plonk_linearize_in*, const gm_plonk_linearize_out*);
template int plonk_linearize_device<CurveBLS12377>(gm_ctx*, const gm_plonk_linearize_in*,
                                                   const gm_plonk_linearize_out*);

}  // namespace gm
