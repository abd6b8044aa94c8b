// Polynomial work of the KZG openings on gfx950 -- replaces the host Horner
// evaluation, the gamma-fold and the synthetic division of gnark-crypto's
// kzg.Open / kzg.BatchOpenSinglePoint (dividePolyByXminusA) for polynomials
// that are resident on the device.
//
// One suffix recurrence gives both results.  For f of m coefficients and a point z
//   s[m] = 0,  s[i] = f[i] + z s[i+1]   =>   f(z) = s[0],  q[i] = s[i+1]  (i <= m-2)
// with q = (f - f(z)) / (X - z).  The scan is blocked: a chunk is C = TPB * E
// consecutive coefficients, a thread owns a run of E of them.
//   k_poly_chunk_eval   c_k = sum_{j in chunk k} f[j] z^(j - kC)   (Horner per run,
//                       then an LDS tree lo + z^(E 2^d) hi)
//   k_poly_chunk_carry  in place, c_k -> S_k = s[kC] = c_k + z^C S_{k+1}; S_0 = f(z)
//                       (one block: the same run / scan shape over the chunk values)
//   k_poly_div_write    s[i] inside chunk k from the runs' Horner values (a
//                       Hillis-Steele suffix scan over the TPB runs) and S_{k+1};
//                       q[i-1] = s[i]
// All runs have one length and all chunks have one length, so the multiplier of a
// combine level is one power of z for the whole launch: z^(E 2^d), computed on the
// host by squaring and passed by value (PolyPoint).  Only the additive part is
// scanned.
//
// Number forms: coefficients, s and every stored value are gnark Montgomery
// elements, the powers of z are internal-form (field.hpp): mul(a_gnark,
// w_internal) = (a w)_gnark, so nothing is converted on the way in or out.  Every
// sum and product is fully reduced, so the stored words are gnark-crypto's.
#include <cstring>
#include <vector>

#include "curves.hpp"
#include "kzg.hpp"
#include "runtime.hpp"

namespace gm {

constexpr int KZG_TPB_LOG = 7;
constexpr int KZG_TPB = 1 << KZG_TPB_LOG;
constexpr int KZG_E_LOG = 3;
constexpr int KZG_E = 1 << KZG_E_LOG;      // coefficients per thread
constexpr int KZG_C = KZG_TPB * KZG_E;     // coefficients per chunk (1024)
constexpr int KZG_R_LOG = 2;
constexpr int KZG_R = 1 << KZG_R_LOG;      // chunks per thread of the carry scan
// pw[d] = z^(E 2^d): pw[TPB_LOG] = z^C = Z, pw[TPB_LOG + R_LOG + d] = Z^(R 2^d)
constexpr int KZG_NPOW = 2 * KZG_TPB_LOG + KZG_R_LOG;
// LDS staging of a chunk: gnark words as 16 B units, a run's 2E units followed by
// one unit of padding, so the runs of consecutive lanes start 17 units apart
// (ds_read_b128 of lane t at unit 17 t + const: the 16 lanes of a group on 16
// different 4-bank slots)
constexpr int KZG_RUN_U4 = 2 * KZG_E + 1;
constexpr unsigned KZG_MAX_GRID_Y = 65535;

// z and its powers, internal form in gnark's word layout
template <class P>
struct PolyPoint {
  FeG<P> z;
  FeG<P> pw[KZG_NPOW];
};

// one polynomial of a batch: coefficients, length, first slot in the chunk array
struct PolyRef {
  const void* p;
  size_t len;
  size_t off;
};

// Coefficients [base, base + C) of f -> staging; zero at and past m.  Lane t
// loads unit r TPB + t: 16 B per lane, consecutive lanes consecutive addresses.
template <class P>
GM_DEV void chunk_load(uint4* __restrict__ stage, const void* __restrict__ f, size_t m, size_t base) {
  static_assert(P::NG == 8, "two 16 B units per element");
  const uint4* src = reinterpret_cast<const uint4*>(f);
#pragma unroll
  for (int r = 0; r < 2 * KZG_E; r++) {
    const int u = r * KZG_TPB + (int)threadIdx.x;
    const int e = u >> 1;
    const size_t g = base + e;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (g < m) v = src[2 * g + (u & 1)];
    stage[(e >> KZG_E_LOG) * KZG_RUN_U4 + (e & (KZG_E - 1)) * 2 + (u & 1)] = v;
  }
}
// element e of run t (gnark form, unpacked)
template <class P>
GM_DEV Fe<P> stage_get(const uint4* __restrict__ stage, int t, int e) {
  const uint4 a = stage[t * KZG_RUN_U4 + 2 * e], b = stage[t * KZG_RUN_U4 + 2 * e + 1];
  FeG<P> g;
  g.w[0] = a.x, g.w[1] = a.y, g.w[2] = a.z, g.w[3] = a.w;
  g.w[4] = b.x, g.w[5] = b.y, g.w[6] = b.z, g.w[7] = b.w;
  return fe_unpack<P>(g);
}
template <class P>
GM_DEV void stage_put(uint4* __restrict__ stage, int t, int e, const Fe<P>& v) {
  const FeG<P> g = fe_pack(v);
  stage[t * KZG_RUN_U4 + 2 * e] = make_uint4(g.w[0], g.w[1], g.w[2], g.w[3]);
  stage[t * KZG_RUN_U4 + 2 * e + 1] = make_uint4(g.w[4], g.w[5], g.w[6], g.w[7]);
}
// sum_e run[e] z^e
template <class P>
GM_DEV Fe<P> run_horner(const uint4* __restrict__ stage, int t, const Fe<P>& z) {
  Fe<P> h = stage_get<P>(stage, t, KZG_E - 1);
#pragma unroll
  for (int e = KZG_E - 2; e >= 0; e--) h = fe_add(stage_get<P>(stage, t, e), fe_mul(h, z));
  return h;
}

// blockIdx.y: polynomial, blockIdx.x: chunk (blocks past a shorter polynomial's
// last chunk leave at once).  chunks[off + k] = c_k.
template <class P>
__global__ void __launch_bounds__(KZG_TPB) k_poly_chunk_eval(const PolyRef* __restrict__ polys, PolyPoint<P> pt,
                                                             void* __restrict__ chunks) {
  __shared__ uint4 stage[KZG_TPB * KZG_RUN_U4];
  __shared__ Fe<P> v[KZG_TPB];
  const PolyRef pr = polys[blockIdx.y];
  const size_t base = (size_t)blockIdx.x * KZG_C;
  if (base >= pr.len) return;
  chunk_load<P>(stage, pr.p, pr.len, base);
  __syncthreads();
  const int t = threadIdx.x;
  v[t] = run_horner<P>(stage, t, fe_unpack<P>(pt.z));
  // level d: v[j 2^(d+1)] += z^(E 2^d) v[j 2^(d+1) + 2^d], the active threads packed
  // into the low lanes
  for (int d = 0; d < KZG_TPB_LOG; d++) {
    __syncthreads();
    if (t < (KZG_TPB >> (d + 1))) {
      const int lo = t << (d + 1);
      v[lo] = fe_add(v[lo], fe_mul(v[lo + (1 << d)], fe_unpack<P>(pt.pw[d])));
    }
  }
  if (t == 0) fe_store_g<P>(chunks, pr.off + blockIdx.x, v[0]);
}

// One block per polynomial: the chunk values become their suffix scan with
// multiplier Z = z^C, S_k = c_k + Z S_{k+1}, in tiles of TPB * R chunks from the
// top down.  A thread owns a run of R consecutive chunks: Horner over the run,
// a Hillis-Steele suffix scan over the TPB run values with multiplier
// Z^(R 2^d), then down the run again from the next run's S.  The tile's topmost
// run takes in the S of the tile above.  Chunk slots at and past the last chunk
// hold nothing and count as zero; every S above them is zero too, so they are
// skipped.  vals[blockIdx.x] = S_0 = f(z) (0 for an empty polynomial).
template <class P>
__global__ void __launch_bounds__(KZG_TPB) k_poly_chunk_carry(const PolyRef* __restrict__ polys, PolyPoint<P> pt,
                                                              void* __restrict__ chunks, void* __restrict__ vals) {
  __shared__ Fe<P> v[KZG_TPB];
  const PolyRef pr = polys[blockIdx.x];
  const size_t nchunk = (pr.len + KZG_C - 1) / KZG_C;
  const int t = threadIdx.x;
  const Fe<P> Z = fe_unpack<P>(pt.pw[KZG_TPB_LOG]);
  constexpr int TILE = KZG_TPB * KZG_R;
  Fe<P> above = fe_zero<P>();
  for (size_t tile = (nchunk + TILE - 1) / TILE; tile-- > 0;) {
    const size_t k0 = tile * TILE + (size_t)t * KZG_R;
    Fe<P> x = fe_zero<P>();
#pragma unroll
    for (int j = KZG_R - 1; j >= 0; j--)
      if (k0 + j < nchunk) x = fe_add(fe_load_g<P>(chunks, pr.off + k0 + j), fe_mul(x, Z));
    if (t == KZG_TPB - 1) x = fe_add(x, fe_mul(above, fe_unpack<P>(pt.pw[KZG_TPB_LOG + KZG_R_LOG])));
    v[t] = x;
    for (int d = 0; d < KZG_TPB_LOG; d++) {
      __syncthreads();
      const bool has = t + (1 << d) < KZG_TPB;
      Fe<P> hi = fe_zero<P>();
      if (has) hi = v[t + (1 << d)];
      __syncthreads();
      if (has) {
        x = fe_add(x, fe_mul(hi, fe_unpack<P>(pt.pw[KZG_TPB_LOG + KZG_R_LOG + d])));
        v[t] = x;
      }
    }
    __syncthreads();
    Fe<P> s = t + 1 < KZG_TPB ? v[t + 1] : above;
    above = v[0];
#pragma unroll
    for (int j = KZG_R - 1; j >= 0; j--)
      if (k0 + j < nchunk) {
        s = fe_add(fe_load_g<P>(chunks, pr.off + k0 + j), fe_mul(s, Z));
        fe_store_g<P>(chunks, pr.off + k0 + j, s);
      }
    __syncthreads();
  }
  if (t == 0) fe_store_g<P>(vals, blockIdx.x, above);
}

// One block per chunk of f (gridDim.x chunks).  S: the scanned chunk values.
// q[i-1] = s[i] for the chunk's i in [1, m): the chunk's first coefficient goes
// one element below the chunk's lower edge.
template <class P>
__global__ void __launch_bounds__(KZG_TPB) k_poly_div_write(const void* __restrict__ f, size_t m, PolyPoint<P> pt,
                                                            const void* __restrict__ S, void* __restrict__ q) {
  __shared__ uint4 stage[KZG_TPB * KZG_RUN_U4];
  __shared__ Fe<P> v[KZG_TPB];
  const size_t kc = blockIdx.x;
  const size_t base = kc * KZG_C;
  chunk_load<P>(stage, f, m, base);
  __syncthreads();
  const int t = threadIdx.x;
  const Fe<P> z = fe_unpack<P>(pt.z);
  const Fe<P> carry = kc + 1 < gridDim.x ? fe_load_g<P>(S, kc + 1) : fe_zero<P>();  // s[base + C]
  Fe<P> x = run_horner<P>(stage, t, z);
  if (t == KZG_TPB - 1) x = fe_add(x, fe_mul(carry, fe_unpack<P>(pt.pw[0])));
  v[t] = x;
  // suffix scan over the runs: x -> s[base + t E]
  for (int d = 0; d < KZG_TPB_LOG; d++) {
    __syncthreads();
    const bool has = t + (1 << d) < KZG_TPB;
    Fe<P> hi = fe_zero<P>();
    if (has) hi = v[t + (1 << d)];
    __syncthreads();
    if (has) {
      x = fe_add(x, fe_mul(hi, fe_unpack<P>(pt.pw[d])));
      v[t] = x;
    }
  }
  __syncthreads();
  // s at the start of the next run, then down this run; s[i] replaces f[i] in staging
  Fe<P> s = t + 1 < KZG_TPB ? v[t + 1] : carry;
#pragma unroll
  for (int e = KZG_E - 1; e >= 0; e--) {
    s = fe_add(stage_get<P>(stage, t, e), fe_mul(s, z));
    stage_put<P>(stage, t, e, s);
  }
  __syncthreads();
  uint4* dst = reinterpret_cast<uint4*>(q);
#pragma unroll
  for (int r = 0; r < 2 * KZG_E; r++) {
    const int u = r * KZG_TPB + t;
    const int e = u >> 1;
    const size_t g = base + e;
    if (g >= 1 && g < m)
      dst[2 * (g - 1) + (u & 1)] = stage[(e >> KZG_E_LOG) * KZG_RUN_U4 + (e & (KZG_E - 1)) * 2 + (u & 1)];
  }
}

// out[j] = sum_i gamma^i f_i[j], j < n: Horner in gamma from the last polynomial
// down; a polynomial that ends at or before j adds nothing.
template <class P>
__global__ void __launch_bounds__(256) k_poly_fold(const PolyRef* __restrict__ polys, size_t k, size_t n,
                                                   FeG<P> gamma, void* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const Fe<P> g = fe_unpack<P>(gamma);
  Fe<P> acc = fe_zero<P>();
  for (size_t i = k; i-- > 0;) {
    const PolyRef pr = polys[i];
    if (i + 1 < k) acc = fe_mul(acc, g);
    if (j < pr.len) acc = fe_add(acc, fe_load_g<P>(pr.p, j));
  }
  fe_store_g<P>(out, j, acc);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <class C>
static PolyPoint<typename C::Fr> make_point(const void* z_host) {
  host::F<typename C::HFr> p;
  memcpy(p.v, z_host, sizeof(p.v));
  PolyPoint<typename C::Fr> pt;
  pt.z = to_internal_words<C>(p);
  for (int i = 0; i < KZG_E_LOG; i++) p = p * p;
  for (int d = 0; d < KZG_NPOW; d++) {
    pt.pw[d] = to_internal_words<C>(p);
    p = p * p;
  }
  return pt;
}

static int check_polys(const void* const* polys, const size_t* lens, size_t k, const char* what) {
  if (!polys || !lens || k == 0) {
    set_error(std::string(what) + ": no polynomials");
    return GM_ERR_INVALID;
  }
  for (size_t i = 0; i < k; i++)
    if (lens[i] && (!polys[i] || (uintptr_t)polys[i] % 16)) {
      set_error(std::string(what) + ": polynomial pointers must be non-null and 16-byte aligned");
      return GM_ERR_INVALID;
    }
  return GM_OK;
}

// Chunk sums and their scan for k polynomials: vals[i] = f_i(z) (k gnark
// elements), chunks[refs[i].off + j] = s_i[j C].  refs is the host copy of the
// uploaded table; it has to outlive the copy (the caller synchronises).
template <class C>
static int eval_launch(gm_ctx* ctx, Arena& arena, const void* const* polys, const size_t* lens, size_t k,
                       const PolyPoint<typename C::Fr>& pt, std::vector<PolyRef>& refs, DevBuf& chunks,
                       DevBuf& vals) {
  using Fr = typename C::Fr;
  refs.resize(k);
  size_t total = 0;
  for (size_t i = 0; i < k; i++) {
    refs[i] = {polys[i], lens[i], total};
    total += (lens[i] + KZG_C - 1) / KZG_C;
  }
  DevBuf tab;
  int rc;
  if ((rc = tab.alloc(arena, k * sizeof(PolyRef)))) return rc;
  if ((rc = chunks.alloc(arena, 32 * total))) return rc;
  if ((rc = vals.alloc(arena, 32 * k))) return rc;
  GM_HIP(hipMemcpyAsync(tab.p, refs.data(), k * sizeof(PolyRef), hipMemcpyHostToDevice, ctx->stream));
  for (size_t b0 = 0; b0 < k; b0 += KZG_MAX_GRID_Y) {
    const size_t nb = std::min<size_t>(KZG_MAX_GRID_Y, k - b0);
    size_t maxc = 0;
    for (size_t i = b0; i < b0 + nb; i++) maxc = std::max(maxc, (lens[i] + KZG_C - 1) / KZG_C);
    if (maxc >= (size_t(1) << 31)) {
      set_error("kzg: polynomial too long");
      return GM_ERR_INVALID;
    }
    if (maxc) {
      ProfScope ps(ctx, "kzg_chunk_eval");
      hipLaunchKernelGGL(k_poly_chunk_eval<Fr>, dim3((unsigned)maxc, (unsigned)nb), dim3(KZG_TPB), 0, ctx->stream,
                         tab.as<PolyRef>() + b0, pt, chunks.p);
      GM_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, "kzg_chunk_carry");
    hipLaunchKernelGGL(k_poly_chunk_carry<Fr>, dim3((unsigned)nb), dim3(KZG_TPB), 0, ctx->stream,
                       tab.as<PolyRef>() + b0, pt, chunks.p, (void*)(vals.as<char>() + 32 * b0));
    GM_HIP(hipGetLastError());
  }
  return GM_OK;
}

template <class C>
int poly_eval_device(gm_ctx* ctx, const void* const* polys, const size_t* lens, size_t k, const void* z_host,
                     void* values_host) {
  if (int rc = check_polys(polys, lens, k, "kzg eval")) return rc;
  const auto pt = make_point<C>(z_host);
  Arena arena(ctx);
  std::vector<PolyRef> refs;
  DevBuf chunks, vals;
  if (int rc = eval_launch<C>(ctx, arena, polys, lens, k, pt, refs, chunks, vals)) return rc;
  GM_HIP(hipMemcpyAsync(values_host, vals.p, 32 * k, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

template <class C>
int poly_div_linear_device(gm_ctx* ctx, const void* f, size_t m, const void* z_host, void* q, void* value_host) {
  using Fr = typename C::Fr;
  if (m == 0) {
    set_error("poly div: empty polynomial");
    return GM_ERR_INVALID;
  }
  if (int rc = check_polys(&f, &m, 1, "poly div")) return rc;
  if (m > 1) {
    if (!q || (uintptr_t)q % 16) {
      set_error("poly div: the quotient pointer must be non-null and 16-byte aligned");
      return GM_ERR_INVALID;
    }
    const uintptr_t f0 = (uintptr_t)f, f1 = f0 + 32 * m, q0 = (uintptr_t)q, q1 = q0 + 32 * (m - 1);
    if (q0 < f1 && f0 < q1) {
      set_error("poly div: the quotient must not overlap the polynomial");
      return GM_ERR_INVALID;
    }
  }
  const auto pt = make_point<C>(z_host);
  Arena arena(ctx);
  std::vector<PolyRef> refs;
  DevBuf chunks, vals;
  if (int rc = eval_launch<C>(ctx, arena, &f, &m, 1, pt, refs, chunks, vals)) return rc;
  if (m > 1) {
    ProfScope ps(ctx, "kzg_div_write");
    hipLaunchKernelGGL(k_poly_div_write<Fr>, dim3((unsigned)((m + KZG_C - 1) / KZG_C)), dim3(KZG_TPB), 0,
                       ctx->stream, f, m, pt, (const void*)chunks.p, q);
    GM_HIP(hipGetLastError());
  }
  GM_HIP(hipMemcpyAsync(value_host, vals.p, 32, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

template <class C>
int poly_fold_device(gm_ctx* ctx, const void* const* polys, const size_t* lens, size_t k, const void* gamma_host,
                     void* out) {
  using Fr = typename C::Fr;
  if (int rc = check_polys(polys, lens, k, "poly fold")) return rc;
  size_t n = 0;
  std::vector<PolyRef> refs(k);
  for (size_t i = 0; i < k; i++) {
    refs[i] = {polys[i], lens[i], 0};
    n = std::max(n, lens[i]);
  }
  if (n == 0) return GM_OK;
  if (!out || (uintptr_t)out % 16) {
    set_error("poly fold: the output pointer must be non-null and 16-byte aligned");
    return GM_ERR_INVALID;
  }
  host::F<typename C::HFr> g;
  memcpy(g.v, gamma_host, sizeof(g.v));
  Arena arena(ctx);
  DevBuf tab;
  if (int rc = tab.alloc(arena, k * sizeof(PolyRef))) return rc;
  GM_HIP(hipMemcpyAsync(tab.p, refs.data(), k * sizeof(PolyRef), hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, "kzg_fold");
    hipLaunchKernelGGL(k_poly_fold<Fr>, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, tab.as<PolyRef>(), k,
                       n, to_internal_words<C>(g), out);
    GM_HIP(hipGetLastError());
  }
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

#define GM_KZG_INST(C)                                                                                       \
  template int poly_eval_device<C>(gm_ctx*, const void* const*, const size_t*, size_t, const void*, void*);  \
  template int poly_div_linear_device<C>(gm_ctx*, const void*, size_t, const void*, void*, void*);           \
  template int poly_fold_device<C>(gm_ctx*, const void* const*, const size_t*, size_t, const void*, void*);
GM_KZG_INST(CurveBN254)
GM_KZG_INST(CurveBLS12377)
GM_KZG_INST(CurveBLS12381)

}  // namespace gm
