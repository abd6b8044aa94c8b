// Groth16 setup on the device: fixed-base batch scalar multiplication, and below
// it the scalar side of Setup over the resident R1CS ("The scalar side of Setup").
//
// gnark's Setup turns five vectors of scalars into points of one base each
// (curve.BatchScalarMultiplicationG1/G2, backend/groth16/bn254/setup.go:239-275, 318-330).
// gm_batch_mul_base does that with a double-and-add chain and a Fermat inversion
// per lane; here the doublings move into a table that all lanes share, and the
// inversions into one per block.
//
//  * Table.  W = ceil((FR_BITS + 1) / c) signed-digit windows of c bits;
//    T[w][d - 1] = [d 2^(c w)] base for 1 <= d <= 2^(c-1), affine in the packed
//    internal form (gnark's size: 64 B for BN254 G1, 192 B for BLS12-377 G2), built
//    in the call's workspace.  The W window bases [2^(c w)] base come from the host
//    (host_arith.hpp: c doublings each, W affine conversions); a lane per entry
//    multiplies its window base by d (xyzz_mul_small, at most c - 1 doublings and
//    additions) and the entries are normalised like the results below.
//
//  * Multiply.  One scalar per lane: the canonical scalar is recoded from the
//    low window up into digits in [-2^(c-1), 2^(c-1)] with a carry, and each
//    non-zero digit is one mixed addition of the gathered entry: W additions, no
//    doubling.  The additions are the complete ones (curve.hpp): with low-to-high
//    accumulation the sum of the lower windows can equal the top window's addend
//    (k = 2 d 2^(c (W-1)) - r), which takes the doubling branch.  G1 runs the
//    lazily reduced addition under its stated bounds, G2 the canonical one.
//
//  * Normalisation.  x = X / ZZ, y = Y / ZZZ by Montgomery's trick per block
//    (g16_setup.hpp): the multiply stores its XYZZ sums and one product of
//    zz zzz per block (infinity contributes 1), a second launch inverts the block
//    products one per lane, a third walks each block's product tree back and
//    writes affine points.  The scratch is bounded by working through the
//    scalars in chunks of FB_CHUNK.
//
// Window model.  cost(c) = W (n + 2^(c-1) FB_ENTRY_COST c) in mixed additions: n W
// for the multiply, and per table entry its short double-and-add on the general
// formulas plus its share of the normalisation, about FB_ENTRY_COST c mixed
// additions.  c is the minimum over [FB_MODEL_C_MIN, FIXED_BASE_C_MAX]; the cap
// keeps the table (32 MiB for BN254 G1 and 96 MiB for BLS12-377 G2 at c = 16)
// well inside the 256 MiB Infinity Cache.
#include <cstring>
#include <string>
#include <vector>

#include "curves.hpp"
#include "g16_setup.hpp"
#include "groth16.hpp"
#include "ntt.hpp"
#include "runtime.hpp"
#include "scan.hpp"

namespace gm {

namespace {

constexpr int FB_MODEL_C_MIN = 4;
// measured at n = 2^20, c = 16 (profiles/g16_setup_timing.json): a table entry costs
// 1.6 c (G2) to 2.4 c (BN254 G1) of the multiply kernel's additions
constexpr double FB_ENTRY_COST = 2.0;
// scalars per pass: bounds the XYZZ scratch (448 B per BLS12-377 G2 point)
constexpr size_t FB_CHUNK = size_t(1) << 22;

// lanes per block: the product tree takes 2 TPB elements of LDS (at most 28 KiB)
template <class F>
constexpr unsigned fb_tpb() {
  return sizeof(F) > 64 ? 128 : 256;
}

// acc += (neg ? -p : p), complete
template <class P>
GM_DEV void fb_add(XYZZ<Fe<P>>& acc, const Affine<Fe<P>>& p, bool neg) {
  xyzz_add_aff_lz<P>(acc, p, neg);
}
template <class P, int B>
GM_DEV void fb_add(XYZZ<Fe2<P, B>>& acc, Affine<Fe2<P, B>> p, bool neg) {
  if (neg) p.y = fe_neg(p.y);
  xyzz_add_aff(acc, p);
}
// canonical coordinates of what fb_add leaves
template <class P>
GM_DEV XYZZ<Fe<P>> fb_canon(const XYZZ<Fe<P>>& a) {
  return xyzz_canon_raw(a);
}
template <class P, int B>
GM_DEV XYZZ<Fe2<P, B>> fb_canon(const XYZZ<Fe2<P, B>>& a) {
  return a;
}

// The tail of the two kernels that produce points: lane i < n stores its canonical
// XYZZ sum, and the block stores the product of its lanes' zz zzz (1 for
// infinity and for lanes past n).
template <class F>
GM_DEV void fb_emit(size_t i, size_t n, const XYZZ<F>& acc, XYZZ<F>* __restrict__ sums, F* __restrict__ bprod,
                    F* __restrict__ tree) {
  F d = FOps<F>::one();
  if (i < n) {
    sums[i] = acc;
    if (!xyzz_is_inf(acc)) d = fe_mul(acc.zz, acc.zzz);
  }
  const F root = block_product<F, fb_tpb<F>()>(d, tree);
  if (threadIdx.x == 0) bprod[blockIdx.x] = root;
}

// entry e = w 2^(c-1) + d - 1 of the table, as an XYZZ point: [d] bases[w]
template <class F>
__global__ void __launch_bounds__(fb_tpb<F>())
    k_fb_table(const uint32_t* __restrict__ bases, uint32_t c, size_t entries, XYZZ<F>* __restrict__ sums,
               F* __restrict__ bprod) {
  constexpr unsigned TPB = fb_tpb<F>();
  __shared__ F tree[2 * TPB];
  const size_t e = (size_t)blockIdx.x * TPB + threadIdx.x;
  XYZZ<F> acc = xyzz_inf<F>();
  if (e < entries) {
    const uint32_t w = (uint32_t)(e >> (c - 1));
    const uint32_t d = ((uint32_t)e & ((1u << (c - 1)) - 1)) + 1;
    const Affine<F> b = load_affine_gnark<F>(bases + (size_t)w * 2 * Coord<F>::WORDS);
    if (!aff_is_inf(b)) {
      XYZZ<F> p;
      p.x = b.x;
      p.y = b.y;
      p.zz = FOps<F>::one();
      p.zzz = FOps<F>::one();
      acc = xyzz_mul_small(p, d);
    }
  }
  fb_emit<F>(e, entries, acc, sums, bprod, tree);
}

// sums[i] = [k_i] base for the scalars [0, n) of this pass
template <class Fr, class F>
__global__ void __launch_bounds__(fb_tpb<F>())
    k_fb_mul(const uint32_t* __restrict__ scalars, size_t n, const uint32_t* __restrict__ table, uint32_t c,
             uint32_t W, XYZZ<F>* __restrict__ sums, F* __restrict__ bprod) {
  static_assert(Fr::NG == 8, "scalars of 8 u32 words");
  constexpr unsigned TPB = fb_tpb<F>();
  constexpr size_t PW = 2 * Coord<F>::WORDS;
  __shared__ F tree[2 * TPB];
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  XYZZ<F> acc = xyzz_inf<F>();
  if (i < n) {
    FeG<Fr> k = fe_pack(fe_gnark_to_canonical(fe_load_g<Fr>(scalars, i)));
    const uint32_t mask = (1u << c) - 1, half = 1u << (c - 1);
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t w = 0; w < W; w++) {
      // k < 2^FR_BITS and W c > FR_BITS: the top window's raw digit stays <= 2^(c-1)
      const uint32_t raw = (k.w[0] & mask) + carry;
#pragma unroll
      for (int q = 0; q < 7; q++) k.w[q] = (k.w[q] >> c) | (k.w[q + 1] << (32 - c));
      k.w[7] >>= c;
      carry = raw > half;
      const uint32_t d = carry ? (1u << c) - raw : raw;
      if (d) fb_add(acc, load_affine_packed<F>(table + (((size_t)w << (c - 1)) + d - 1) * PW), carry != 0);
    }
    acc = fb_canon(acc);
  }
  fb_emit<F>(i, n, acc, sums, bprod, tree);
}

template <class F>
__global__ void __launch_bounds__(256) k_fb_invert(F* __restrict__ bprod, size_t nb) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) bprod[i] = fe_inv(bprod[i]);
}

// out[i] = sums[i] in affine form: gnark layout, or the packed internal one of
// the table (PACKED); infinity is (0, 0) in both
template <class F, bool PACKED>
__global__ void __launch_bounds__(fb_tpb<F>())
    k_fb_affine(const XYZZ<F>* __restrict__ sums, size_t n, const F* __restrict__ binv, uint32_t* __restrict__ out) {
  constexpr unsigned TPB = fb_tpb<F>();
  __shared__ F tree[2 * TPB];
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  XYZZ<F> a = xyzz_inf<F>();
  if (i < n) a = sums[i];
  const bool inf = xyzz_is_inf(a);
  const F d = inf ? FOps<F>::one() : fe_mul(a.zz, a.zzz);
  const F t = block_inverse<F, TPB>(d, binv[blockIdx.x], tree);
  if (i >= n) return;
  Affine<F> r;
  if (inf) {
    r.x = FOps<F>::zero();
    r.y = FOps<F>::zero();
  } else {
    r.x = fe_mul(a.x, fe_mul(t, a.zzz));  // X / ZZ
    r.y = fe_mul(a.y, fe_mul(t, a.zz));   // Y / ZZZ
  }
  uint32_t* const dst = out + i * 2 * Coord<F>::WORDS;
  if constexpr (PACKED)
    store_affine_packed<F>(dst, r);
  else
    store_affine_gnark<F>(dst, r);
}

// nothing queued may outlive the call's workspace, also after a failure
struct StreamDrain {
  gm_ctx* ctx;
  ~StreamDrain() {
    hipStreamSynchronize(ctx->stream);
    prof_collect(ctx);
  }
};

// launches 2 and 3 of the normalisation over the m sums of the last producer
template <class F, bool PACKED>
int fb_normalise(gm_ctx* ctx, const XYZZ<F>* sums, size_t m, F* bprod, void* out) {
  constexpr unsigned TPB = fb_tpb<F>();
  const unsigned nb = blocks_for(m, TPB);
  hipLaunchKernelGGL(k_fb_invert<F>, dim3(blocks_for(nb, 256)), dim3(256), 0, ctx->stream, bprod, (size_t)nb);
  hipLaunchKernelGGL((k_fb_affine<F, PACKED>), dim3(nb), dim3(TPB), 0, ctx->stream, sums, m, (const F*)bprod,
                     (uint32_t*)out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // namespace

int fixed_base_window(const gm_ctx* ctx, size_t n, int bits) {
  if (ctx && ctx->fixed_base_c > 0) return ctx->fixed_base_c;
  int best = FB_MODEL_C_MIN;
  double best_cost = 0;
  for (int c = FB_MODEL_C_MIN; c <= FIXED_BASE_C_MAX; c++) {
    const double W = (double)((bits + 1 + c - 1) / c);
    const double cost = W * ((double)n + (double)(size_t(1) << (c - 1)) * FB_ENTRY_COST * c);
    if (c == FB_MODEL_C_MIN || cost < best_cost) {
      best = c;
      best_cost = cost;
    }
  }
  return best;
}

template <class C, bool G2>
int batch_mul_fixed_device(gm_ctx* ctx, const void* base_affine_host, const void* scalars_dev, size_t n,
                           void* out_dev) {
  using F = typename GroupSel<C, G2>::DF;
  using HF = typename GroupSel<C, G2>::HF;
  using Fr = typename C::Fr;
  constexpr unsigned TPB = fb_tpb<F>();
  constexpr size_t pb = sizeof(host::Aff<HF>);
  static_assert(pb == 2 * Coord<F>::WORDS * sizeof(uint32_t), "gnark layout");
  if (n == 0) return GM_OK;
  host::Aff<HF> base;
  memcpy(&base, base_affine_host, pb);
  if (base.is_inf()) {
    GM_HIP(hipMemsetAsync(out_dev, 0, pb * n, ctx->stream));
    GM_HIP(hipStreamSynchronize(ctx->stream));
    return GM_OK;
  }
  const uint32_t c = (uint32_t)fixed_base_window(ctx, n, C::FR_BITS);
  const uint32_t W = (C::FR_BITS + 1 + c - 1) / c;
  const size_t entries = (size_t)W << (c - 1);
  // the window bases [2^(c w)] base
  std::vector<host::Aff<HF>> bases(W);
  host::Jac<HF> run = host::to_jac(base);
  for (uint32_t w = 0; w < W; w++) {
    bases[w] = host::to_aff(run);
    if (w + 1 < W)
      for (uint32_t b = 0; b < c; b++) run = host::jdbl(run);
  }
  const size_t pass = std::min(n, FB_CHUNK), most = std::max(pass, entries);
  int rc;
  Arena arena(ctx);
  DevBuf table, bases_dev, sums, bprod;
  if ((rc = table.alloc(arena, pb * entries))) return rc;
  if ((rc = bases_dev.alloc(arena, pb * W))) return rc;
  if ((rc = sums.alloc(arena, sizeof(XYZZ<F>) * most))) return rc;
  if ((rc = bprod.alloc(arena, sizeof(F) * blocks_for(most, TPB)))) return rc;
  StreamDrain drain{ctx};  // destroyed before the arena
  GM_HIP(hipMemcpyAsync(bases_dev.p, bases.data(), pb * W, hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, "fixed_base_table");
    hipLaunchKernelGGL(k_fb_table<F>, dim3(blocks_for(entries, TPB)), dim3(TPB), 0, ctx->stream,
                       bases_dev.as<uint32_t>(), c, entries, sums.as<XYZZ<F>>(), bprod.as<F>());
    if ((rc = fb_normalise<F, true>(ctx, sums.as<XYZZ<F>>(), entries, bprod.as<F>(), table.p))) return rc;
  }
  for (size_t lo = 0; lo < n; lo += pass) {
    const size_t m = std::min(pass, n - lo);
    {
      ProfScope ps(ctx, "fixed_base_mul");
      hipLaunchKernelGGL((k_fb_mul<Fr, F>), dim3(blocks_for(m, TPB)), dim3(TPB), 0, ctx->stream,
                         (const uint32_t*)scalars_dev + lo * Fr::NG, m, table.as<uint32_t>(), c, W,
                         sums.as<XYZZ<F>>(), bprod.as<F>());
    }
    ProfScope ps(ctx, "fixed_base_normalise");
    if ((rc = fb_normalise<F, false>(ctx, sums.as<XYZZ<F>>(), m, bprod.as<F>(), (char*)out_dev + lo * pb)))
      return rc;
  }
  return GM_OK;
}

#define GM_FB_INST(C, G2) \
  template int batch_mul_fixed_device<C, G2>(gm_ctx*, const void*, const void*, size_t, void*);
GM_FB_INST(CurveBN254, false)
GM_FB_INST(CurveBN254, true)
GM_FB_INST(CurveBLS12377, false)
GM_FB_INST(CurveBLS12377, true)

// ===========================================================================
// The scalar side of Setup (setup.go:120-237, setupABC :364-445)
// ===========================================================================
//
//  * L_j(tau) = w^j (tau^n - 1) / (n (tau - w^j)), j < nb_constraints: the powers
//    per lane, the denominators inverted by the block-wise batch inversion.
//  * A_w = sum coeff L_row over the terms of matrix L whose wire is w (B over R,
//    C over O).  The resident form is CSR by row, so each matrix is transposed:
//    a histogram of wire ids, an exclusive scan, a scatter of (row, coeff id).
//    The order inside a column is whatever the scatter's atomics gave; the sums
//    are canonical field values, so the bytes do not depend on it.  Three
//    classes by column length: up to COL_SHORT terms one lane; up to the cut one
//    block with an LDS tree; above it pieces of `cut` terms, one block each, and
//    a second launch that adds a column's pieces.
//  * InfinityA / InfinityB from exact zero tests; A, B compacted by flag, scan,
//    scatter.  K over host-made wire lists (the key's side by 1/delta, the
//    verifier's by 1/gamma).  Z_i = tau^i (tau^n - 1) / delta, bit-reversed.
namespace {

constexpr uint32_t COL_SHORT = 32;
constexpr uint32_t COL_CUT_DEFAULT = 1u << 14;
constexpr unsigned COL_TPB = 256;
// the documented limit of gm_g16_setup: wires, constraints
constexpr size_t SETUP_MAX = (size_t)1 << 25;

// ---- Lagrange values ---------------------------------------------------------
// lane j: wj[j] = w^j (gnark form), den[j] = tau - w^j (internal form), and the
// block's product of denominators
template <class Fr>
__global__ void __launch_bounds__(256)
    k_lag_den(size_t nc, FeG<Fr> omega, FeG<Fr> tau, uint32_t* __restrict__ wj, Fe<Fr>* __restrict__ den,
              Fe<Fr>* __restrict__ bprod) {
  __shared__ Fe<Fr> tree[2 * 256];
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  Fe<Fr> d = fe_one<Fr>();
  if (j < nc) {
    const Fe<Fr> w = fe_pow(fe_to_internal(fe_unpack<Fr>(omega)), j);
    d = fe_sub(fe_to_internal(fe_unpack<Fr>(tau)), w);
    fe_store_g<Fr>(wj, j, fe_to_gnark(w));
    den[j] = d;
  }
  const Fe<Fr> root = block_product<Fe<Fr>, 256>(d, tree);
  if (threadIdx.x == 0) bprod[blockIdx.x] = root;
}
// lag[j] = wj[j] scale / den[j] (gnark form, in place over wj); scale = (tau^n - 1) / n
template <class Fr>
__global__ void __launch_bounds__(256)
    k_lag_apply(size_t nc, FeG<Fr> scale, const Fe<Fr>* __restrict__ den, const Fe<Fr>* __restrict__ binv,
                uint32_t* __restrict__ lag) {
  __shared__ Fe<Fr> tree[2 * 256];
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const Fe<Fr> d = j < nc ? den[j] : fe_one<Fr>();
  const Fe<Fr> inv = block_inverse<Fe<Fr>, 256>(d, binv[blockIdx.x], tree);
  if (j >= nc) return;
  const Fe<Fr> ws = fe_mul(fe_load_g<Fr>(lag, j), fe_to_internal(fe_unpack<Fr>(scale)));
  fe_store_g<Fr>(lag, j, fe_mul(ws, inv));
}

// ---- transpose ---------------------------------------------------------------
__global__ void __launch_bounds__(256)
    k_col_hist(const uint32_t* __restrict__ vid, size_t nnz, uint32_t* __restrict__ counts) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nnz) atomicAdd(&counts[vid[q]], 1u);
}
__global__ void __launch_bounds__(256)
    k_col_scatter(const uint32_t* __restrict__ rowptr, size_t nc, const uint32_t* __restrict__ cid,
                  const uint32_t* __restrict__ vid, uint32_t* __restrict__ cursor, uint32_t* __restrict__ trow,
                  uint32_t* __restrict__ tcid) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  for (uint32_t q = rowptr[i]; q < rowptr[i + 1]; q++) {
    const uint32_t pos = atomicAdd(&cursor[vid[q]], 1u);
    trow[pos] = (uint32_t)i;
    tcid[pos] = cid[q];
  }
}

// one term: coeff * L_row in gnark form (CoeffTable ids 0 and 1 as k_r1cs_eval has them)
template <class Fr>
GM_DEV Fe<Fr> col_term(uint32_t row, uint32_t k, const uint32_t* __restrict__ lag, const Fe<Fr>* __restrict__ ci) {
  if (k == 0) return fe_zero<Fr>();
  const Fe<Fr> l = fe_load_g<Fr>(lag, row);
  return k == 1 ? l : fe_mul(l, ci[k]);
}
template <class Fr>
GM_DEV Fe<Fr> block_sum(Fe<Fr> v, Fe<Fr>* __restrict__ tree) {
  const unsigned t = threadIdx.x;
  tree[t] = v;
  __syncthreads();
  for (unsigned s = COL_TPB / 2; s >= 1; s >>= 1) {
    if (t < s) tree[t] = fe_add(tree[t], tree[t + s]);
    __syncthreads();
  }
  return tree[0];
}

// lane per wire: a short column is summed here, a longer one is listed as
// (wire, start, length)
template <class Fr>
__global__ void __launch_bounds__(256)
    k_col_short(const uint32_t* __restrict__ colptr, size_t nb_wires, const uint32_t* __restrict__ trow,
                const uint32_t* __restrict__ tcid, const uint32_t* __restrict__ lag,
                const Fe<Fr>* __restrict__ ci, uint32_t* __restrict__ out, uint32_t* __restrict__ long_list,
                uint32_t* __restrict__ long_count, uint32_t long_cap) {
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nb_wires) return;
  const uint32_t lo = colptr[w], hi = colptr[w + 1];
  if (hi - lo > COL_SHORT) {
    const uint32_t k = atomicAdd(long_count, 1u);
    if (k < long_cap) {
      long_list[3 * k] = (uint32_t)w;
      long_list[3 * k + 1] = lo;
      long_list[3 * k + 2] = hi - lo;
    }
    return;
  }
  Fe<Fr> acc = fe_zero<Fr>();
  for (uint32_t q = lo; q < hi; q++) acc = fe_add(acc, col_term<Fr>(trow[q], tcid[q], lag, ci));
  fe_store_g<Fr>(out, w, acc);
}
// block per piece (start, length, destination element of dst)
struct ColPiece {
  uint32_t start, len, dst, to_part;
};
template <class Fr>
__global__ void __launch_bounds__(COL_TPB)
    k_col_piece(const ColPiece* __restrict__ pieces, const uint32_t* __restrict__ trow,
                const uint32_t* __restrict__ tcid, const uint32_t* __restrict__ lag, const Fe<Fr>* __restrict__ ci,
                uint32_t* __restrict__ out, uint32_t* __restrict__ parts) {
  __shared__ Fe<Fr> tree[COL_TPB];
  const ColPiece p = pieces[blockIdx.x];
  Fe<Fr> acc = fe_zero<Fr>();
  for (uint32_t q = threadIdx.x; q < p.len; q += COL_TPB)
    acc = fe_add(acc, col_term<Fr>(trow[p.start + q], tcid[p.start + q], lag, ci));
  const Fe<Fr> sum = block_sum<Fr>(acc, tree);
  if (threadIdx.x == 0) fe_store_g<Fr>(p.to_part ? parts : out, p.dst, sum);
}
// block per column of several pieces: out[wire] = sum of parts[first, first + count)
struct ColMerge {
  uint32_t wire, first, count;
};
template <class Fr>
__global__ void __launch_bounds__(COL_TPB)
    k_col_merge(const ColMerge* __restrict__ cols, const uint32_t* __restrict__ parts, uint32_t* __restrict__ out) {
  __shared__ Fe<Fr> tree[COL_TPB];
  const ColMerge c = cols[blockIdx.x];
  Fe<Fr> acc = fe_zero<Fr>();
  for (uint32_t q = threadIdx.x; q < c.count; q += COL_TPB) acc = fe_add(acc, fe_load_g<Fr>(parts, c.first + q));
  const Fe<Fr> sum = block_sum<Fr>(acc, tree);
  if (threadIdx.x == 0) fe_store_g<Fr>(out, c.wire, sum);
}

// ---- infinity flags and compaction ---------------------------------------------
// gnark-form zero is the all-zero word pattern (values are fully reduced)
__global__ void __launch_bounds__(256)
    k_zero_flags(const uint4* __restrict__ v, size_t n, uint8_t* __restrict__ inf, uint32_t* __restrict__ keep) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 a = v[2 * i], b = v[2 * i + 1];
  const bool z = (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0;
  inf[i] = z ? 1 : 0;
  keep[i] = z ? 0u : 1u;
}
__global__ void __launch_bounds__(256)
    k_compact(const uint4* __restrict__ v, size_t n, const uint32_t* __restrict__ keep,
              const uint32_t* __restrict__ pos, uint4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !keep[i]) return;
  out[2 * (size_t)pos[i]] = v[2 * i];
  out[2 * (size_t)pos[i] + 1] = v[2 * i + 1];
}

// ---- K and Z ---------------------------------------------------------------------
// out[i] = (beta A_w + alpha B_w + C_w) scale for w = wires[i]
template <class Fr>
__global__ void __launch_bounds__(256)
    k_setup_k(const uint32_t* __restrict__ wires, size_t count, const uint32_t* __restrict__ A,
              const uint32_t* __restrict__ B, const uint32_t* __restrict__ Cc, FeG<Fr> alpha, FeG<Fr> beta,
              FeG<Fr> scale, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const size_t w = wires[i];
  Fe<Fr> v = fe_mul(fe_load_g<Fr>(A, w), fe_to_internal(fe_unpack<Fr>(beta)));
  v = fe_add(v, fe_mul(fe_load_g<Fr>(B, w), fe_to_internal(fe_unpack<Fr>(alpha))));
  v = fe_add(v, fe_load_g<Fr>(Cc, w));
  fe_store_g<Fr>(out, i, fe_mul(v, fe_to_internal(fe_unpack<Fr>(scale))));
}
// out[i] = tau^brev(i) scale, i < n - 1; scale = (tau^n - 1) / delta
template <class Fr>
__global__ void __launch_bounds__(256)
    k_setup_z(size_t n, uint32_t logn, FeG<Fr> tau, FeG<Fr> scale, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 >= n) return;
  const size_t src = brev_bits((uint32_t)i, (int)logn);  // n <= SETUP_MAX
  const Fe<Fr> p = fe_pow(fe_to_internal(fe_unpack<Fr>(tau)), src);
  fe_store_g<Fr>(out, i, fe_mul(fe_unpack<Fr>(scale), p));
}

int refuse_setup(const char* entry, const std::string& msg) {
  set_error(std::string(entry) + ": " + msg);
  return GM_ERR_INVALID;
}

template <class HF, class Fr>
FeG<Fr> to_dev(const HF& h) {
  FeG<Fr> r;
  static_assert(sizeof(r.w) == sizeof(h.v), "gnark layout");
  memcpy(r.w, h.v, sizeof(r.w));
  return r;
}

// what the host derives from the inputs, after judging them
template <class C>
struct SetupHost {
  using HF = host::F<typename C::HFr>;
  size_t n = 1;
  int logn = 0;
  HF tau, alpha, beta, gamma, delta, omega, lag_scale, z_scale, dinv, ginv;
  std::vector<uint32_t> k_wires, g_wires;
};

template <class C>
int setup_judge(const char* entry, const gm_r1cs* r, const gm_g16_setup_in* in, SetupHost<C>& h) {
  using HF = typename SetupHost<C>::HF;
  if (!in->toxic) return refuse_setup(entry, "the toxic scalars are NULL");
  if (r->has_const) return refuse_setup(entry, "the R1CS has a constant term (GM_R1CS_CONST), which gnark's never has");
  if (r->nb_wires == 0) return refuse_setup(entry, "the R1CS has no wire");
  if (in->nb_public > r->nb_wires) return refuse_setup(entry, "nb_public exceeds nb_wires");
  if (in->nb_gamma && !in->gamma_wires) return refuse_setup(entry, "nb_gamma > 0 needs gamma_wires");
  for (size_t i = 0; i < in->nb_gamma; i++) {
    const uint32_t w = in->gamma_wires[i];
    if (w < in->nb_public || w >= r->nb_wires || (i && w <= in->gamma_wires[i - 1]))
      return refuse_setup(entry, "gamma_wires[" + std::to_string(i) + "] = " + std::to_string(w) +
                                     " is not strictly increasing inside [nb_public, nb_wires)");
  }
  HF t[5];
  memcpy(t, in->toxic, sizeof(t));
  h.tau = t[0], h.alpha = t[1], h.beta = t[2], h.gamma = t[3], h.delta = t[4];
  if (h.delta.is_zero()) return refuse_setup(entry, "delta is zero");
  if (h.gamma.is_zero()) return refuse_setup(entry, "gamma is zero");
  while (h.n < r->nc) h.n <<= 1, h.logn++;
  if (r->nb_wires + 1 > SETUP_MAX || h.n > SETUP_MAX)
    return refuse_setup(entry, "more than 2^25 wires or constraints");
  h.omega = HF::one();
  if (h.logn)
    if (int rc = ntt_root<C>(h.logn, h.omega.v)) return rc;
  HF tn = h.tau;
  for (int i = 0; i < h.logn; i++) tn = tn * tn;
  const HF tn1 = tn - HF::one();
  if (tn1.is_zero()) return refuse_setup(entry, "tau^n = 1: the Lagrange formula divides by zero");
  h.dinv = host::finv(h.delta);
  h.ginv = host::finv(h.gamma);
  h.lag_scale = tn1 * host::finv(host::from_u64<typename C::HFr>(h.n));
  h.z_scale = tn1 * h.dinv;
  // the verifier's side: the public wires, then gamma_wires; the key's K: the rest
  size_t g = 0;
  for (size_t w = 0; w < r->nb_wires; w++) {
    const bool listed = g < in->nb_gamma && in->gamma_wires[g] == w;
    if (listed) g++;
    if (w < in->nb_public || listed)
      h.g_wires.push_back((uint32_t)w);
    else
      h.k_wires.push_back((uint32_t)w);
  }
  return GM_OK;
}

// the scalar vectors, in the caller's arena
struct SetupScalars {
  size_t nbA = 0, nbB = 0;
  DevBuf sum[3];            // A_w, B_w, C_w: nb_wires Fr each
  DevBuf inf[2];            // InfinityA, InfinityB: nb_wires bytes each
  DevBuf compact[2];        // the non-zero A_w and B_w in wire order
  DevBuf k, kg, z, kw, gw;  // K, the verifier's K, Z; the two wire lists
};

template <class C>
int column_sums(gm_ctx* ctx, Arena& arena, const gm_r1cs* r, int m, const uint32_t* lag, uint32_t* out) {
  using Fr = typename C::Fr;
  const size_t nw = r->nb_wires, nnz = r->nnz[m];
  const uint32_t cut = ctx->g16_column_cut > 0 ? (uint32_t)ctx->g16_column_cut : COL_CUT_DEFAULT;
  const uint32_t long_cap = (uint32_t)(nnz / (COL_SHORT + 1) + 1);
  int rc;
  DevBuf counts, colptr, cursor, bsum, trow, tcid, llist, lcount;
  if ((rc = counts.alloc(arena, 4 * (nw + 1))) || (rc = colptr.alloc(arena, 4 * (nw + 1))) ||
      (rc = cursor.alloc(arena, 4 * (nw + 1))) || (rc = bsum.alloc(arena, 4 * scan_ws_words(nw))) ||
      (rc = trow.alloc(arena, 4 * (nnz + 1))) || (rc = tcid.alloc(arena, 4 * (nnz + 1))) ||
      (rc = llist.alloc(arena, 12 * (size_t)long_cap)) || (rc = lcount.alloc(arena, 4)))
    return rc;
  {
    ProfScope ps(ctx, "g16_setup_transpose");
    GM_HIP(hipMemsetAsync(counts.p, 0, 4 * (nw + 1), ctx->stream));
    GM_HIP(hipMemsetAsync(lcount.p, 0, 4, ctx->stream));
    if (nnz)
      hipLaunchKernelGGL(k_col_hist, dim3(blocks_for(nnz, 256)), dim3(256), 0, ctx->stream, r->vid[m], nnz,
                         counts.as<uint32_t>());
    if ((rc = device_excl_scan(ctx, counts.as<uint32_t>(), nw, colptr.as<uint32_t>(), bsum.as<uint32_t>()))) return rc;
    GM_HIP(hipMemcpyAsync(cursor.p, colptr.p, 4 * (nw + 1), hipMemcpyDeviceToDevice, ctx->stream));
    if (r->nc)
      hipLaunchKernelGGL(k_col_scatter, dim3(blocks_for(r->nc, 256)), dim3(256), 0, ctx->stream, r->rowptr[m], r->nc,
                         r->cid[m], r->vid[m], cursor.as<uint32_t>(), trow.as<uint32_t>(), tcid.as<uint32_t>());
  }
  ProfScope ps(ctx, "g16_setup_columns");
  hipLaunchKernelGGL(k_col_short<Fr>, dim3(blocks_for(nw, 256)), dim3(256), 0, ctx->stream, colptr.as<uint32_t>(),
                     nw, trow.as<uint32_t>(), tcid.as<uint32_t>(), lag, (const Fe<Fr>*)r->coeff_i, out,
                     llist.as<uint32_t>(), lcount.as<uint32_t>(), long_cap);
  GM_HIP(hipGetLastError());
  uint32_t nlong = 0;
  GM_HIP(hipMemcpyAsync(&nlong, lcount.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  if (nlong == 0) return GM_OK;
  if (nlong > long_cap) return refuse_setup("g16 setup", "internal: long-column list overflow");
  std::vector<uint32_t> ll(3 * (size_t)nlong);
  GM_HIP(hipMemcpyAsync(ll.data(), llist.p, 12 * (size_t)nlong, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<ColPiece> pieces;
  std::vector<ColMerge> merges;
  uint32_t nparts = 0;
  for (uint32_t k = 0; k < nlong; k++) {
    const uint32_t w = ll[3 * k], start = ll[3 * k + 1], len = ll[3 * k + 2];
    if (len <= cut) {
      pieces.push_back({start, len, w, 0u});
      continue;
    }
    const uint32_t np = (len + cut - 1) / cut;
    merges.push_back({w, nparts, np});
    for (uint32_t q = 0; q < np; q++)
      pieces.push_back({start + q * cut, std::min(cut, len - q * cut), nparts + q, 1u});
    nparts += np;
  }
  DevBuf pdev, mdev, parts;
  if ((rc = pdev.alloc(arena, sizeof(ColPiece) * pieces.size())) ||
      (rc = mdev.alloc(arena, sizeof(ColMerge) * (merges.size() + 1))) || (rc = parts.alloc(arena, 32 * ((size_t)nparts + 1))))
    return rc;
  GM_HIP(hipMemcpyAsync(pdev.p, pieces.data(), sizeof(ColPiece) * pieces.size(), hipMemcpyHostToDevice, ctx->stream));
  if (!merges.empty())
    GM_HIP(hipMemcpyAsync(mdev.p, merges.data(), sizeof(ColMerge) * merges.size(), hipMemcpyHostToDevice,
                          ctx->stream));
  hipLaunchKernelGGL(k_col_piece<Fr>, dim3((unsigned)pieces.size()), dim3(COL_TPB), 0, ctx->stream,
                     pdev.as<ColPiece>(), trow.as<uint32_t>(), tcid.as<uint32_t>(), lag, (const Fe<Fr>*)r->coeff_i,
                     out, parts.as<uint32_t>());
  if (!merges.empty())
    hipLaunchKernelGGL(k_col_merge<Fr>, dim3((unsigned)merges.size()), dim3(COL_TPB), 0, ctx->stream,
                       mdev.as<ColMerge>(), parts.as<uint32_t>(), out);
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(ctx->stream));  // the host vectors were copied from
  return GM_OK;
}

// counts_only: stops after the compaction counts (gm_g16_setup_sizes)
template <class C>
int setup_scalars(gm_ctx* ctx, Arena& arena, const gm_r1cs* r, const SetupHost<C>& h, bool counts_only,
                  SetupScalars& s) {
  using Fr = typename C::Fr;
  using HF = typename SetupHost<C>::HF;
  const size_t nw = r->nb_wires, nc = r->nc;
  int rc;
  for (int m = 0; m < 3; m++)
    if ((rc = s.sum[m].alloc(arena, 32 * (nw + 1)))) return rc;
  for (int x = 0; x < 2; x++)
    if ((rc = s.inf[x].alloc(arena, nw + 1)) || (rc = s.compact[x].alloc(arena, 32 * (nw + 1)))) return rc;
  DevBuf lag;
  if ((rc = lag.alloc(arena, 32 * (nc + 1)))) return rc;
  {
    // Lagrange values
    Arena scope(ctx);
    DevBuf den, bprod;
    const unsigned nb = blocks_for(nc, 256);
    if ((rc = den.alloc(arena, sizeof(Fe<Fr>) * (nc + 1))) || (rc = bprod.alloc(arena, sizeof(Fe<Fr>) * (nb + 1))))
      return rc;
    if (nc) {
      ProfScope ps(ctx, "g16_setup_lagrange");
      hipLaunchKernelGGL(k_lag_den<Fr>, dim3(nb), dim3(256), 0, ctx->stream, nc, to_dev<HF, Fr>(h.omega),
                         to_dev<HF, Fr>(h.tau), lag.as<uint32_t>(), den.as<Fe<Fr>>(), bprod.as<Fe<Fr>>());
      hipLaunchKernelGGL(k_fb_invert<Fe<Fr>>, dim3(blocks_for(nb, 256)), dim3(256), 0, ctx->stream,
                         bprod.as<Fe<Fr>>(), (size_t)nb);
      hipLaunchKernelGGL(k_lag_apply<Fr>, dim3(nb), dim3(256), 0, ctx->stream, nc, to_dev<HF, Fr>(h.lag_scale),
                         (const Fe<Fr>*)den.as<Fe<Fr>>(), (const Fe<Fr>*)bprod.as<Fe<Fr>>(), lag.as<uint32_t>());
      GM_HIP(hipGetLastError());
    }
    GM_HIP(hipStreamSynchronize(ctx->stream));
  }
  for (int m = 0; m < 3; m++) {
    Arena scope(ctx);
    if ((rc = column_sums<C>(ctx, arena, r, m, lag.as<uint32_t>(), s.sum[m].as<uint32_t>()))) return rc;
  }
  {
    // InfinityA / InfinityB and the compaction
    Arena scope(ctx);
    ProfScope ps(ctx, "g16_setup_compact");
    DevBuf keep, pos, bsum;
    if ((rc = keep.alloc(arena, 4 * (nw + 1))) || (rc = pos.alloc(arena, 4 * (nw + 1))) ||
        (rc = bsum.alloc(arena, 4 * scan_ws_words(nw))))
      return rc;
    for (int x = 0; x < 2; x++) {
      uint32_t total = 0;
      if (nw) {
        hipLaunchKernelGGL(k_zero_flags, dim3(blocks_for(nw, 256)), dim3(256), 0, ctx->stream,
                           s.sum[x].as<uint4>(), nw, s.inf[x].as<uint8_t>(), keep.as<uint32_t>());
        if ((rc = device_excl_scan(ctx, keep.as<uint32_t>(), nw, pos.as<uint32_t>(), bsum.as<uint32_t>()))) return rc;
        if (!counts_only)
          hipLaunchKernelGGL(k_compact, dim3(blocks_for(nw, 256)), dim3(256), 0, ctx->stream, s.sum[x].as<uint4>(),
                             nw, (const uint32_t*)keep.as<uint32_t>(), (const uint32_t*)pos.as<uint32_t>(),
                             s.compact[x].as<uint4>());
        GM_HIP(hipGetLastError());
        GM_HIP(hipMemcpyAsync(&total, pos.as<uint32_t>() + nw, 4, hipMemcpyDeviceToHost, ctx->stream));
      }
      GM_HIP(hipStreamSynchronize(ctx->stream));
      (x ? s.nbB : s.nbA) = total;
    }
  }
  if (counts_only) return GM_OK;
  const size_t nbK = h.k_wires.size(), nbG = h.g_wires.size();
  if ((rc = s.k.alloc(arena, 32 * (nbK + 1))) || (rc = s.kg.alloc(arena, 32 * (nbG + 1))) ||
      (rc = s.z.alloc(arena, 32 * h.n)) || (rc = s.kw.alloc(arena, 4 * (nbK + 1))) ||
      (rc = s.gw.alloc(arena, 4 * (nbG + 1))))
    return rc;
  ProfScope ps(ctx, "g16_setup_kz");
  if (nbK) GM_HIP(hipMemcpyAsync(s.kw.p, h.k_wires.data(), 4 * nbK, hipMemcpyHostToDevice, ctx->stream));
  if (nbG) GM_HIP(hipMemcpyAsync(s.gw.p, h.g_wires.data(), 4 * nbG, hipMemcpyHostToDevice, ctx->stream));
  const uint32_t *A = s.sum[0].as<uint32_t>(), *B = s.sum[1].as<uint32_t>(), *Cc = s.sum[2].as<uint32_t>();
  if (nbK)
    hipLaunchKernelGGL(k_setup_k<Fr>, dim3(blocks_for(nbK, 256)), dim3(256), 0, ctx->stream,
                       (const uint32_t*)s.kw.as<uint32_t>(), nbK, A, B, Cc, to_dev<HF, Fr>(h.alpha),
                       to_dev<HF, Fr>(h.beta), to_dev<HF, Fr>(h.dinv), s.k.as<uint32_t>());
  if (nbG)
    hipLaunchKernelGGL(k_setup_k<Fr>, dim3(blocks_for(nbG, 256)), dim3(256), 0, ctx->stream,
                       (const uint32_t*)s.gw.as<uint32_t>(), nbG, A, B, Cc, to_dev<HF, Fr>(h.alpha),
                       to_dev<HF, Fr>(h.beta), to_dev<HF, Fr>(h.ginv), s.kg.as<uint32_t>());
  if (h.n > 1)
    hipLaunchKernelGGL(k_setup_z<Fr>, dim3(blocks_for(h.n - 1, 256)), dim3(256), 0, ctx->stream, h.n,
                       (uint32_t)h.logn, to_dev<HF, Fr>(h.tau), to_dev<HF, Fr>(h.z_scale), s.z.as<uint32_t>());
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

// n points [k_i] G in gnark layout, left in the caller's arena
template <class C, bool G2>
int points_on_device(gm_ctx* ctx, Arena& arena, const void* scalars_dev, size_t n, DevBuf& pts) {
  const int curve = C::id == 0 ? GM_BN254 : GM_BLS12_377;
  const size_t pb = fp_bytes(curve) * (G2 ? 4 : 2);
  if (int rc = pts.alloc(arena, pb * (n + 1))) return rc;
  if (n == 0) return GM_OK;
  uint8_t gen[192];
  gm_generator(curve, G2 ? 1 : 0, gen);
  return batch_mul_fixed_device<C, G2>(ctx, gen, scalars_dev, n, pts.p);
}

// sizes != NULL: the counts alone.  Else the key's arrays, copied into the non-NULL
// members of `out` (if any) and, with pk_out, made the resident key.
template <class C>
int setup_t(gm_ctx* ctx, const char* entry, const gm_r1cs* r, const gm_g16_setup_in* in, const gm_g16_setup_out* out,
            size_t* sizes, unsigned flags, gm_g16_pk** pk_out) {
  using HF = typename SetupHost<C>::HF;
  SetupHost<C> h;
  if (int rc = setup_judge<C>(entry, r, in, h)) return rc;
  if (pk_out && h.n < 2) return refuse_setup(entry, "a key needs a domain of at least two constraints");
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  StreamDrain drain{ctx};
  SetupScalars s;
  int rc;
  if ((rc = setup_scalars<C>(ctx, arena, r, h, sizes != nullptr, s))) return rc;
  if (sizes) {
    sizes[0] = s.nbA, sizes[1] = s.nbB, sizes[2] = h.k_wires.size();
    return GM_OK;
  }
  const size_t nw = r->nb_wires, nbK = h.k_wires.size(), nbG = h.g_wires.size();
  const size_t g1b = 2 * fp_bytes(r->curve), g2b = 2 * g1b;
  DevBuf pA, pB, pZ, pK, pB2, pKg;
  {
    ProfScope ps(ctx, "g16_setup_g1");
    if ((rc = points_on_device<C, false>(ctx, arena, s.compact[0].p, s.nbA, pA)) ||
        (rc = points_on_device<C, false>(ctx, arena, s.compact[1].p, s.nbB, pB)) ||
        (rc = points_on_device<C, false>(ctx, arena, s.z.p, h.n - 1, pZ)) ||
        (rc = points_on_device<C, false>(ctx, arena, s.k.p, nbK, pK)))
      return rc;
    if (out && out->g1_K_gamma && (rc = points_on_device<C, false>(ctx, arena, s.kg.p, nbG, pKg))) return rc;
  }
  {
    ProfScope ps(ctx, "g16_setup_g2");
    if ((rc = points_on_device<C, true>(ctx, arena, s.compact[1].p, s.nbB, pB2))) return rc;
  }
  // the single points: alpha, beta, delta in G1; beta, delta, gamma in G2
  const HF one1[3] = {h.alpha, h.beta, h.delta}, one2[3] = {h.beta, h.delta, h.gamma};
  uint8_t p1[3 * 96], p2[3 * 192];
  DevBuf sc, sp;
  if ((rc = sc.alloc(arena, 256))) return rc;
  GM_HIP(hipMemcpyAsync(sc.p, one1, sizeof(one1), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = points_on_device<C, false>(ctx, arena, sc.p, 3, sp))) return rc;
  GM_HIP(hipMemcpyAsync(p1, sp.p, 3 * g1b, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipMemcpyAsync(sc.p, one2, sizeof(one2), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = points_on_device<C, true>(ctx, arena, sc.p, 3, sp))) return rc;
  GM_HIP(hipMemcpyAsync(p2, sp.p, 3 * g2b, hipMemcpyDeviceToHost, ctx->stream));
  std::vector<uint8_t> infA(nw), infB(nw);
  GM_HIP(hipMemcpyAsync(infA.data(), s.inf[0].p, nw, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipMemcpyAsync(infB.data(), s.inf[1].p, nw, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  if (out) {
    ProfScope ps(ctx, "g16_setup_d2h");
    void* const d1[3] = {out->g1_alpha, out->g1_beta, out->g1_delta};
    void* const d2[3] = {out->g2_beta, out->g2_delta, out->g2_gamma};
    for (int i = 0; i < 3; i++) {
      if (d1[i]) memcpy(d1[i], p1 + g1b * i, g1b);
      if (d2[i]) memcpy(d2[i], p2 + g2b * i, g2b);
    }
    if (out->infA) memcpy(out->infA, infA.data(), nw);
    if (out->infB) memcpy(out->infB, infB.data(), nw);
    if (out->k_wires && nbK) memcpy(out->k_wires, h.k_wires.data(), 4 * nbK);
    const struct {
      void* dst;
      const DevBuf* src;
      size_t bytes;
    } copies[6] = {{out->g1_A, &pA, g1b * s.nbA}, {out->g1_B, &pB, g1b * s.nbB}, {out->g1_Z, &pZ, g1b * (h.n - 1)},
                   {out->g1_K, &pK, g1b * nbK},   {out->g1_K_gamma, &pKg, g1b * nbG}, {out->g2_B, &pB2, g2b * s.nbB}};
    for (const auto& cp : copies)
      if (cp.dst && cp.bytes)
        GM_HIP(hipMemcpyAsync(cp.dst, cp.src->p, cp.bytes, hipMemcpyDeviceToHost, ctx->stream));
    GM_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (!pk_out) return GM_OK;
  // the resident key: gm_g16_pk_upload_ex's own tail, fed from the derived arrays
  gm_g16_pk_host hk = {};
  hk.domain_size = h.n, hk.nb_wires = nw, hk.nb_public = in->nb_public;
  hk.nbA = s.nbA, hk.nbB = s.nbB, hk.nbK = nbK;
  hk.g1_alpha = p1, hk.g1_beta = p1 + g1b, hk.g1_delta = p1 + 2 * g1b;
  hk.g2_beta = p2, hk.g2_delta = p2 + g2b;
  hk.infA = infA.data(), hk.infB = infB.data();
  hk.k_wires = h.k_wires.data();
  const void* const derived[5] = {pA.p, pB.p, pZ.p, pK.p, pB2.p};  // PkArray order
  const PointSource src = [&](int which, size_t count, bool g2, const MsmPrecomp* pre, void* dst) -> int {
    int e = prepare_points_into(ctx, r->curve, g2, derived[which], count, pre, dst);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && !e) e = GM_ERR_DEVICE;
    return e;
  };
  const Ranges rg = {0, s.nbA, 0, s.nbB, 0, nbK, 0, h.n - 1, false};
  return pk_upload_ranges(ctx, r->curve, &hk, flags, rg, pk_out, &src);
}

}  // namespace

int g16_setup_run(gm_ctx* ctx, const char* entry, const gm_r1cs* r, const gm_g16_setup_in* in,
                  const gm_g16_setup_out* out, size_t* sizes, unsigned flags, gm_g16_pk** pk_out) {
  return r->curve == GM_BN254 ? setup_t<CurveBN254>(ctx, entry, r, in, out, sizes, flags, pk_out)
                              : setup_t<CurveBLS12377>(ctx, entry, r, in, out, sizes, flags, pk_out);
}

}  // namespace gm
