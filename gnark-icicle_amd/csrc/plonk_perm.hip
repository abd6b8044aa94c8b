// PLONK permutation polynomial Z on gfx950 -- replaces buildRatioCopyConstraint of
// gnark's PLONK prover (backend/plonk/bls12-377/prove.go:565-597, gnark-crypto's
// iop.BuildRatioCopyConstraint + fr.BatchInvert) for wires that are resident on
// the device.  The result is defined in include/gnark_mi355x.h (gm_plonk_perm_z):
//   Z[0] = 1,  Z[i+1] = N_i inv0(D_i),  N_i = prod_{j<=i} num_j,  D_i = prod_{j<=i} den_j
// over the rows i < n - 1.
//
// One inversion serves the whole call.  With d'_j = den_j, or 1 where den_j = 0,
// and T = prod_j d'_j (never zero):
//   inv(D'_i) = inv(T) prod_{j>i} d'_j
// so Z[i+1] = (prefix product of num up to i) (suffix product of d' past i) inv(T),
// and D'_i = D_i for every row before the first zero denominator j0; the rows
// i >= j0 store 0 (inv0).  A zero numerator needs nothing: the prefix product is 0
// from there on.  The scans are blocked: a chunk is C = TPB * E consecutive rows
// (512), a thread owns a run of E of them.
//   k_perm_chunk_prod  per chunk k: n_k = prod num_j, d_k = prod d'_j, and the first
//                      row with a zero denominator.  A product needs no order, so
//                      lane t takes rows r TPB + t (consecutive lanes consecutive
//                      32 B elements) and an LDS tree finishes.
//   k_perm_carry       one block, tiled in the shape of k_poly_chunk_carry (CT =
//                      64 chunks per tile, a lane per chunk), three waves side by
//                      side: prod_{j<k} n_j (tiles upwards), prod_{j>k} d_j (tiles
//                      downwards), and inv(T) by the call's only fe_inv with j0 =
//                      the minimum of the chunks' first zero rows.  The scans go by
//                      wave shuffles: no LDS, no barrier, and nothing waits for
//                      another wave or block.
//   k_perm_write       num and d' of the chunk again, row by row as above, into two
//                      LDS stagings laid out by run; the run's lane turns them into
//                      prefix / exclusive suffix products in place, a Hillis-Steele
//                      scan over the TPB run totals (prefix for num, suffix for d')
//                      joins the runs, and Z[i+1] = (pn_i sd_i) X_t with one X_t per
//                      run that holds the run's and the chunk's carries and inv(T).
//                      Z replaces num in the staging and leaves by 16 B units,
//                      consecutive lanes consecutive addresses, one element up:
//                      the shift by one costs nothing at run, chunk or tile edges.
//                      Z[0] = 1 is stored by chunk 0; rows >= n - 1 count as
//                      num = d' = 1 and store nothing.
// w^i: lane t reads w^(base + t) once from the domain's table w^brev(p)
// (ntt_brev_roots) and multiplies along by w^TPB, another entry of the same table.
//
// Number forms (field.hpp): mul(a, b) = a b / 2^(29 N).  Stored values are gnark
// Montgomery elements (v 2^256), the table and g, beta for the s_k products are
// internal (v 2^(29 N)): mul(gnark, internal) is gnark, so the six factors of a
// row are gnark sums with no conversion.  The product of three gnark factors is
// the internal form of num_i c with c = 2^(2 (256 - 29 N)), the same c for den_i:
// prefix and suffix products then carry c^(i+1) and c^-(i+1), which cancel in
// N_i / D_i.  inv(T) is multiplied once by the internal -> gnark constant, so the
// last product of a row leaves Z in gnark form.  Every sum and product is fully
// reduced: the stored words are gnark-crypto's.
//
// LDS staging as kzg.hip: gnark words as 16 B units, a run's 2E units followed by
// one unit of padding (runs of consecutive lanes 9 units apart).  Two stagings of
// 18432 B and two scan arrays of 4608 B: 46080 B per block of two waves, three
// blocks (six waves) per CU.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage;
// BN254 / BLS12-377 Fr), no scratch and no VGPR spill in any of them:
//   k_perm_chunk_prod  152 / 157 VGPRs,  9220 B LDS, 3 waves per SIMD
//   k_perm_carry        58 /  66 VGPRs,     0 B LDS (one block of three waves)
//   k_perm_write       142 / 183 VGPRs, 46080 B LDS, 2 waves per SIMD by registers,
//                      three blocks (six waves) per CU by LDS
// Runs of eight rows would halve the share of the scan over the runs (14 products
// per run) but need 79 KB of LDS per block: one wave per SIMD.
#include <cstring>

#include "curves.hpp"
#include "kzg.hpp"
#include "ntt.hpp"
#include "plonk_perm.hpp"
#include "runtime.hpp"

namespace gm {

constexpr int PERM_RUN_U4 = 2 * PERM_E + 1;
constexpr unsigned PERM_NO_ZERO = 0xFFFFFFFFu;

// the constants of one call, by value
template <class P>
struct PermK {
  FeG<P> beta_g;   // gnark: mul(w^i internal, beta_g) = beta w^i gnark
  FeG<P> beta_i;   // internal: mul(s gnark, beta_i) = beta s gnark
  FeG<P> g_i;      // internal: the coset generator g
  FeG<P> gamma_g;  // gnark
  FeG<P> one_g;    // gnark: Z[0]
};

// beta g^k w^i for the rows row0 + r TPB of one lane, gnark form
template <class P>
struct PermX {
  Fe<P> bx[3];
  Fe<P> step;  // internal: w^TPB
};

template <class P>
GM_DEV PermX<P> perm_x_init(const PermK<P>& k, const Fe<P>* __restrict__ wbrev, size_t n, int logn, size_t row0) {
  PermX<P> x;
  x.bx[0] = x.bx[1] = x.bx[2] = fe_zero<P>();
  x.step = fe_one<P>();
  if (row0 < n) {
    const Fe<P> g = fe_unpack<P>(k.g_i);
    x.bx[0] = fe_mul(wbrev[brev_bits((uint32_t)row0, logn)], fe_unpack<P>(k.beta_g));
    x.bx[1] = fe_mul(x.bx[0], g);
    x.bx[2] = fe_mul(x.bx[1], g);
  }
  if ((size_t)PERM_TPB < n) x.step = wbrev[brev_bits((uint32_t)PERM_TPB, logn)];
  return x;
}

struct PermIn {
  const void *l, *r, *o, *s1, *s2, *s3;
};

// num and d' of one row (internal form of num c, den c); a row at or past n - 1
// gives 1, 1.  *zero: the row's denominator was 0 (d' = 1 then).
template <class P>
GM_DEV void perm_row(const PermIn& in, const PermK<P>& k, const PermX<P>& x, size_t row, size_t n, Fe<P>& num,
                     Fe<P>& den, bool& zero) {
  zero = false;
  if (row + 1 >= n) {
    num = den = fe_one<P>();
    return;
  }
  const Fe<P> gam = fe_unpack<P>(k.gamma_g), be = fe_unpack<P>(k.beta_i);
  const Fe<P> lg = fe_add(fe_load_g<P>(in.l, row), gam);
  const Fe<P> rg = fe_add(fe_load_g<P>(in.r, row), gam);
  const Fe<P> og = fe_add(fe_load_g<P>(in.o, row), gam);
  num = fe_mul(fe_mul(fe_add(lg, x.bx[0]), fe_add(rg, x.bx[1])), fe_add(og, x.bx[2]));
  den = fe_mul(fe_mul(fe_add(lg, fe_mul(fe_load_g<P>(in.s1, row), be)), fe_add(rg, fe_mul(fe_load_g<P>(in.s2, row), be))),
               fe_add(og, fe_mul(fe_load_g<P>(in.s3, row), be)));
  if (fe_is_zero(den)) {
    zero = true;
    den = fe_one<P>();
  }
}

template <class P>
GM_DEV void perm_x_next(PermX<P>& x) {
#pragma unroll
  for (int c = 0; c < 3; c++) x.bx[c] = fe_mul(x.bx[c], x.step);
}

// element e of run t of a staging (unpacked)
template <class P>
GM_DEV Fe<P> perm_get(const uint4* __restrict__ stage, int t, int e) {
  const uint4 a = stage[t * PERM_RUN_U4 + 2 * e], b = stage[t * PERM_RUN_U4 + 2 * e + 1];
  FeG<P> g;
  g.w[0] = a.x, g.w[1] = a.y, g.w[2] = a.z, g.w[3] = a.w;
  g.w[4] = b.x, g.w[5] = b.y, g.w[6] = b.z, g.w[7] = b.w;
  return fe_unpack<P>(g);
}
template <class P>
GM_DEV void perm_put(uint4* __restrict__ stage, int t, int e, const Fe<P>& v) {
  static_assert(P::NG == 8, "two 16 B units per element");
  const FeG<P> g = fe_pack(v);
  stage[t * PERM_RUN_U4 + 2 * e] = make_uint4(g.w[0], g.w[1], g.w[2], g.w[3]);
  stage[t * PERM_RUN_U4 + 2 * e + 1] = make_uint4(g.w[4], g.w[5], g.w[6], g.w[7]);
}

// One block per chunk.  tot[2 k] = n_k, tot[2 k + 1] = d_k (internal values in gnark
// word layout), zr[k] = the chunk's first row with den = 0, or PERM_NO_ZERO.
template <class P>
__global__ void __launch_bounds__(PERM_TPB) k_perm_chunk_prod(PermIn in, size_t n, int logn, PermK<P> k,
                                                              const Fe<P>* __restrict__ wbrev, void* __restrict__ tot,
                                                              unsigned* __restrict__ zr) {
  __shared__ Fe<P> vn[PERM_TPB], vd[PERM_TPB];
  __shared__ unsigned zmin;
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * PERM_C;
  if (t == 0) zmin = PERM_NO_ZERO;
  PermX<P> x = perm_x_init<P>(k, wbrev, n, logn, base + t);
  Fe<P> pn = fe_one<P>(), pd = fe_one<P>();
  unsigned z = PERM_NO_ZERO;
#pragma unroll 1
  for (int r = 0; r < PERM_E; r++) {
    const size_t row = base + (size_t)r * PERM_TPB + t;
    Fe<P> num, den;
    bool zero;
    perm_row<P>(in, k, x, row, n, num, den, zero);
    if (zero && z == PERM_NO_ZERO) z = (unsigned)row;
    pn = fe_mul(pn, num);
    pd = fe_mul(pd, den);
    perm_x_next(x);
  }
  vn[t] = pn;
  vd[t] = pd;
  __syncthreads();
  if (z != PERM_NO_ZERO) atomicMin(&zmin, z);
  // level d: v[j 2^(d+1)] *= v[j 2^(d+1) + 2^d], the active threads packed low
  for (int d = 0; d < PERM_TPB_LOG; d++) {
    __syncthreads();
    if (t < (PERM_TPB >> (d + 1))) {
      const int lo = t << (d + 1);
      vn[lo] = fe_mul(vn[lo], vn[lo + (1 << d)]);
      vd[lo] = fe_mul(vd[lo], vd[lo + (1 << d)]);
    }
  }
  if (t == 0) {
    fe_store_g<P>(tot, 2 * (size_t)blockIdx.x, vn[0]);
    fe_store_g<P>(tot, 2 * (size_t)blockIdx.x + 1, vd[0]);
    zr[blockIdx.x] = zmin;
  }
}

// lane l takes the value of lane l - d (lanes below d: their own)
template <class P>
GM_DEV Fe<P> perm_shfl_up(const Fe<P>& a, int d) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::N; i++) r.v[i] = __shfl_up(a.v[i], d, PERM_CT);
  return r;
}
template <class P>
GM_DEV Fe<P> perm_shfl_xor(const Fe<P>& a, int d) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::N; i++) r.v[i] = __shfl_xor(a.v[i], d, PERM_CT);
  return r;
}
template <class P>
GM_DEV Fe<P> perm_shfl(const Fe<P>& a, int lane) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::N; i++) r.v[i] = __shfl(a.v[i], lane, PERM_CT);
  return r;
}

// One block of three waves, each on its own and none waiting for another:
//   wave 0  car[2 k] = prod_{j<k} n_j: an exclusive prefix scan in tiles of CT = 64
//           chunks, a lane per chunk, Hillis-Steele by wave shuffles; the tile's
//           first lane takes in the product of the tiles below
//   wave 1  car[2 k + 1] = prod_{j>k} d_j: the same scan over the chunks in
//           reverse order
//   wave 2  car[2 nchunk] = inv(prod_j d_j) times the internal -> gnark constant
//           (strided products, a butterfly, the call's only fe_inv), and
//           zr[nchunk] = min_k zr[k]
// tot is only read, so the waves share nothing they write.
template <class P>
__global__ void __launch_bounds__(3 * PERM_CT) k_perm_carry(size_t nchunk, const void* __restrict__ tot,
                                                            void* __restrict__ car, unsigned* __restrict__ zr) {
  static_assert(PERM_CT == 64, "a tile of the carry scan is one wave");
  const int role = threadIdx.x >> PERM_CT_LOG, lane = threadIdx.x & (PERM_CT - 1);
  if (role == 2) {
    Fe<P> p = fe_one<P>();
    unsigned z = PERM_NO_ZERO;
    for (size_t c = lane; c < nchunk; c += PERM_CT) {
      p = fe_mul(p, fe_load_g<P>(tot, 2 * c + 1));
      z = min(z, zr[c]);
    }
    for (int d = 1; d < PERM_CT; d <<= 1) {
      p = fe_mul(p, perm_shfl_xor(p, d));
      z = min(z, (unsigned)__shfl_xor(z, d, PERM_CT));
    }
    if (lane == 0) {
      fe_store_g<P>(car, 2 * nchunk, fe_to_gnark(fe_inv(p)));
      zr[nchunk] = z;
    }
    return;
  }
  const size_t ntile = (nchunk + PERM_CT - 1) / PERM_CT;
  Fe<P> edge = fe_one<P>();
  for (size_t tile = 0; tile < ntile; tile++) {
    const size_t q = tile * PERM_CT + lane;  // position in scan order
    const bool valid = q < nchunk;
    const size_t slot = role == 0 ? 2 * q : 2 * (nchunk - 1 - q) + 1;
    Fe<P> x = valid ? fe_load_g<P>(tot, slot) : fe_one<P>();
    if (lane == 0) x = fe_mul(x, edge);
    for (int d = 1; d < PERM_CT; d <<= 1) {
      const Fe<P> lo = perm_shfl_up(x, d);
      if (lane >= d) x = fe_mul(x, lo);
    }
    Fe<P> ex = perm_shfl_up(x, 1);
    if (lane == 0) ex = edge;
    edge = perm_shfl(x, PERM_CT - 1);
    if (valid) fe_store_g<P>(car, slot, ex);
  }
}

// One block per chunk; car, zr as k_perm_carry left them.
template <class P>
__global__ void __launch_bounds__(PERM_TPB) k_perm_write(PermIn in, size_t n, int logn, PermK<P> k,
                                                         const Fe<P>* __restrict__ wbrev, size_t nchunk,
                                                         const void* __restrict__ car,
                                                         const unsigned* __restrict__ zr, void* __restrict__ out) {
  __shared__ uint4 sn[PERM_TPB * PERM_RUN_U4], sd[PERM_TPB * PERM_RUN_U4];
  __shared__ Fe<P> vn[PERM_TPB], vd[PERM_TPB];
  const int t = threadIdx.x;
  const size_t kc = blockIdx.x;
  const size_t base = kc * PERM_C;
  {
    PermX<P> x = perm_x_init<P>(k, wbrev, n, logn, base + t);
#pragma unroll 1
    for (int r = 0; r < PERM_E; r++) {
      const int e = r * PERM_TPB + t;
      Fe<P> num, den;
      bool zero;
      perm_row<P>(in, k, x, base + e, n, num, den, zero);
      perm_put<P>(sn, e >> PERM_E_LOG, e & (PERM_E - 1), num);
      perm_put<P>(sd, e >> PERM_E_LOG, e & (PERM_E - 1), den);
      perm_x_next(x);
    }
  }
  __syncthreads();
  // the run: sn[e] -> prod_{j<=e} num, sd[e] -> prod_{j>e} d'
  Fe<P> xn = perm_get<P>(sn, t, 0);
#pragma unroll
  for (int e = 1; e < PERM_E; e++) {
    xn = fe_mul(xn, perm_get<P>(sn, t, e));
    perm_put<P>(sn, t, e, xn);
  }
  Fe<P> xd = perm_get<P>(sd, t, PERM_E - 1);
  perm_put<P>(sd, t, PERM_E - 1, fe_one<P>());
#pragma unroll
  for (int e = PERM_E - 2; e >= 0; e--) {
    const Fe<P> d = perm_get<P>(sd, t, e);
    perm_put<P>(sd, t, e, xd);
    xd = fe_mul(xd, d);
  }
  vn[t] = xn;
  vd[t] = xd;
  // over the runs: xn -> prefix of the run totals, xd -> suffix
  for (int d = 0; d < PERM_TPB_LOG; d++) {
    __syncthreads();
    const bool hl = t >= (1 << d), hh = t + (1 << d) < PERM_TPB;
    Fe<P> lo = fe_one<P>(), hi = fe_one<P>();
    if (hl) lo = vn[t - (1 << d)];
    if (hh) hi = vd[t + (1 << d)];
    __syncthreads();
    if (hl) {
      xn = fe_mul(xn, lo);
      vn[t] = xn;
    }
    if (hh) {
      xd = fe_mul(xd, hi);
      vd[t] = xd;
    }
  }
  __syncthreads();
  // X_t = (numerators below the run) (denominators above it) inv(T)
  Fe<P> X = fe_mul(fe_load_g<P>(car, 2 * kc), fe_mul(fe_load_g<P>(car, 2 * kc + 1), fe_load_g<P>(car, 2 * nchunk)));
  if (t > 0) X = fe_mul(X, vn[t - 1]);
  if (t + 1 < PERM_TPB) X = fe_mul(X, vd[t + 1]);
  const size_t j0 = zr[nchunk];  // PERM_NO_ZERO is past every row
  for (int e = 0; e < PERM_E; e++) {
    Fe<P> z = fe_mul(fe_mul(perm_get<P>(sn, t, e), perm_get<P>(sd, t, e)), X);
    if (base + (size_t)t * PERM_E + e >= j0) z = fe_zero<P>();
    perm_put<P>(sn, t, e, z);
  }
  __syncthreads();
  // row i's value is Z[i + 1]
  uint4* dst = reinterpret_cast<uint4*>(out);
#pragma unroll
  for (int r = 0; r < 2 * PERM_E; r++) {
    const int u = r * PERM_TPB + t;
    const int e = u >> 1;
    const size_t g = base + e;
    if (g + 1 < n)
      dst[2 * (g + 1) + (u & 1)] = sn[(e >> PERM_E_LOG) * PERM_RUN_U4 + (e & (PERM_E - 1)) * 2 + (u & 1)];
  }
  if (kc == 0 && t == 0) feg_store<P>(reinterpret_cast<uint32_t*>(out), k.one_g);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <class C>
int plonk_perm_z_device(gm_ctx* ctx, const gm_plonk_perm_in* in, void* z_lagrange, void* z_canonical) {
  using Fr = typename C::Fr;
  using HFr = typename C::HFr;
  using HF = host::F<HFr>;
  const size_t n = in->n;
  int logn = 0;
  while (((size_t)1 << logn) < n && logn < 62) logn++;
  if (((size_t)1 << logn) != n || n < 8 || logn > C::TWO_ADICITY || logn > 30) {
    set_error("plonk perm: n must be a power of two >= 8 within the 2-adicity");
    return GM_ERR_INVALID;
  }
  if (!in->beta || !in->gamma) {
    set_error("plonk perm: beta and gamma must be non-null");
    return GM_ERR_INVALID;
  }
  const void* src[6] = {in->l, in->r, in->o, in->s1, in->s2, in->s3};
  const void* dst[2] = {z_lagrange, z_canonical};
  if (!z_lagrange) {
    set_error("plonk perm: z_lagrange must be non-null");
    return GM_ERR_INVALID;
  }
  for (const void* p : src)
    if (!p || (uintptr_t)p % 16) {
      set_error("plonk perm: polynomial pointers must be non-null and 16-byte aligned");
      return GM_ERR_INVALID;
    }
  for (const void* q : dst) {
    if (!q) continue;
    if ((uintptr_t)q % 16) {
      set_error("plonk perm: output pointers must be 16-byte aligned");
      return GM_ERR_INVALID;
    }
    const uintptr_t q0 = (uintptr_t)q, q1 = q0 + 32 * n;
    for (const void* p : src) {
      const uintptr_t p0 = (uintptr_t)p;
      if (p0 < q1 && q0 < p0 + 32 * n) {
        set_error("plonk perm: an output must not overlap an input");
        return GM_ERR_INVALID;
      }
    }
  }
  if (z_canonical) {
    const uintptr_t a0 = (uintptr_t)z_lagrange, b0 = (uintptr_t)z_canonical;
    if (a0 < b0 + 32 * n && b0 < a0 + 32 * n) {
      set_error("plonk perm: the outputs must not overlap each other");
      return GM_ERR_INVALID;
    }
  }

  auto ld = [](const void* p) {
    HF v;
    memcpy(v.v, p, sizeof(v.v));
    return v;
  };
  const HF beta = ld(in->beta), gamma = ld(in->gamma);
  auto G = [](const HF& h) {
    FeG<Fr> r;
    static_assert(sizeof(r.w) == sizeof(h.v), "gnark layout");
    memcpy(r.w, h.v, sizeof(r.w));
    return r;
  };
  PermK<Fr> k;
  k.beta_g = G(beta);
  k.beta_i = to_internal_words<C>(beta);
  k.g_i = to_internal_words<C>(host::from_u64<HFr>(C::COSET_GEN));
  k.gamma_g = G(gamma);
  k.one_g = G(HF::one());
  const PermIn pin = {in->l, in->r, in->o, in->s1, in->s2, in->s3};

  const size_t nchunk = (n - 1 + PERM_C - 1) / PERM_C;
  int rc;
  const void* wbrev;
  if ((rc = ntt_brev_roots<C>(ctx, n, &wbrev))) return rc;
  Arena arena(ctx);
  DevBuf tot, car, zr;
  if ((rc = tot.alloc(arena, 32 * 2 * nchunk))) return rc;
  if ((rc = car.alloc(arena, 32 * (2 * nchunk + 1)))) return rc;
  if ((rc = zr.alloc(arena, sizeof(unsigned) * (nchunk + 1)))) return rc;
  {
    ProfScope ps(ctx, "plonk_perm_chunk_prod");
    hipLaunchKernelGGL(k_perm_chunk_prod<Fr>, dim3((unsigned)nchunk), dim3(PERM_TPB), 0, ctx->stream, pin, n, logn,
                       k, (const Fe<Fr>*)wbrev, tot.p, zr.as<unsigned>());
    GM_HIP(hipGetLastError());
  }
  {
    ProfScope ps(ctx, "plonk_perm_carry");
    hipLaunchKernelGGL(k_perm_carry<Fr>, dim3(1), dim3(3 * PERM_CT), 0, ctx->stream, nchunk, (const void*)tot.p,
                       car.p, zr.as<unsigned>());
    GM_HIP(hipGetLastError());
  }
  {
    ProfScope ps(ctx, "plonk_perm_write");
    hipLaunchKernelGGL(k_perm_write<Fr>, dim3((unsigned)nchunk), dim3(PERM_TPB), 0, ctx->stream, pin, n, logn, k,
                       (const Fe<Fr>*)wbrev, nchunk, (const void*)car.p, (const unsigned*)zr.p, z_lagrange);
    GM_HIP(hipGetLastError());
  }
  if (!z_canonical) return GM_OK;
  // Lagrange regular -> canonical regular: reversal, then the inverse DIT
  // (bit-reversed in, natural out)
  ProfScope ps(ctx, "plonk_perm_canonical");
  if ((rc = bitrev_copy_device<C>(ctx, z_canonical, z_lagrange, n))) return rc;
  return ntt_device<C>(ctx, z_canonical, n, true, true, false);
}

template int plonk_perm_z_device<CurveBN254>(gm_ctx*, const gm_plonk_perm_in*, void*, void*);
template int plonk_perm_z_device<CurveBLS12377>(gm_ctx*, const gm_plonk_perm_in*, void*, void*);

}  // namespace gm
