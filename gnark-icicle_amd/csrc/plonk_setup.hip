// PLONK setup on the device: what gnark's plonk.Setup (backend/plonk/bls12-377/
// setup.go) and its caller compute on the CPU before a first proof.
//
//  * The Lagrange-form SRS (gnark-crypto kzg.ToLagrangeG1): an inverse FFT over
//    G1 points, out[i] = (1/n) sum_j w^(-ij) in[j].  Radix-2 decimation in
//    frequency on XYZZ points in workspace, one launch per stage, one thread per
//    butterfly (a, b) -> (a + b, [t](a - b)), t = w^(-j 2^s) in stage s; then one
//    pass that multiplies by 1/n, converts to affine and writes natural order
//    (stage outputs are bit-reversed).  Affine coordinates are unique, so the
//    bytes do not depend on the butterfly order.
//
//    The work is the scalar multiplication [t](a - b): a doubling per bit and
//    an addition of +-(a - b) per non-zero digit of t's non-adjacent form (a
//    third of the digits, against half of the bits), on complete XYZZ formulas
//    (a - b may be any point, infinity included, and so may every partial sum).
//    Twiddles are canonical integers recoded once, 16 u32 words each, in one
//    table of n/2 entries.
//      - Stage s has 2^s butterflies per twiddle, and they are numbered
//        twiddle-major.  From s = 6 on the 64 lanes of a wave share t: its words
//        are read once per wave (readfirstlane) and the add is a uniform branch,
//        taken for the non-zero digits only.
//      - For s < 6 a wave holds 64 / 2^s twiddles and the loop diverges: the add
//        runs under the mask of the lanes with a non-zero digit.  With 8 or more
//        twiddles nearly every position has one, so the wave pays a doubling and
//        an addition per bit there (with 2 twiddles, s = 5, 5 positions in 9).  A
//        branch-free select would issue the doubling and the addition at every
//        position for the whole wave and a 4-coordinate select on top, so the
//        divergent loop is kept: never more instructions, fewer registers.
//      - t = 1 (j = 0) takes no multiplication: the whole last stage, and one
//        butterfly per block elsewhere.
//
//  * S1, S2, S3 (computePermutationPolynomials, setup.go:330-374): a gather
//    s_k[i] = g^(S / n) w^(S mod n) through one table of w^i.
//
//  * The key from what Setup holds: the two derivations, then the tail
//    gm_plonk_pk_upload runs (plonk_pk.hip), with commitTrace's digests
//    (setup.go:217-251) taken over the derived Lagrange SRS on the way.
#include <cstring>
#include <string>

#include "curves.hpp"
#include "msm.hpp"
#include "ntt.hpp"
#include "plonk_pk.hpp"
#include "plonk_scs.hpp"
#include "plonk_setup.hpp"
#include "plonk_wires_perm.hpp"
#include "runtime.hpp"

namespace gm {

namespace {

// one wave per block: a wave is the unit that shares a twiddle, and the
// butterfly's register need leaves no room for a second one per SIMD anyway
constexpr unsigned ECFFT_TPB = 64;
// first stage in which a wave has a single twiddle (2^s >= the wave's 64 lanes)
constexpr uint32_t ECFFT_UNIFORM_STAGE = 6;

// A scalar k < 2^254 as the kernels read it: its non-adjacent form, digit i =
// bit i of plus - bit i of minus, i < 255.  With h = 3k, digit i is bit i + 1 of h
// minus bit i + 1 of k.  A third of the digits are non-zero, against half of k's bits.
struct Naf {
  uint32_t plus[8], minus[8];
};
constexpr int NAF_WORDS = 16;

GM_HD Naf naf_of(const uint32_t (&k)[8]) {
  uint32_t h[9];
  uint64_t c = 0;
  for (int i = 0; i < 8; i++) {
    c += 3ull * k[i];
    h[i] = (uint32_t)c;
    c >>= 32;
  }
  h[8] = (uint32_t)c;
  Naf r;
  for (int i = 0; i < 8; i++) {
    const uint32_t hs = (h[i] >> 1) | (h[i + 1] << 31);
    const uint32_t ks = (k[i] >> 1) | ((i < 7 ? k[i + 1] : 0u) << 31);
    r.plus[i] = hs & ~ks;
    r.minus[i] = ks & ~hs;
  }
  return r;
}

// out[i] = base^i for i < count: the non-adjacent form of the canonical integer
// (NAF; the EC-FFT's twiddles, 16 u32 words) or the gnark Montgomery form (the
// table S1, S2, S3 gather from, 8 u32 words)
template <class Fr, bool NAF>
__global__ void __launch_bounds__(256) k_powers(uint32_t* __restrict__ out, size_t count, FeG<Fr> base_gnark) {
  static_assert(Fr::NG == 8 && Fr::BITS <= 254, "scalar fields of 8 u32 words, 3 k < 2^256");
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const Fe<Fr> r = fe_pow(fe_to_internal(fe_unpack<Fr>(base_gnark)), i);
  if constexpr (NAF) {
    const Naf d = naf_of(fe_pack(fe_from_mont(r)).w);
    uint4* const dst = reinterpret_cast<uint4*>(out + i * NAF_WORDS);
    dst[0] = make_uint4(d.plus[0], d.plus[1], d.plus[2], d.plus[3]);
    dst[1] = make_uint4(d.plus[4], d.plus[5], d.plus[6], d.plus[7]);
    dst[2] = make_uint4(d.minus[0], d.minus[1], d.minus[2], d.minus[3]);
    dst[3] = make_uint4(d.minus[4], d.minus[5], d.minus[6], d.minus[7]);
  } else {
    feg_store<Fr>(out + i * Fr::NG, fe_pack(fe_to_gnark(r)));
  }
}

// [k]p for k below the group order, given as its Naf words: double and add +-p
// from the top on complete formulas.  -p is p with y negated in place when the
// digit's sign changes, so no second copy of the point is kept.  UNIFORM: k is
// the same for every lane of the wave; its words go through readfirstlane, so
// the add is a uniform branch.
template <bool UNIFORM, class F>
GM_DEV XYZZ<F> xyzz_mul_naf(XYZZ<F> p, const uint32_t* __restrict__ k) {
  XYZZ<F> acc = xyzz_inf<F>();
  bool neg = false;  // p holds -p
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    uint32_t plus = k[w], minus = k[8 + w];
    if constexpr (UNIFORM) {
      plus = __builtin_amdgcn_readfirstlane(plus);
      minus = __builtin_amdgcn_readfirstlane(minus);
    }
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      acc = xyzz_dbl(acc);
      const bool dm = (minus >> b) & 1;
      if (((plus >> b) & 1) | dm) {
        if (dm != neg) {
          p.y = fe_neg(p.y);
          neg = dm;
        }
        acc = xyzz_add(acc, p);
      }
    }
  }
  return acc;
}

template <class F>
__global__ void __launch_bounds__(256)
    k_ecfft_load(const uint32_t* __restrict__ in, size_t n, XYZZ<F>* __restrict__ pts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> a = load_affine_gnark<F>(in + i * 2 * Coord<F>::WORDS);
  XYZZ<F> r = xyzz_inf<F>();
  if (!aff_is_inf(a)) {
    r.x = a.x;
    r.y = a.y;
    r.zz = FOps<F>::one();
    r.zzz = FOps<F>::one();
  }
  pts[i] = r;
}

// Stage s of the decimation in frequency on n = 2^logn points: butterfly (blk, j),
// j < half = n / 2^(s+1), works on pts[blk 2 half + j] and the point half above
// it with the twiddle tw[j 2^s].  Thread k is butterfly (k % 2^s, k / 2^s),
// twiddle-major: 2^s consecutive k share j, so a wave holds max(1, 64 / 2^s)
// twiddles.  UNIFORM (2^s >= 64): the wave's one twiddle is read as such.
template <class F, bool UNIFORM>
__global__ void __launch_bounds__(ECFFT_TPB)
    k_ecfft_stage(XYZZ<F>* __restrict__ pts, const uint32_t* __restrict__ tw, uint32_t logn, uint32_t s) {
  const size_t k = (size_t)blockIdx.x * ECFFT_TPB + threadIdx.x;
  if (k >= ((size_t)1 << (logn - 1))) return;
  const uint32_t lh = logn - 1 - s;
  const size_t j = k >> s;
  const size_t blk = k & (((size_t)1 << s) - 1);
  const size_t i0 = (blk << (lh + 1)) + j, i1 = i0 + ((size_t)1 << lh);
  const XYZZ<F> a = pts[i0];
  XYZZ<F> b = pts[i1];
  pts[i0] = xyzz_add(a, b);
  b.y = fe_neg(b.y);  // infinity stays infinity (zz = 0)
  XYZZ<F> d = xyzz_add(a, b);
  if (j != 0) d = xyzz_mul_naf<UNIFORM>(d, tw + (j << s) * NAF_WORDS);
  pts[i1] = d;
}

// out[i] = [1/n] pts[brev(i)] as a gnark affine point; ninv: the Naf words of 1/n
template <class F>
__global__ void __launch_bounds__(ECFFT_TPB) k_ecfft_store(const XYZZ<F>* __restrict__ pts, uint32_t logn,
                                                           const uint32_t* __restrict__ ninv,
                                                           uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * ECFFT_TPB + threadIdx.x;
  if (i >= ((size_t)1 << logn)) return;
  const size_t src = brev_bits((uint32_t)i, (int)logn);  // logn <= 30
  const XYZZ<F> acc = xyzz_mul_naf<true>(pts[src], ninv);
  Affine<F> r;
  if (xyzz_is_inf(acc)) {
    r.x = FOps<F>::zero();
    r.y = FOps<F>::zero();
  } else {
    const F t = fe_inv(fe_mul(acc.zz, acc.zzz));
    r.x = fe_mul(acc.x, fe_mul(t, acc.zzz));  // X / ZZ
    r.y = fe_mul(acc.y, fe_mul(t, acc.zz));   // Y / ZZZ
  }
  store_affine_gnark<F>(out + i * 2 * Coord<F>::WORDS, r);
}

// lane t: row t % n of s_(t / n).  coset1, coset2: g and g^2, gnark form.
// IDX: int64 (gnark's trace.S) or u32 (positions from the wire tables).
template <class Fr, class IDX>
__global__ void __launch_bounds__(256)
    k_sigma(const IDX* __restrict__ perm, const uint32_t* __restrict__ wtab, uint32_t logn, FeG<Fr> coset1,
            FeG<Fr> coset2, uint32_t* __restrict__ s1, uint32_t* __restrict__ s2, uint32_t* __restrict__ s3) {
  const size_t n = (size_t)1 << logn;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  const uint64_t v = (uint64_t)perm[t];  // in [0, 3n): checked on the host, or a permutation by construction
  const uint64_t c = v >> logn;
  Fe<Fr> r = fe_load_g<Fr>(wtab, v & (n - 1));
  // gnark form times internal form is gnark form (field.hpp)
  if (c) r = fe_mul(r, fe_to_internal(fe_unpack<Fr>(c == 1 ? coset1 : coset2)));
  uint32_t* const dst = t < n ? s1 : (t < 2 * n ? s2 : s3);
  fe_store_g<Fr>(dst, t & (n - 1), r);
}

template <class HF, class Fr>
FeG<Fr> to_dev(const HF& h) {
  FeG<Fr> r;
  static_assert(sizeof(r.w) == sizeof(h.v), "gnark layout");
  memcpy(r.w, h.v, sizeof(r.w));
  return r;
}

int log2_of(size_t n) {
  int l = 0;
  while (((size_t)1 << l) < n && l < 62) l++;
  return ((size_t)1 << l) == n ? l : -1;
}

int refuse(const std::string& msg) {
  set_error("plonk setup: " + msg);
  return GM_ERR_INVALID;
}

// nothing queued may outlive the call's workspace, also after a failure
struct StreamDrain {
  gm_ctx* ctx;
  ~StreamDrain() {
    hipStreamSynchronize(ctx->stream);
    prof_collect(ctx);
  }
};

template <class C>
int setup_t(gm_ctx* ctx, const gm_plonk_setup_host* in, const gm_plonk_wires* w, const PlonkPkFixed& f,
            unsigned flags, gm_plonk_pk* pk, void* vk_digests, void* srs_lagrange_out) {
  const size_t n = in->n, pb = 2 * fp_bytes(pk->curve);
  int rc;
  {
    // the first n canonical points, transformed where they lie, then prepared
    Arena arena(ctx);
    DevBuf raw;
    if ((rc = raw.alloc(arena, pb * n))) return rc;
    StreamDrain drain{ctx};
    GM_HIP(hipMemcpyAsync(raw.p, in->srs_canonical, pb * n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = kzg_srs_lagrange_device<C>(ctx, raw.p, n, raw.p))) return rc;
    if (srs_lagrange_out)
      GM_HIP(hipMemcpyAsync(srs_lagrange_out, raw.p, pb * n, hipMemcpyDeviceToHost, ctx->stream));
    const hipError_t e = hipMalloc(&pk->srs_lagrange, msm_internal_point_bytes<C, false>() * n);
    if (e != hipSuccess) {
      pk->srs_lagrange = nullptr;
      set_error(std::string("plonk setup: hipMalloc of the Lagrange SRS: ") + hipGetErrorString(e));
      return GM_ERR_OOM;
    }
    if ((rc = msm_prepare_points<C, false>(ctx, raw.p, n, pk->srs_lagrange))) return rc;
  }
  auto lag = [&](size_t k) { return const_cast<void*>(pk->lagrange(k)); };
  rc = w ? plonk_sigma_wires_device<C>(ctx, w, lag(gm_plonk_pk::LAG_S1), lag(gm_plonk_pk::LAG_S2),
                                       lag(gm_plonk_pk::LAG_S3))
         : plonk_sigma_device<C>(ctx, n, in->permutation, lag(gm_plonk_pk::LAG_S1), lag(gm_plonk_pk::LAG_S2),
                                 lag(gm_plonk_pk::LAG_S3));
  if (rc) return rc;
  return plonk_pk_finish(ctx, f, flags, pk, vk_digests);
}

}  // namespace

template <class C>
int kzg_srs_lagrange_device(gm_ctx* ctx, const void* srs_dev, size_t n, void* lagrange_dev) {
  using F = typename C::G1F;
  using Fr = typename C::Fr;
  using HF = host::F<typename C::HFr>;
  const int logn = log2_of(n);
  if (logn < 1 || logn > ecfft_max_logn<C>())
    return refuse("the Lagrange SRS needs n a power of two, 2 <= n <= 2^" + std::to_string(ecfft_max_logn<C>()));
  HF w;
  int rc;
  if ((rc = ntt_root<C>(logn, w.v))) return rc;
  const HF ninv = host::from_mont(host::finv(host::from_u64<typename C::HFr>(n)));
  uint32_t ninv_words[8];
  static_assert(sizeof(ninv_words) == sizeof(ninv.v), "8 u32 words");
  memcpy(ninv_words, ninv.v, sizeof(ninv_words));
  const Naf ninv_naf = naf_of(ninv_words);
  static_assert(sizeof(Naf) == NAF_WORDS * sizeof(uint32_t), "the table's entry");
  const size_t half = n / 2;
  Arena arena(ctx);
  DevBuf pts, tw;
  if ((rc = pts.alloc(arena, sizeof(XYZZ<F>) * n))) return rc;
  // the twiddles w^(-j), j < n / 2, then 1/n
  if ((rc = tw.alloc(arena, sizeof(Naf) * (half + 1)))) return rc;
  uint32_t* const ninv_dev = tw.as<uint32_t>() + NAF_WORDS * half;
  StreamDrain drain{ctx};
  ProfScope ps(ctx, "kzg_srs_lagrange");
  GM_HIP(hipMemcpyAsync(ninv_dev, &ninv_naf, sizeof(ninv_naf), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL((k_powers<Fr, true>), dim3(blocks_for(half, 256)), dim3(256), 0, ctx->stream,
                     tw.as<uint32_t>(), half, to_dev<HF, Fr>(host::finv(w)));
  hipLaunchKernelGGL(k_ecfft_load<F>, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream,
                     (const uint32_t*)srs_dev, n, pts.as<XYZZ<F>>());
  for (uint32_t s = 0; s < (uint32_t)logn; s++) {
    auto k = s >= ECFFT_UNIFORM_STAGE ? k_ecfft_stage<F, true> : k_ecfft_stage<F, false>;
    hipLaunchKernelGGL(k, dim3(blocks_for(half, ECFFT_TPB)), dim3(ECFFT_TPB), 0, ctx->stream, pts.as<XYZZ<F>>(),
                       tw.as<uint32_t>(), (uint32_t)logn, s);
  }
  hipLaunchKernelGGL(k_ecfft_store<F>, dim3(blocks_for(n, ECFFT_TPB)), dim3(ECFFT_TPB), 0, ctx->stream,
                     pts.as<XYZZ<F>>(), (uint32_t)logn, ninv_dev, (uint32_t*)lagrange_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int plonk_perm_check(size_t n, const int64_t* perm) {
  for (size_t i = 0; i < 3 * n; i++)
    if (perm[i] < 0 || (uint64_t)perm[i] >= 3 * n)
      return refuse("permutation[" + std::to_string(i) + "] = " + std::to_string(perm[i]) +
                    " lies outside [0, 3n = " + std::to_string(3 * n) + ")");
  return GM_OK;
}

// perm: 3n int64 on the host (copied into the workspace) or, with w, derived from
// the wire tables on the device as 3n u32
template <class C>
static int sigma_t(gm_ctx* ctx, size_t n, const int64_t* perm_host, const gm_plonk_wires* w, void* s1, void* s2,
                   void* s3) {
  using Fr = typename C::Fr;
  using HF = host::F<typename C::HFr>;
  const int logn = log2_of(n);
  if (logn < 1 || logn > ecfft_max_logn<C>())
    return refuse("sigma needs n a power of two, 2 <= n <= 2^" + std::to_string(ecfft_max_logn<C>()));
  HF wn;
  int rc;
  if ((rc = ntt_root<C>(logn, wn.v))) return rc;
  const HF g = host::from_u64<typename C::HFr>(C::COSET_GEN);
  Arena arena(ctx);
  DevBuf perm, wtab;
  if (!w && (rc = perm.alloc(arena, sizeof(int64_t) * 3 * n))) return rc;
  if ((rc = wtab.alloc(arena, 32 * n))) return rc;
  StreamDrain drain{ctx};
  ProfScope ps(ctx, w ? "plonk_sigma_wires" : "plonk_sigma");
  const uint32_t* perm32 = nullptr;
  if (w) {
    if ((rc = plonk_wires_perm_queue(ctx, arena, w, nullptr, &perm32))) return rc;
  } else {
    GM_HIP(hipMemcpyAsync(perm.p, perm_host, sizeof(int64_t) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
  }
  hipLaunchKernelGGL((k_powers<Fr, false>), dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream,
                     wtab.as<uint32_t>(), n, to_dev<HF, Fr>(wn));
  if (w)
    hipLaunchKernelGGL((k_sigma<Fr, uint32_t>), dim3(blocks_for(3 * n, 256)), dim3(256), 0, ctx->stream, perm32,
                       wtab.as<uint32_t>(), (uint32_t)logn, to_dev<HF, Fr>(g), to_dev<HF, Fr>(g * g), (uint32_t*)s1,
                       (uint32_t*)s2, (uint32_t*)s3);
  else
    hipLaunchKernelGGL((k_sigma<Fr, int64_t>), dim3(blocks_for(3 * n, 256)), dim3(256), 0, ctx->stream,
                       perm.as<int64_t>(), wtab.as<uint32_t>(), (uint32_t)logn, to_dev<HF, Fr>(g),
                       to_dev<HF, Fr>(g * g), (uint32_t*)s1, (uint32_t*)s2, (uint32_t*)s3);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

template <class C>
int plonk_sigma_device(gm_ctx* ctx, size_t n, const int64_t* perm_host, void* s1, void* s2, void* s3) {
  return sigma_t<C>(ctx, n, perm_host, nullptr, s1, s2, s3);
}

template <class C>
int plonk_sigma_wires_device(gm_ctx* ctx, const gm_plonk_wires* w, void* s1, void* s2, void* s3) {
  return sigma_t<C>(ctx, w->n, nullptr, w, s1, s2, s3);
}

static int pk_setup_run(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, const gm_plonk_wires* w,
                        const PlonkPkFixed& f, unsigned flags, gm_plonk_pk** out, void* vk_digests,
                        void* srs_lagrange_out) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  gm_plonk_pk* pk = nullptr;
  int rc = plonk_pk_begin(ctx, curve, f, &pk);
  if (!rc)
    rc = curve == GM_BN254 ? setup_t<CurveBN254>(ctx, in, w, f, flags, pk, vk_digests, srs_lagrange_out)
                           : setup_t<CurveBLS12377>(ctx, in, w, f, flags, pk, vk_digests, srs_lagrange_out);
  if (rc) {
    hipStreamSynchronize(ctx->stream);  // nothing queued may outlive the buffers
    plonk_pk_release(pk);
    return rc;
  }
  *out = pk;
  return GM_OK;
}

int plonk_pk_setup(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, unsigned flags, gm_plonk_pk** out,
                   void* vk_digests, void* srs_lagrange_out) {
  const PlonkPkFixed f = {in->n,      in->nb_public, in->ql, in->qr, in->qm, in->qo, in->qk,
                          in->nb_bsb, in->qcp,       in->commitment_row, in->srs_canonical, in->srs_canonical_len};
  if (int rc = plonk_pk_check(curve, f, flags, false)) return rc;
  if (!in->permutation || !vk_digests) return refuse("the permutation and vk_digests must be non-null");
  if (int rc = plonk_perm_check(in->n, in->permutation)) return rc;
  return pk_setup_run(ctx, curve, in, nullptr, f, flags, out, vk_digests, srs_lagrange_out);
}

int plonk_pk_setup_wires(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, const gm_plonk_wires* w,
                         unsigned flags, gm_plonk_pk** out, void* vk_digests, void* srs_lagrange_out) {
  const PlonkPkFixed f = {in->n,      in->nb_public, in->ql, in->qr, in->qm, in->qo, in->qk,
                          in->nb_bsb, in->qcp,       in->commitment_row, in->srs_canonical, in->srs_canonical_len};
  if (int rc = plonk_pk_check(curve, f, flags, false)) return rc;
  if (!vk_digests) return refuse("vk_digests must be non-null");
  if (in->permutation) return refuse("the permutation comes from the wire tables: in->permutation must be null");
  if (w->ctx != ctx) return refuse("the wire tables were uploaded on another context");
  if (w->n != in->n)
    return refuse("the wire tables have n = " + std::to_string(w->n) + ", the key has n = " + std::to_string(in->n));
  if (w->n > WIRES_PERM_MAX_N) return refuse("the permutation from the wire tables needs n <= 2^30");
  return pk_setup_run(ctx, curve, in, w, f, flags, out, vk_digests, srs_lagrange_out);
}

// The _wires call with nothing dense from the host: sizes, commitment rows and
// tables from the circuit, every selector made by its kernel into the column
// where plonk_pk_finish would copy the host vector.
int plonk_pk_setup_scs(gm_ctx* ctx, const gm_plonk_scs* s, const void* srs_canonical, size_t srs_canonical_len,
                       unsigned flags, gm_plonk_pk** out, void* vk_digests, void* srs_lagrange_out) {
  const PlonkColumnGen gen = {plonk_scs_column, s};
  gm_plonk_setup_host in = {};
  in.n = s->n;
  in.nb_public = s->nb_public;
  in.nb_bsb = s->nb_bsb;
  in.commitment_row = s->commitment_row.data();
  in.srs_canonical = srs_canonical;
  in.srs_canonical_len = srs_canonical_len;
  const PlonkPkFixed f = {in.n,      in.nb_public, nullptr, nullptr, nullptr, nullptr, nullptr,
                          in.nb_bsb, nullptr,      in.commitment_row, in.srs_canonical, in.srs_canonical_len, &gen};
  if (int rc = plonk_pk_check(s->curve, f, flags, false)) return rc;
  if (!vk_digests) return refuse("vk_digests must be non-null");
  if (s->ctx != ctx) return refuse("the circuit was uploaded on another context");
  if (s->n > WIRES_PERM_MAX_N) return refuse("the permutation from the wire tables needs n <= 2^30");
  return pk_setup_run(ctx, s->curve, &in, &s->wires, f, flags, out, vk_digests, srs_lagrange_out);
}

#define GM_SETUP_INST(C)                                                                     \
  template int kzg_srs_lagrange_device<C>(gm_ctx*, const void*, size_t, void*);               \
  template int plonk_sigma_device<C>(gm_ctx*, size_t, const int64_t*, void*, void*, void*);     \
  template int plonk_sigma_wires_device<C>(gm_ctx*, const gm_plonk_wires*, void*, void*, void*);
GM_SETUP_INST(CurveBN254)
GM_SETUP_INST(CurveBLS12377)

}  // namespace gm
