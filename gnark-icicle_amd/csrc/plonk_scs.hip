// A PLONK constraint system resident on the device: the PLONK twin of r1cs.hip.
// gnark holds a compiled circuit as []SparseR1C (constraint/r1cs_sparse.go:143-147:
// XA XB XC QL QR QO QM QC Commitment, nine u32), a CoeffTable and the commitment
// info.  Everything NewTrace (backend/plonk/bls12-377/setup.go:153-213) derives
// from them is a function of that data, so it goes up once, 36 bytes per
// constraint, and is split on the device into
//   * the wire tables of evaluateLROSmallDomain, in gm_plonk_wires' layout: rows
//     (i, 0, 0) for the public inputs, the constraints from row nb_public on,
//     (0, 0, 0) padding;
//   * five columns of coefficient ids, one byte of Commitment per constraint;
//   * the CoeffTable and the committed rows of every BSB22 gate.
// From these: a selector column per launch (k_scs_selector, a gather of 32-byte
// words shaped like k_gather_lro), the proving key (plonk_setup.hip, through
// plonk_pk_finish's column source) and the gate equation on a witness
// (k_scs_check).  No field arithmetic but in the check; the curve enters the
// selectors only as the Montgomery words of -1 and 1.
#include <algorithm>
#include <string>
#include <vector>

#include "curves.hpp"
#include "plonk_scs.hpp"
#include "runtime.hpp"

namespace gm {

void plonk_scs_release(gm_plonk_scs* s) {
  if (!s) return;
  if (s->ctx) {
    auto& v = s->ctx->plonk_scs;
    v.erase(std::remove(v.begin(), v.end(), s), v.end());
    hipSetDevice(s->ctx->device);
  }
  if (s->buf) hipFree(s->buf);
  delete s;
}

namespace {

constexpr unsigned SCS_TPB = 256;  // the block of grid_for (runtime.hpp)
constexpr unsigned REC_WORDS = 9;  // XA XB XC QL QR QO QM QC Commitment
// SparseR1C.Commitment (constraint/r1cs_sparse.go): NOT, COMMITTED, COMMITMENT
constexpr uint32_t COMMITMENT_NOT = 0, COMMITMENT_MAX = 2;

// A tile of 256 records goes through LDS: the block reads its 2304 words in
// order (coalesced u32), then lane t takes record t and writes one entry of each
// column, so every column store is contiguous over the block.  Record t starts
// at word 9 t: an odd stride, no two lanes of a wave on one bank.  After the
// tiles the rows outside the constraints: (k, 0, 0) for k < nb_public, (0, 0, 0)
// from nb_public + nc on.  The caller has checked nb_public + nc <= n.
__global__ void __launch_bounds__(SCS_TPB)
    k_scs_split(const uint32_t* __restrict__ rec, size_t nc, size_t n, size_t nb_public, size_t stride,
                uint32_t* __restrict__ tab, uint32_t* __restrict__ cid, uint8_t* __restrict__ commitment) {
  __shared__ uint32_t tile[SCS_TPB * REC_WORDS];
  const size_t tiles = (nc + SCS_TPB - 1) / SCS_TPB;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const size_t base = t * SCS_TPB;
    const size_t cnt = nc - base < SCS_TPB ? nc - base : SCS_TPB;
    const unsigned words = (unsigned)cnt * REC_WORDS;
    for (unsigned k = threadIdx.x; k < words; k += SCS_TPB) tile[k] = rec[base * REC_WORDS + k];
    __syncthreads();
    if (threadIdx.x < cnt) {
      const uint32_t* r = tile + threadIdx.x * REC_WORDS;
      const size_t i = base + threadIdx.x, row = nb_public + i;
      tab[row] = r[0];
      tab[n + row] = r[1];
      tab[2 * n + row] = r[2];
      cid[GM_SCS_QL * stride + i] = r[3];
      cid[GM_SCS_QR * stride + i] = r[4];
      cid[GM_SCS_QO * stride + i] = r[5];
      cid[GM_SCS_QM * stride + i] = r[6];
      cid[GM_SCS_QK * stride + i] = r[7];
      commitment[i] = (uint8_t)r[8];
    }
    __syncthreads();
  }
  const size_t lanes = (size_t)gridDim.x * SCS_TPB;
  for (size_t k = (size_t)blockIdx.x * SCS_TPB + threadIdx.x; k < n - nc; k += lanes) {
    const size_t row = k < nb_public ? k : k + nc;
    tab[row] = k < nb_public ? (uint32_t)k : 0u;
    tab[n + row] = 0;
    tab[2 * n + row] = 0;
  }
}

// one 32-byte element as its two 16-byte halves
struct Halves {
  uint4 lo, hi;
};

// lane t: half t & 1 of row t >> 1.  cid != nullptr: a coefficient column,
// coeffs[cid[row - nb_public]] on the constraint rows, `pub` on the public rows (-1
// for QL, 0 otherwise), 0 on the padding.  cid == nullptr: a qcp column, `one` on
// the rows found in the ascending list rows[0, nrows), 0 elsewhere.
__global__ void __launch_bounds__(SCS_TPB)
    k_scs_selector(const uint32_t* __restrict__ cid, const uint4* __restrict__ coeffs,
                   const uint32_t* __restrict__ rows, size_t nrows, size_t n, size_t nb_public, size_t nc, Halves pub,
                   Halves one, uint4* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * SCS_TPB;
  for (size_t t = (size_t)blockIdx.x * SCS_TPB + threadIdx.x; t < 2 * n; t += stride) {
    const size_t row = t >> 1, half = t & 1;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (cid) {
      if (row < nb_public) v = half ? pub.hi : pub.lo;
      else if (row - nb_public < nc) v = coeffs[2 * (size_t)cid[row - nb_public] + half];
    } else {
      size_t lo = 0, hi = nrows;
      while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        if (rows[mid] < row) lo = mid + 1;
        else hi = mid;
      }
      if (lo < nrows && rows[lo] == row) v = half ? one.hi : one.lo;
    }
    out[t] = v;
  }
}

// One lane per constraint: ql l + qr r + qm l r + qo o + qk on canonical operands.
// The wires go to internal form once; a coefficient in gnark form times a wire in
// internal form is the product in gnark form (field.hpp), qk is added as it is,
// and zero is zero in every form.  A wave counts its failures with one atomicAdd
// (ballot + popcount) by its lowest failing lane, whose constraint is the wave's
// smallest and goes to the atomicMin.
template <class Fr>
__global__ void __launch_bounds__(SCS_TPB)
    k_scs_check(const uint32_t* __restrict__ tab, size_t n, size_t nb_public, size_t nc,
                const uint32_t* __restrict__ cid, size_t stride, const uint8_t* __restrict__ commitment,
                const void* __restrict__ coeffs, const void* __restrict__ witness,
                unsigned long long* __restrict__ result) {
  const size_t i = (size_t)blockIdx.x * SCS_TPB + threadIdx.x;
  bool fail = false;
  if (i < nc && commitment[i] == COMMITMENT_NOT) {
    const size_t row = nb_public + i;
    const Fe<Fr> l = fe_to_internal(fe_load_g<Fr>(witness, tab[row]));
    const Fe<Fr> r = fe_to_internal(fe_load_g<Fr>(witness, tab[n + row]));
    const Fe<Fr> o = fe_to_internal(fe_load_g<Fr>(witness, tab[2 * n + row]));
    auto q = [&](unsigned which) { return fe_load_g<Fr>(coeffs, cid[which * stride + i]); };
    Fe<Fr> acc = fe_mul(q(GM_SCS_QL), l);
    acc = fe_add(acc, fe_mul(q(GM_SCS_QR), r));
    acc = fe_add(acc, fe_mul(fe_mul(q(GM_SCS_QM), l), r));
    acc = fe_add(acc, fe_mul(q(GM_SCS_QO), o));
    acc = fe_add(acc, q(GM_SCS_QK));
    fail = !fe_is_zero(acc);
  }
  const unsigned long long mask = __ballot(fail);
  if (mask && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)mask) - 1)) {
    atomicAdd(result, (unsigned long long)__popcll(mask));
    atomicMin(result + 1, (unsigned long long)i);
  }
}

int refuse(const std::string& msg) {
  set_error("plonk scs: " + msg);
  return GM_ERR_INVALID;
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

template <class C>
Halves mont_words(bool minus) {
  using HF = host::F<typename C::HFr>;
  const HF one = host::from_u64<typename C::HFr>(1);
  const HF v = minus ? -one : one;
  static_assert(sizeof(v.v) == sizeof(Halves), "a 32-byte gnark element");
  Halves h;
  memcpy(&h, v.v, sizeof(h));
  return h;
}

// nothing queued may outlive the call's workspace, also after a failure
struct StreamDrain {
  gm_ctx* ctx;
  ~StreamDrain() {
    hipStreamSynchronize(ctx->stream);
    prof_collect(ctx);
  }
};

}  // namespace

int plonk_scs_upload(gm_ctx* ctx, int curve, const gm_plonk_scs_host* h, gm_plonk_scs** out) {
  const size_t n = h->n, nc = h->nb_constraints, nb = h->nb_bsb;
  if (!h->coeffs || (nc && !h->records)) return refuse("gm_plonk_scs_upload: a required pointer is NULL");
  if (nb && (!h->committed || !h->committed_len || !h->commitment_index))
    return refuse("gm_plonk_scs_upload: nb_bsb > 0 needs committed, committed_len and commitment_index");
  if (n < 8 || (n & (n - 1)) || n > (size_t(1) << 30)) return refuse("n must be a power of two, 8 <= n <= 2^30");
  if (h->nb_public > n || nc > n - h->nb_public)
    return refuse("n = " + std::to_string(n) + " is too small for nb_public + nb_constraints = " +
                  std::to_string(h->nb_public) + " + " + std::to_string(nc) + " rows");
  if (h->nb_wires == 0 || h->nb_wires > 0xffffffffull) return refuse("nb_wires must lie in [1, 2^32 - 1]");
  if (h->nb_wires < h->nb_public)
    return refuse("nb_wires = " + std::to_string(h->nb_wires) + " is below nb_public = " +
                  std::to_string(h->nb_public));
  if (h->ncoeffs < 2) return refuse("the CoeffTable holds at least zero and one (ncoeffs >= 2)");
  if (nb > 1024) return refuse("nb_bsb > 1024");
  static const char* const names[REC_WORDS] = {"XA", "XB", "XC", "QL", "QR", "QO", "QM", "QC", "Commitment"};
  for (size_t i = 0; i < nc; i++) {
    const uint32_t* r = h->records + i * REC_WORDS;
    for (unsigned k = 0; k < REC_WORDS; k++) {
      const size_t bound = k < 3 ? h->nb_wires : (k < 8 ? h->ncoeffs : COMMITMENT_MAX + 1);
      if (r[k] >= bound)
        return refuse("record " + std::to_string(i) + ": " + names[k] + " = " + std::to_string(r[k]) +
                      (k < 3   ? " is not below nb_wires = " + std::to_string(h->nb_wires)
                       : k < 8 ? " is not below ncoeffs = " + std::to_string(h->ncoeffs)
                               : std::string(" is no CommitmentConstraint (0, 1 or 2)")));
    }
  }
  std::vector<size_t> off(nb + 1, 0), crow(nb);
  for (size_t j = 0; j < nb; j++) {
    if (h->committed_len[j] && !h->committed[j])
      return refuse("gm_plonk_scs_upload: committed[" + std::to_string(j) + "] is NULL");
    for (size_t k = 0; k < h->committed_len[j]; k++)
      if (h->committed[j][k] >= nc)
        return refuse("committed[" + std::to_string(j) + "][" + std::to_string(k) + "] = " +
                      std::to_string(h->committed[j][k]) + " is not below nb_constraints = " + std::to_string(nc));
    if (h->commitment_index[j] >= nc)
      return refuse("commitment_index[" + std::to_string(j) + "] = " + std::to_string(h->commitment_index[j]) +
                    " is not below nb_constraints = " + std::to_string(nc));
    off[j + 1] = off[j] + h->committed_len[j];
    crow[j] = h->nb_public + h->commitment_index[j];
  }
  // the committed rows as the selector kernel searches them
  std::vector<uint32_t> rows(off[nb]);
  for (size_t j = 0; j < nb; j++) {
    for (size_t k = 0; k < h->committed_len[j]; k++) rows[off[j] + k] = (uint32_t)(h->nb_public + h->committed[j][k]);
    std::sort(rows.begin() + off[j], rows.begin() + off[j + 1]);
  }

  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  gm_plonk_scs* s = new gm_plonk_scs;
  s->curve = curve;
  s->n = n;
  s->nb_public = h->nb_public;
  s->nb_constraints = nc;
  s->nb_wires = h->nb_wires;
  s->ncoeffs = h->ncoeffs;
  s->nb_bsb = nb;
  s->committed_off = off;
  s->commitment_row = crow;
  s->stride = align256(std::max<size_t>(nc, 1) * sizeof(uint32_t)) / sizeof(uint32_t);
  const size_t o_cid = align256(3 * n * sizeof(uint32_t));
  const size_t o_coeffs = o_cid + 5 * s->stride * sizeof(uint32_t);
  const size_t o_rows = o_coeffs + align256(32 * h->ncoeffs);
  const size_t o_commitment = o_rows + align256(std::max<size_t>(rows.size(), 1) * sizeof(uint32_t));
  s->bytes = o_commitment + align256(std::max<size_t>(nc, 1));
  const hipError_t e = hipMalloc((void**)&s->buf, s->bytes);
  if (e != hipSuccess) {
    set_error(std::string("plonk scs: hipMalloc(") + std::to_string(s->bytes) + "): " + hipGetErrorString(e));
    delete s;
    return GM_ERR_OOM;
  }
  s->cid = (uint32_t*)(s->buf + o_cid);
  s->coeffs = s->buf + o_coeffs;
  s->committed = (uint32_t*)(s->buf + o_rows);
  s->commitment = (uint8_t*)(s->buf + o_commitment);
  s->wires.n = n;
  s->wires.nb_wires = h->nb_wires;
  s->wires.tab = (uint32_t*)s->buf;
  s->wires.borrowed = true;
  int rc = GM_OK;
  {
    Arena arena(ctx);
    DevBuf rec;
    StreamDrain drain{ctx};  // no host pointer is read after the call returns
    auto copy = [&](void* dst, const void* src, size_t bytes) {
      if (rc == GM_OK && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        set_error("plonk scs: an upload failed");
        rc = GM_ERR_DEVICE;
      }
    };
    rc = rec.alloc(arena, REC_WORDS * sizeof(uint32_t) * std::max<size_t>(nc, 1));
    copy(rec.p, h->records, REC_WORDS * sizeof(uint32_t) * nc);
    copy(s->coeffs, h->coeffs, 32 * h->ncoeffs);
    copy(s->committed, rows.data(), rows.size() * sizeof(uint32_t));
    if (rc == GM_OK) {
      ProfScope ps(ctx, "plonk_scs_split");
      hipLaunchKernelGGL(k_scs_split, dim3(grid_for(std::max(nc, n - nc))), dim3(SCS_TPB), 0, ctx->stream,
                         rec.as<uint32_t>(), nc, n, s->nb_public, s->stride, s->wires.tab, s->cid, s->commitment);
      if (hipGetLastError() != hipSuccess) {
        set_error("plonk scs: the split kernel could not be launched");
        rc = GM_ERR_DEVICE;
      }
    }
  }
  if (rc) {
    plonk_scs_release(s);
    return rc;
  }
  s->ctx = ctx;
  s->wires.ctx = ctx;
  ctx->plonk_scs.push_back(s);
  *out = s;
  return GM_OK;
}

int plonk_scs_selector_device(gm_ctx* ctx, const gm_plonk_scs* s, unsigned which, void* out_dev) {
  const bool bn = s->curve == GM_BN254;
  const Halves zero = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
  const Halves one = bn ? mont_words<CurveBN254>(false) : mont_words<CurveBLS12377>(false);
  const Halves pub =
      which != GM_SCS_QL ? zero : (bn ? mont_words<CurveBN254>(true) : mont_words<CurveBLS12377>(true));
  const uint32_t* cid = nullptr;
  const uint32_t* rows = nullptr;
  size_t nrows = 0;
  if (which < GM_SCS_QCP0) {
    cid = s->cid + which * s->stride;
  } else {
    const size_t j = which - GM_SCS_QCP0;
    rows = s->committed + s->committed_off[j];
    nrows = s->committed_off[j + 1] - s->committed_off[j];
  }
  ProfScope ps(ctx, "plonk_scs_selector");
  hipLaunchKernelGGL(k_scs_selector, dim3(grid_for(2 * s->n)), dim3(SCS_TPB), 0, ctx->stream, cid,
                     (const uint4*)s->coeffs, rows, nrows, s->n, s->nb_public, s->nb_constraints, pub, one,
                     (uint4*)out_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int plonk_scs_column(gm_ctx* ctx, const void* scs, unsigned which, void* out_dev) {
  return plonk_scs_selector_device(ctx, (const gm_plonk_scs*)scs, which, out_dev);
}

int plonk_scs_selector(gm_ctx* ctx, const gm_plonk_scs* s, unsigned which, void* out_dev) {
  if (s->ctx != ctx) return refuse("the circuit was uploaded on another context");
  if (which >= GM_SCS_QCP0 + s->nb_bsb)
    return refuse("selector " + std::to_string(which) + " of a circuit with " + std::to_string(s->nb_bsb) +
                  " commitments (GM_SCS_QL .. GM_SCS_QCP0 + nb_bsb - 1)");
  const uintptr_t a = (uintptr_t)out_dev, b = (uintptr_t)s->buf;
  if (a % 16) return refuse("the output must be 16-byte aligned");
  if (a < b + s->bytes && b < a + 32 * s->n) return refuse("the output overlaps the circuit");
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const int rc = plonk_scs_selector_device(ctx, s, which, out_dev);
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return rc;
}

int plonk_scs_check_device(gm_ctx* ctx, const gm_plonk_scs* s, const void* witness_dev,
                           unsigned long long* result_dev) {
  static const unsigned long long init[2] = {0ull, ~0ull};
  GM_HIP(hipMemcpyAsync(result_dev, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
  if (s->nb_constraints == 0) return GM_OK;
  ProfScope ps(ctx, "plonk_scs_check");
  const dim3 grid(blocks_for(s->nb_constraints, SCS_TPB)), block(SCS_TPB);
  if (s->curve == GM_BN254)
    hipLaunchKernelGGL(k_scs_check<Bn254Fr>, grid, block, 0, ctx->stream, s->wires.tab, s->n, s->nb_public,
                       s->nb_constraints, s->cid, s->stride, s->commitment, s->coeffs, witness_dev, result_dev);
  else
    hipLaunchKernelGGL(k_scs_check<Bls377Fr>, grid, block, 0, ctx->stream, s->wires.tab, s->n, s->nb_public,
                       s->nb_constraints, s->cid, s->stride, s->commitment, s->coeffs, witness_dev, result_dev);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int plonk_scs_check(gm_ctx* ctx, const gm_plonk_scs* s, const void* witness_host, size_t* nb_unsatisfied,
                    size_t* first_unsatisfied) {
  if (s->ctx != ctx) return refuse("the circuit was uploaded on another context");
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  unsigned long long got[2] = {0, 0};
  {
    Arena arena(ctx);
    DevBuf wit, res;
    int rc;
    if ((rc = wit.alloc(arena, 32 * s->nb_wires))) return rc;
    if ((rc = res.alloc(arena, sizeof(got)))) return rc;
    StreamDrain drain{ctx};
    GM_HIP(hipMemcpyAsync(wit.p, witness_host, 32 * s->nb_wires, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = plonk_scs_check_device(ctx, s, wit.p, res.as<unsigned long long>()))) return rc;
    GM_HIP(hipMemcpyAsync(got, res.p, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    GM_HIP(hipStreamSynchronize(ctx->stream));
  }
  *nb_unsatisfied = (size_t)got[0];
  if (got[0] && first_unsatisfied) *first_unsatisfied = (size_t)got[1];
  return GM_OK;
}

}  // namespace gm
