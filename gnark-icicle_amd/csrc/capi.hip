// C-ABI implementation (include/gnark_mi355x.h): context, memory, MSM, KZG,
// NTT / computeH, host group helpers and synthetic inputs.  The Groth16 prover
// entry points live in groth16.hip.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <string>
#include <vector>

#include "curves.hpp"
#include "g16_setup.hpp"
#include "groth16.hpp"
#include "kzg.hpp"
#include "plonk.hpp"
#include "plonk_lin.hpp"
#include "plonk_perm.hpp"
#include "plonk_pk.hpp"
#include "plonk_session.hpp"
#include "plonk_setup.hpp"
#include "plonk_scs.hpp"
#include "plonk_verify.hpp"
#include "plonk_wires.hpp"
#include "plonk_wires_perm.hpp"
#include "points_check.hpp"
#include "points_codec.hpp"
#include "msm.hpp"
#include "ntt.hpp"
#include "pairing.hpp"
#include "runtime.hpp"

namespace gm {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
std::string last_error() { return g_last_error; }

// ---------------------------------------------------------------------------
// synthetic-input kernels (bench / tests)
// ---------------------------------------------------------------------------
GM_DEV uint64_t splitmix64(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// n Montgomery (gnark-layout) scalars: random canonical value below 2^BITS,
// reduced once (2^BITS < 2r for every scalar field), then x*Rg.
template <class Fr>
__global__ void k_random_scalars(uint32_t* out, size_t n, uint64_t seed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t st = seed ^ (0xD1B54A32D192ED03ull * (i + 1));
  FeG<Fr> g;
  for (int q = 0; q < Fr::NG / 2; q++) {
    uint64_t v = splitmix64(st);
    g.w[2 * q] = (uint32_t)v;
    g.w[2 * q + 1] = (uint32_t)(v >> 32);
  }
  const int top = Fr::BITS - 32 * (Fr::NG - 1);
  g.w[Fr::NG - 1] &= (top >= 32) ? 0xffffffffu : ((1u << top) - 1);
  Fe<Fr> k = fe_unpack<Fr>(g);
  fe_reduce_once(k);
  feg_store<Fr>(out + i * Fr::NG, fe_pack(fe_canonical_to_gnark(k)));
}

// gnark-layout affine point passed by value
template <class F>
struct GPoint {
  uint32_t w[2 * Coord<F>::WORDS];
};

// out[i] = [k_i] base (gnark-layout affine), double-and-add over the canonical scalar.
template <class Fr, class F>
__global__ void __launch_bounds__(128) k_batch_mul_base(const uint32_t* __restrict__ scalars,
                                                        size_t n, GPoint<F> base_g,
                                                        uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const FeG<Fr> k = fe_pack(fe_gnark_to_canonical(fe_load_g<Fr>(scalars, i)));
  const Affine<F> base = load_affine_gnark<F>(base_g.w);
  XYZZ<F> acc = xyzz_inf<F>();
  for (int w = Fr::NG - 1; w >= 0; w--) {
    for (int b = 31; b >= 0; b--) {
      acc = xyzz_dbl(acc);
      if ((k.w[w] >> b) & 1) xyzz_add_aff(acc, base);
    }
  }
  Affine<F> r;
  if (xyzz_is_inf(acc)) {
    r.x = FOps<F>::zero();
    r.y = FOps<F>::zero();
  } else {
    F t = fe_inv(fe_mul(acc.zz, acc.zzz));
    r.x = fe_mul(acc.x, fe_mul(t, acc.zzz));  // X / ZZ
    r.y = fe_mul(acc.y, fe_mul(t, acc.zz));   // Y / ZZZ
  }
  store_affine_gnark<F>(out + i * 2 * Coord<F>::WORDS, r);
}

// ---------------------------------------------------------------------------
// dispatch helpers
// ---------------------------------------------------------------------------
template <class C, bool G2>
static int msm_to_host(gm_ctx* ctx, const void* sc, const void* pts, size_t n, void* out_jac,
                       void* out_aff) {
  using HF = typename GroupSel<C, G2>::HF;
  HF j[3];
  int rc = msm_device<C, G2>(ctx, sc, pts, n, j);
  if (rc) return rc;
  if (out_jac) memcpy(out_jac, j, sizeof(j));
  if (out_aff) {
    host::Aff<HF> a = host::to_aff(host::Jac<HF>{j[0], j[1], j[2]});
    memcpy(out_aff, &a, sizeof(a));
  }
  return GM_OK;
}

int check_curve(int curve, CurveCaps caps, const char* entry) {
  if (curve < 0 || curve >= CURVE_COUNT) {
    set_error("unknown curve id");
    return GM_ERR_INVALID;
  }
  if (curve == CurveBLS12381::id && caps != CURVES_ALL) {
    set_error(std::string(entry) + ": not built for " + curve_name(curve) + " (curve id " + std::to_string(curve) +
              ")");
    return GM_ERR_UNSUPPORTED;
  }
  return GM_OK;
}

size_t fp_bytes(int curve) {
  static constexpr size_t t[CURVE_COUNT] = {sizeof(CurveBN254::HG1F), sizeof(CurveBLS12377::HG1F),
                                            sizeof(CurveBLS12381::HG1F)};
  return curve >= 0 && curve < CURVE_COUNT ? t[curve] : 0;
}

// bytes of one device-internal point of a prepared set (0 for an unknown id)
static size_t internal_point_bytes(int curve, int g2) {
  return with_curve(
      curve,
      [&](auto tag_) {
        using C = typename decltype(tag_)::type;
        return g2 ? msm_internal_point_bytes<C, true>() : msm_internal_point_bytes<C, false>();
      },
      (size_t)0);
}

void orphan_pending_msms(gm_ctx* ctx);  // below gm_msm_pending

}  // namespace gm

using namespace gm;

extern "C" {

const char* gm_last_error(void) { return g_last_error.c_str(); }
int gm_version(void) { return 2; }

int gm_device_count(int* count) {
  if (!count) return GM_ERR_INVALID;
  GM_HIP(hipGetDeviceCount(count));
  return GM_OK;
}

int gm_init(int device, gm_ctx** out) {
  if (!out) return GM_ERR_INVALID;
  int ndev = 0;
  GM_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) {
    set_error("gm_init: device index out of range");
    return GM_ERR_INVALID;
  }
  GM_HIP(hipSetDevice(device));
  auto* c = new gm_ctx();
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking);
  if (e != hipSuccess) {
    set_error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
    delete c;
    return GM_ERR_DEVICE;
  }
  *out = c;
  return GM_OK;
}

int gm_destroy(gm_ctx* ctx) {
  if (!ctx) return GM_OK;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  if (ctx->aux) hipStreamSynchronize(ctx->aux);
  if (ctx->copy) hipStreamSynchronize(ctx->copy);
  for (hipStream_t s : ctx->slot_stream)
    if (s) hipStreamSynchronize(s);
  if (ctx->g16_stream) hipStreamSynchronize(ctx->g16_stream);
  orphan_pending_msms(ctx);
  // stages parked with keys of this context (their keys may outlive it)
  while (!ctx->spare_keys.empty()) stage_spare_release(ctx->spare_keys.back());
  while (!ctx->plonk_spare_keys.empty()) plonk_spare_release(ctx->plonk_spare_keys.back());
  while (!ctx->plonk_wires.empty()) plonk_wires_release(ctx->plonk_wires.back());  // wire tables not freed
  while (!ctx->plonk_scs.empty()) plonk_scs_release(ctx->plonk_scs.back());        // circuits not freed
  for (auto& pr : ctx->pending_reads) hipEventDestroy(pr.second);
  ctx->pending_reads.clear();
  ntt_domains_free(ctx);
  std::vector<gm::ArenaState*> arenas{&ctx->arena};
  for (gm::ArenaState& sa : ctx->slots) arenas.push_back(&sa);
  for (gm::ArenaState* a : arenas) {
    for (auto& ch : a->chunks) hipFree(ch.base);
    a->chunks.clear();
  }
  for (void* p : ctx->tail_pinned)
    if (p) hipHostFree(p);
  for (auto e : ctx->event_pool) hipEventDestroy(e);
  for (auto& p : ctx->pending) {
    hipEventDestroy(p.a);
    hipEventDestroy(p.b);
  }
  for (hipStream_t s : ctx->slot_stream)
    if (s) hipStreamDestroy(s);
  if (ctx->g16_stream) hipStreamDestroy(ctx->g16_stream);
  if (ctx->acc_tail) hipEventDestroy(ctx->acc_tail);
  if (ctx->stamp_dev) hipFree(ctx->stamp_dev);
  hipStreamDestroy(ctx->stream);
  if (ctx->aux) hipStreamDestroy(ctx->aux);
  if (ctx->copy) hipStreamDestroy(ctx->copy);
  if (ctx->pinned) hipHostFree(ctx->pinned);
  if (ctx->in_abc) hipFree(ctx->in_abc);
  for (int i = 0; i < gm_ctx::H2D_SLOTS; i++) {
    if (ctx->h2d_pin[i]) hipHostFree(ctx->h2d_pin[i]);
    if (ctx->h2d_ev[i]) hipEventDestroy(ctx->h2d_ev[i]);
  }
  delete ctx;
  return GM_OK;
}

int gm_trim(gm_ctx* ctx) {
  if (!ctx) return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  if (!ctx->live_msms.empty()) {
    set_error("gm_trim: MSMs are pending on this context (gm_msm_wait them first)");
    return GM_ERR_INVALID;
  }
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->aux) GM_HIP(hipStreamSynchronize(ctx->aux));
  if (ctx->copy) GM_HIP(hipStreamSynchronize(ctx->copy));
  for (hipStream_t st : ctx->slot_stream)
    if (st) GM_HIP(hipStreamSynchronize(st));
  if (ctx->g16_stream) GM_HIP(hipStreamSynchronize(ctx->g16_stream));
  std::vector<gm::ArenaState*> arenas{&ctx->arena};
  for (gm::ArenaState& sa : ctx->slots) arenas.push_back(&sa);
  for (gm::ArenaState* a : arenas) {
    for (auto& ch : a->chunks) hipFree(ch.base);
    a->chunks.clear();
    a->cur_chunk = a->cur_top = 0;
  }
  if (ctx->in_abc) hipFree(ctx->in_abc);
  ctx->in_abc = nullptr;
  ctx->in_abc_cap = 0;
  while (!ctx->spare_keys.empty()) stage_spare_release(ctx->spare_keys.back());  // parked stages
  while (!ctx->plonk_spare_keys.empty()) plonk_spare_release(ctx->plonk_spare_keys.back());  // session buffers
  for (int i = 0; i < gm_ctx::H2D_SLOTS; i++) {
    if (ctx->h2d_pin[i]) hipHostFree(ctx->h2d_pin[i]);
    ctx->h2d_pin[i] = nullptr;
  }
  ntt_domains_free(ctx);
  return GM_OK;
}

int gm_synchronize(gm_ctx* ctx) {
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return GM_OK;
}

int gm_profile_enable(gm_ctx* ctx, int on) {
  gm::CtxLock g(ctx);
  ctx->profiling = on != 0;
  if (ctx->profiling) {
    GM_HIP(hipSetDevice(ctx->device));
    gm::stamp_ensure(ctx);  // best effort: without the ring only the event brackets are recorded
    (void)hipGetLastError();
  }
  return GM_OK;
}
int gm_profile_reset(gm_ctx* ctx) {
  gm::CtxLock g(ctx);
  hipStreamSynchronize(ctx->stream);
  prof_collect(ctx);
  stamp_collect(ctx);
  ctx->stats.clear();
  return GM_OK;
}
int gm_profile_get(gm_ctx* ctx, const char* name, double* total_ms, uint64_t* count) {
  gm::CtxLock g(ctx);
  hipStreamSynchronize(ctx->stream);
  prof_collect(ctx);
  stamp_collect(ctx);
  auto it = ctx->stats.find(name);
  if (it == ctx->stats.end()) {
    *total_ms = 0;
    *count = 0;
    return GM_OK;
  }
  *total_ms = it->second.total_ms;
  *count = it->second.count;
  return GM_OK;
}
int gm_profile_dump(gm_ctx* ctx, char* buf, size_t cap) {
  gm::CtxLock g(ctx);
  hipStreamSynchronize(ctx->stream);
  prof_collect(ctx);
  stamp_collect(ctx);
  std::string s;
  for (auto& kv : ctx->stats)
    s += kv.first + " " + std::to_string(kv.second.total_ms) + " " + std::to_string(kv.second.count) + "\n";
  if (cap) {
    size_t m = std::min(cap - 1, s.size());
    memcpy(buf, s.data(), m);
    buf[m] = 0;
  }
  return GM_OK;
}
int gm_set_msm_window(gm_ctx* ctx, int c) {
  if (c != 0 && (c < 2 || c > 24)) return GM_ERR_INVALID;
  ctx->msm_c_override = c;
  return GM_OK;
}

int gm_set_msm_glv(gm_ctx* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  ctx->msm_glv = mode;
  return GM_OK;
}

int gm_set_msm_piece_len(gm_ctx* ctx, int t) {
  if (!ctx || t < 0 || t > (int)gm::PIECE_MAX_LEN) return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  ctx->msm_piece_len = t;
  return GM_OK;
}

// ---- memory -----------------------------------------------------------------
int gm_malloc(gm_ctx* ctx, size_t bytes, void** dev_out) {
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  hipError_t e = hipMalloc(dev_out, bytes ? bytes : 16);
  if (e != hipSuccess) {
    set_error(std::string("hipMalloc: ") + hipGetErrorString(e));
    return GM_ERR_OOM;
  }
  return GM_OK;
}
int gm_free(gm_ctx* ctx, void* dev) {
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  GM_HIP(hipFree(dev));
  return GM_OK;
}
int gm_memcpy_h2d(gm_ctx* ctx, void* dev, const void* host, size_t bytes) {
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}
int gm_memcpy_d2h(gm_ctx* ctx, void* host, const void* dev, size_t bytes) {
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}
int gm_memcpy_d2d(gm_ctx* ctx, void* dst, const void* src, size_t bytes) {
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}
int gm_copy_to_device(gm_ctx* ctx, const void* host, size_t bytes, void** dev_out) {
  int rc = gm_malloc(ctx, bytes, dev_out);
  if (rc) return rc;
  return gm_memcpy_h2d(ctx, *dev_out, host, bytes);
}
int gm_copy_points_to_device(gm_ctx* ctx, int curve, int g2, const void* host_points, size_t n,
                             void** dev_out) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_copy_points_to_device")) return rc;
  return gm_copy_to_device(ctx, host_points, n * fp_bytes(curve) * (g2 ? 4 : 2), dev_out);
}

// ---- MSM ------------------------------------------------------------------------
int gm_msm(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* points_dev,
           size_t n, void* out_jac, void* out_affine) {
  if (!ctx) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_msm")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const int rc = GM_CURVE(curve, g2 ? msm_to_host<C, true>(ctx, scalars_dev, points_dev, n, out_jac, out_affine)
                                    : msm_to_host<C, false>(ctx, scalars_dev, points_dev, n, out_jac, out_affine));
  prof_collect(ctx);
  return rc;
}

}  // extern "C"

// Piece length of the G1 accumulation (MsmPlan, msm.hpp) for a plan of at most
// M entries: the same size split as the G2 slice length K (msm_launch).  The
// values are the measured ones (profiles/piece_plan_ab.txt).
#ifndef GM_PIECE_LEN_SMALL
#define GM_PIECE_LEN_SMALL 48
#endif
#ifndef GM_PIECE_LEN_LARGE
#define GM_PIECE_LEN_LARGE 64
#endif
uint32_t gm::msm_piece_len(const gm_ctx* ctx, size_t M) {
  if (ctx && ctx->msm_piece_len > 0) return (uint32_t)ctx->msm_piece_len;
  return M <= (size_t(1) << 25) ? GM_PIECE_LEN_SMALL : GM_PIECE_LEN_LARGE;
}

bool gm::msm_glv_on(const gm_ctx* ctx, bool g2, size_t n) {
  if (ctx && ctx->msm_glv >= 0) return ctx->msm_glv != 0;
  // Default: GLV up to 2^21 points.  Measured (r03, same box, sync MSMs): at
  // 2^20 it halves the bucket reduction (BN254 G1 2.26 -> 2.14 ms, G2 7.65 ->
  // 6.51 ms); at 2^22 (BLS12-377) the reduction is a small share while the 2n
  // virtual points double the gathered point set (G1 14.2 -> 15.8 ms, G2 56.6
  // -> 62.1 ms).  BLS12-381 (curve id 2) was measured on its own, not inherited
  // (profiles/bls12381_timing.json, medians of five): 2^20 G1 4.23 -> 3.84 ms, G2
  // 12.72 -> 11.31 ms with GLV; 2^22 G1 13.32 -> 13.78 ms, G2 38.22 -> 37.89 ms
  // (inside each other's spread): the same threshold holds for it, so the
  // default takes no curve.  gm_set_msm_glv overrides it per context.
  if (n > (size_t(1) << 21)) return false;
  return true;
}

// MsmTail's pinned readback buffer goes back to its context (msm.hpp)
void gm::MsmTail::release_stage() {
  if (stage_ctx) tail_pinned_release(stage_ctx, stage_idx);
  stage_ctx = nullptr;
  stage_idx = -1;
  stage = nullptr;
}

struct gm_msm_pending {
  gm_ctx* ctx;  // nullptr once gm_destroy orphaned the handle
  int curve, g2;
  hipStream_t st = nullptr;  // stream the MSM runs on (slot stream or ctx->stream)
  gm::SlotArena slot;
  gm::MsmTail tail;
  explicit gm_msm_pending(gm_ctx* c) : ctx(c), slot(c) {}
};

// gm_destroy with MSMs pending (its streams already synchronised): every pending
// handle gives its slot arena and pinned readback buffer back to the context and
// is marked orphaned; the caller's later gm_msm_wait reports it and frees it.
void gm::orphan_pending_msms(gm_ctx* ctx) {
  for (gm_msm_pending* p : ctx->live_msms) {
    p->tail.release_stage();
    p->slot.release();
    p->ctx = nullptr;
  }
  ctx->live_msms.clear();
}

namespace {
template <class C, bool G2>
int msm_wait_t(gm_msm_pending* p, void* out_jac, void* out_aff) {
  using HF = typename GroupSel<C, G2>::HF;
  HF j[3];
  int rc = msm_finish<C, G2>(p->ctx, p->tail, j);
  if (rc) return rc;
  if (out_jac) memcpy(out_jac, j, sizeof(j));
  if (out_aff) {
    host::Aff<HF> a = host::to_aff(host::Jac<HF>{j[0], j[1], j[2]});
    memcpy(out_aff, &a, sizeof(a));
  }
  return GM_OK;
}
}  // namespace

// gm_msm_async, also over a prepared point set (msm.hpp)
int gm::msm_async_queue(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* points_dev, size_t n,
                        bool prepared, gm_msm_pending** out) {
  if (!ctx || !out) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_msm_async")) return rc;
  // no CtxLock: nothing is queued on ctx->stream here (gm_ctx::pending_reads)
  std::lock_guard<std::recursive_mutex> g(ctx->mu);
  GM_HIP(hipSetDevice(ctx->device));
  auto* p = new gm_msm_pending(ctx);
  p->curve = curve;
  p->g2 = g2 ? 1 : 0;
  int rc = p->slot.take();
  // One stream per slot: one MSM's fixup / reduction / readback overlaps the
  // next one's conversion and sort (profiles/r04m_hwq_ab.txt, r05r_slot_stream_ab.txt).
  // It starts after the work already queued on ctx->stream (the inputs).
  hipEvent_t inputs_read = nullptr;
  p->st = ctx->stream;
  if (rc == GM_OK) {
    hipStream_t& ss = ctx->slot_stream[p->slot.k];
    // The slot streams run at the highest stream priority: the runtime keeps a
    // separate pool of hardware queues per priority, so with the default four
    // queues they do not share one with ctx->stream / aux / copy or each other,
    // and the next MSM's conversion and sort start beside this one's reduction
    // (bench 2^20: 599-605 -> 632-645 Mpoints/s with the change below,
    // profiles/r05r_slot_stream_ab.txt).
    if (!ss) {
      int least = 0, greatest = 0;
      GM_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      GM_HIP(hipStreamCreateWithPriority(&ss, hipStreamNonBlocking, greatest));
    }
    // Ordered after the work already queued on ctx->stream (the inputs) -- by a
    // marker only when that stream still has work: a packet on ctx->stream waits
    // behind everything in its hardware queue, which may be shared with a slot
    // stream running the previous MSM.
    const hipError_t q = hipStreamQuery(ctx->stream);
    (void)hipGetLastError();  // hipErrorNotReady is an answer, not an error
    if (q != hipSuccess) {
      hipEvent_t ev;
      GM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      GM_HIP(hipEventRecord(ev, ctx->stream));
      GM_HIP(hipStreamWaitEvent(ss, ev, 0));
      GM_HIP(hipEventDestroy(ev));
    }
    p->st = ss;
    // work queued later on ctx->stream (synchronous calls that may overwrite the
    // scalars or points in place) waits until this MSM has read them: the event is
    // recorded after the digits and the point conversion, before the accumulation
    GM_HIP(hipEventCreateWithFlags(&inputs_read, hipEventDisableTiming));
  }
  {
    // The in-flight MSMs' accumulations run one after another (gm_ctx::acc_tail):
    // each launch then runs with the chip's wave slots free of the previous
    // one, so its start / stop stamps bracket its own execution (the bench's
    // kernel time; without the order a launch was stamped while it waited for the
    // previous accumulation's slots).  Same box: 621-624 against 624-630
    // Mpoints/s unordered (profiles/r06c_acc_chain_ab.txt).
    ctx->acc_chain = p->st != ctx->stream;  // slot streams only
    StreamSwap sw(ctx, p->st);
    struct ChainOff {
      gm_ctx* c;
      ~ChainOff() { c->acc_chain = false; }
    } chain_off{ctx};
    if (rc == GM_OK) {
      Arena& a = *p->slot.a;
      const void* sc = scalars_dev;
      const void* pt = points_dev;
      rc = GM_CURVE(curve,
                    g2 ? msm_device_launch<C, true>(ctx, a, sc, pt, n, prepared, nullptr, p->tail, inputs_read)
                       : msm_device_launch<C, false>(ctx, a, sc, pt, n, prepared, nullptr, p->tail, inputs_read));
    }
  }
  if (inputs_read && rc) hipEventDestroy(inputs_read);
  if (rc) {
    delete p;
    return rc;
  }
  // ctx->stream waits on it at the next call that may queue work there (CtxLock)
  if (inputs_read) ctx->pending_reads.push_back({p, inputs_read});
  ctx->live_msms.push_back(p);
  *out = p;
  return GM_OK;
}

extern "C" {

int gm_msm_async(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* points_dev, size_t n,
                 gm_msm_pending** out) {
  return gm::msm_async_queue(ctx, curve, g2, scalars_dev, points_dev, n, false, out);
}

int gm_msm_wait(gm_msm_pending* p, void* out_jac, void* out_affine) {
  if (!p) return GM_ERR_INVALID;
  gm_ctx* ctx = p->ctx;
  if (!ctx) {
    delete p;
    set_error("gm_msm_wait: the context was destroyed while this MSM was pending");
    return GM_ERR_INVALID;
  }
  std::lock_guard<std::recursive_mutex> g(ctx->mu);  // nothing queued on ctx->stream
  auto& live = ctx->live_msms;
  live.erase(std::remove(live.begin(), live.end(), p), live.end());
  // a finished MSM has read its inputs: ctx->stream need not wait for it
  auto& pr = ctx->pending_reads;
  for (auto it = pr.begin(); it != pr.end();)
    if (it->first == p) {
      hipEventDestroy(it->second);
      it = pr.erase(it);
    } else {
      ++it;
    }
  GM_HIP(hipSetDevice(ctx->device));
  StreamSwap sw(ctx, p->st);  // a long-span redo runs on the MSM's own stream
  const int rc = GM_CURVE(p->curve, p->g2 ? msm_wait_t<C, true>(p, out_jac, out_affine)
                                          : msm_wait_t<C, false>(p, out_jac, out_affine));
  prof_collect(ctx);
  delete p;
  return rc;
}

int gm_msm_host_scalars(gm_ctx* ctx, int curve, int g2, const void* scalars_host,
                        const void* points_dev, size_t n, void* out_jac, void* out_affine) {
  if (!ctx || (n && !scalars_host)) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_msm_host_scalars")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  DevBuf s;
  int rc;
  if ((rc = s.alloc(arena, 32 * n))) return rc;
  GM_HIP(hipMemcpyAsync(s.p, scalars_host, 32 * n, hipMemcpyHostToDevice, ctx->stream));
  return gm_msm(ctx, curve, g2, s.p, points_dev, n, out_jac, out_affine);
}

int gm_points_upload(gm_ctx* ctx, int curve, int g2, const void* host_points, size_t n, void** out) {
  if (!ctx || !out) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_points_upload")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const size_t gb = fp_bytes(curve) * (g2 ? 4 : 2) * n;
  const size_t ib = n * internal_point_bytes(curve, g2);
  Arena arena(ctx);
  DevBuf tmp;
  int rc;
  if ((rc = tmp.alloc(arena, gb))) return rc;
  hipError_t e = hipMalloc(out, ib ? ib : 16);
  if (e != hipSuccess) {
    set_error(std::string("gm_points_upload hipMalloc: ") + hipGetErrorString(e));
    return GM_ERR_OOM;
  }
  GM_HIP(hipMemcpyAsync(tmp.p, host_points, gb, hipMemcpyHostToDevice, ctx->stream));
  rc = GM_CURVE(curve, g2 ? msm_prepare_points<C, true>(ctx, tmp.p, n, *out)
                          : msm_prepare_points<C, false>(ctx, tmp.p, n, *out));
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

extern "C++" {
template <class C, bool G2>
static int msm_prepared_t(gm_ctx* ctx, const void* sc, const void* pts, size_t n, void* out_jac, void* out_aff,
                          const MsmPrecomp* pre = nullptr) {
  using HF = typename GroupSel<C, G2>::HF;
  HF j[3];
  int rc = msm_device<C, G2>(ctx, sc, pts, n, j, true, pre);
  if (rc) return rc;
  if (out_jac) memcpy(out_jac, j, sizeof(j));
  if (out_aff) {
    host::Aff<HF> a = host::to_aff(host::Jac<HF>{j[0], j[1], j[2]});
    memcpy(out_aff, &a, sizeof(a));
  }
  return GM_OK;
}
}  // extern "C++"

int gm_msm_prepared(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* prepared, size_t n,
                    void* out_jac, void* out_affine) {
  if (!ctx) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_msm_prepared")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const int rc = GM_CURVE(curve, g2 ? msm_prepared_t<C, true>(ctx, scalars_dev, prepared, n, out_jac, out_affine)
                                    : msm_prepared_t<C, false>(ctx, scalars_dev, prepared, n, out_jac, out_affine));
  prof_collect(ctx);
  return rc;
}

// ---- fixed-base precomputed point sets -------------------------------------------
static int make_precomp(int curve, size_t n, int window, MsmPrecomp* out) {
  const int bits = fr_bits(curve);
  if (window == 0) {
    *out = msm_choose_precomp(n, bits);
    return GM_OK;
  }
  if (window < 2 || window > 24) {
    set_error("precompute: window must be 0 (auto) or in [2, 24]");
    return GM_ERR_INVALID;
  }
  out->c = (uint32_t)window;
  out->W = (uint32_t)((bits + 1 + window - 1) / window);
  out->narrow = precomp_narrow(out->c, out->W, bits);
  out->stride = n;
  return GM_OK;
}

int gm_precompute_layout(int curve, size_t n, int window, int* c_out, int* copies_out) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_precompute_layout")) return rc;
  MsmPrecomp p;
  if (int rc = make_precomp(curve, n, window, &p)) return rc;
  if (c_out) *c_out = (int)p.c;
  if (copies_out) *copies_out = (int)p.W;
  return GM_OK;
}

int gm_points_upload_precomputed(gm_ctx* ctx, int curve, int g2, const void* host_points, size_t n, int window,
                                 void** out) {
  if (!ctx || !out) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_points_upload_precomputed")) return rc;
  MsmPrecomp pre;
  if (int rc = make_precomp(curve, n, window, &pre)) return rc;
  if ((size_t)pre.W * n >= (size_t(1) << 31)) {
    set_error("precompute: copies * n must be < 2^31");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const size_t gb = fp_bytes(curve) * (g2 ? 4 : 2) * n;
  const size_t ib = (size_t)pre.W * n * internal_point_bytes(curve, g2);
  Arena arena(ctx);
  DevBuf tmp;
  int rc;
  if ((rc = tmp.alloc(arena, gb ? gb : 16))) return rc;
  hipError_t e = hipMalloc(out, ib ? ib : 16);
  if (e != hipSuccess) {
    set_error(std::string("gm_points_upload_precomputed hipMalloc: ") + hipGetErrorString(e));
    return GM_ERR_OOM;
  }
  if (gb) GM_HIP(hipMemcpyAsync(tmp.p, host_points, gb, hipMemcpyHostToDevice, ctx->stream));
  rc = GM_CURVE(curve, g2 ? msm_precompute_points<C, true>(ctx, tmp.p, n, pre, *out)
                          : msm_precompute_points<C, false>(ctx, tmp.p, n, pre, *out));
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

int gm_msm_precomputed(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* prepared,
                       size_t prepared_n, int window, size_t n, void* out_jac, void* out_affine) {
  if (!ctx) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_msm_precomputed")) return rc;
  if (n > prepared_n) {
    set_error("msm_precomputed: n exceeds the prepared point count");
    return GM_ERR_INVALID;
  }
  MsmPrecomp pre;
  if (int rc = make_precomp(curve, prepared_n, window, &pre)) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const int rc =
      GM_CURVE(curve, g2 ? msm_prepared_t<C, true>(ctx, scalars_dev, prepared, n, out_jac, out_affine, &pre)
                         : msm_prepared_t<C, false>(ctx, scalars_dev, prepared, n, out_jac, out_affine, &pre));
  prof_collect(ctx);
  return rc;
}

int gm_kzg_commit(gm_ctx* ctx, int curve, const void* srs, size_t srs_len, const void* coeffs_host, size_t n,
                  void* digest_affine) {
  if (!ctx || !digest_affine) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_kzg_commit")) return rc;
  if (n > srs_len) {
    set_error("kzg commit: polynomial larger than the SRS");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  DevBuf s;
  int rc;
  if ((rc = s.alloc(arena, 32 * (n ? n : 1)))) return rc;
  ProfScope ps(ctx, "kzg_commit_call");  // upload + MSM (collected by the next profile read)
  if (n) GM_HIP(hipMemcpyAsync(s.p, coeffs_host, 32 * n, hipMemcpyHostToDevice, ctx->stream));
  return gm_msm_prepared(ctx, curve, 0, s.p, srs, n, nullptr, digest_affine);
}

// ---- KZG openings: evaluation, fold and division on the device (kzg.hip) ----------
int gm_kzg_eval(gm_ctx* ctx, int curve, const void* const* polys_dev, const size_t* lens, size_t k,
                const void* z_host, void* values_host) {
  if (!ctx || !z_host || !values_host) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_kzg_eval")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const int rc = GM_CURVE(curve, poly_eval_device<C>(ctx, polys_dev, lens, k, z_host, values_host));
  prof_collect(ctx);
  return rc;
}

int gm_poly_div_linear(gm_ctx* ctx, int curve, const void* f_dev, size_t m, const void* z_host, void* q_dev,
                       void* value_host) {
  if (!ctx || !z_host || !value_host) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_poly_div_linear")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const int rc = GM_CURVE(curve, poly_div_linear_device<C>(ctx, f_dev, m, z_host, q_dev, value_host));
  prof_collect(ctx);
  return rc;
}

int gm_poly_fold(gm_ctx* ctx, int curve, const void* const* polys_dev, const size_t* lens, size_t k,
                 const void* gamma_host, void* out_dev) {
  if (!ctx || !gamma_host) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_poly_fold")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  const int rc = GM_CURVE(curve, poly_fold_device<C>(ctx, polys_dev, lens, k, gamma_host, out_dev));
  prof_collect(ctx);
  return rc;
}

// H = commit((f - f(z)) / (X - z)) for f resident on the device; the quotient
// goes from workspace straight into the MSM.  A constant f has the zero
// quotient: the identity (0, 0), no MSM.
static int kzg_open_resident(gm_ctx* ctx, int curve, const void* srs, size_t srs_len, const void* f_dev, size_t m,
                             const void* z_host, void* value_host, void* h_affine) {
  if (m == 0 || m > srs_len) {
    set_error(m ? "kzg open: polynomial larger than the SRS" : "kzg open: empty polynomial");
    return GM_ERR_INVALID;
  }
  Arena arena(ctx);
  DevBuf q;
  int rc;
  if ((rc = q.alloc(arena, 32 * (m - 1)))) return rc;
  ProfScope ps(ctx, "kzg_open_call");  // division + MSM (collected by the next profile read)
  rc = GM_CURVE(curve, poly_div_linear_device<C>(ctx, f_dev, m, z_host, q.p, value_host));
  if (rc) return rc;
  if (m == 1) {
    memset(h_affine, 0, 2 * fp_bytes(curve));
    return GM_OK;
  }
  return gm_msm_prepared(ctx, curve, 0, q.p, srs, m - 1, nullptr, h_affine);
}

int gm_kzg_open(gm_ctx* ctx, int curve, const void* srs, size_t srs_len, const void* f_dev, size_t m,
                const void* z_host, void* claimed_host, void* h_affine) {
  if (!ctx || !z_host || !claimed_host || !h_affine) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_kzg_open")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  // the kernels' profile records are drained inside; the whole-call record closes
  // after the last synchronise and is left for the next profile read
  return kzg_open_resident(ctx, curve, srs, srs_len, f_dev, m, z_host, claimed_host, h_affine);
}

int gm_kzg_batch_open(gm_ctx* ctx, int curve, const void* srs, size_t srs_len, const void* const* polys_dev,
                      const size_t* lens, size_t k, const void* z_host, const void* gamma_host,
                      void* folded_value_host, void* h_affine) {
  if (!ctx || !z_host || !gamma_host || !h_affine) return GM_ERR_INVALID;
  if (int rc = check_curve(curve, CURVES_ALL, "gm_kzg_batch_open")) return rc;
  if (!polys_dev || !lens || k == 0) {
    set_error("kzg batch open: no polynomials");
    return GM_ERR_INVALID;
  }
  size_t m = 0;
  for (size_t i = 0; i < k; i++) m = std::max(m, lens[i]);
  if (m == 0 || m > srs_len) {
    set_error(m ? "kzg batch open: polynomial larger than the SRS" : "kzg batch open: empty polynomials");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  DevBuf folded;
  int rc;
  if ((rc = folded.alloc(arena, 32 * m))) return rc;
  rc = GM_CURVE(curve, poly_fold_device<C>(ctx, polys_dev, lens, k, gamma_host, folded.p));
  uint64_t value[4];
  if (!rc) rc = kzg_open_resident(ctx, curve, srs, srs_len, folded.p, m, z_host, value, h_affine);
  if (!rc && folded_value_host) memcpy(folded_value_host, value, sizeof(value));
  return rc;
}

// ---- PLONK quotient on resident polynomials (plonk.hip) -----------------------------
int gm_plonk_quotient(gm_ctx* ctx, int curve, const gm_plonk_quotient_in* in, void* h_dev) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_quotient")) return rc;
  if (!ctx || !in || !h_dev) return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  int rc;
  {
    ProfScope ps(ctx, "plonk_quotient_call");
    rc = GM_CURVE01(curve, plonk_quotient_device<C>(ctx, in, h_dev));
  }
  // also after a refusal part-way: nothing queued may outlive the call's workspace
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return rc;
}

// ---- PLONK permutation polynomial Z on resident wires (plonk_perm.hip) --------------
int gm_plonk_perm_z(gm_ctx* ctx, int curve, const gm_plonk_perm_in* in, void* z_lagrange_dev,
                    void* z_canonical_dev) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_perm_z")) return rc;
  if (!ctx || !in || !z_lagrange_dev) return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  int rc;
  {
    ProfScope ps(ctx, "plonk_perm_z_call");
    rc = GM_CURVE01(curve, plonk_perm_z_device<C>(ctx, in, z_lagrange_dev, z_canonical_dev));
  }
  // also after a refusal part-way: nothing queued may outlive the call's workspace
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return rc;
}

// ---- PLONK linearized polynomial on resident buffers (plonk_lin.hip) ----------------
int gm_plonk_linearize(gm_ctx* ctx, int curve, const gm_plonk_linearize_in* in, const gm_plonk_linearize_out* out) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_linearize")) return rc;
  if (!ctx || !in || !out) return GM_ERR_INVALID;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  int rc;
  {
    ProfScope ps(ctx, "plonk_linearize_call");
    rc = GM_CURVE01(curve, plonk_linearize_device<C>(ctx, in, out));
  }
  // also after a refusal part-way: nothing queued may outlive the call's workspace
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return rc;
}

// ---- PLONK proving key resident on the device (plonk_pk.hip) ------------------------
static int refuse_null(const char* what) {
  set_error(std::string(what) + ": a required pointer is NULL");
  return GM_ERR_INVALID;
}

int gm_plonk_pk_upload(gm_ctx* ctx, int curve, const gm_plonk_pk_host* pk, unsigned flags, gm_plonk_pk** out) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_pk_upload")) return rc;
  if (!ctx || !pk || !out) return refuse_null("plonk pk upload");
  return plonk_pk_upload(ctx, curve, pk, flags, out);
}

int gm_plonk_pk_bytes(const gm_plonk_pk* pk, size_t* resident_bytes, size_t* coset_cache_bytes) {
  if (!pk) return refuse_null("plonk pk bytes");
  if (resident_bytes) *resident_bytes = pk->resident_bytes;
  if (coset_cache_bytes) *coset_cache_bytes = pk->cache_bytes;
  return GM_OK;
}

int gm_plonk_pk_free(gm_ctx* ctx, gm_plonk_pk* pk) {
  if (!ctx || !pk) return refuse_null("plonk pk free");
  if (pk->ctx != ctx) {
    set_error("plonk pk free: the key was uploaded on another context");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  plonk_pk_release(pk);
  return GM_OK;
}

// ---- PLONK prover session: the five rounds on a resident key (plonk_session.hip) ----
int gm_plonk_session_begin(gm_ctx* ctx, gm_plonk_pk* pk, gm_plonk_session** out) {
  if (!ctx || !pk || !out) return refuse_null("plonk session begin");
  return plonk_session_begin(ctx, pk, out);
}

int gm_plonk_session_bsb22(gm_plonk_session* s, size_t j, const void* committed_host, void* digest_affine) {
  if (!s) return refuse_null("plonk session bsb22");
  return plonk_session_bsb22(s, j, committed_host, digest_affine);
}

int gm_plonk_session_round1(gm_plonk_session* s, const gm_plonk_round1_in* in, void* lro_affine) {
  if (!s || !in) return refuse_null("plonk session round 1");
  return plonk_session_round1(s, in, lro_affine);
}

int gm_plonk_session_round2(gm_plonk_session* s, const void* beta, const void* gamma, void* z_affine) {
  if (!s) return refuse_null("plonk session round 2");
  return plonk_session_round2(s, beta, gamma, z_affine);
}

int gm_plonk_session_round3(gm_plonk_session* s, const void* alpha, void* h_affine) {
  if (!s) return refuse_null("plonk session round 3");
  return plonk_session_round3(s, alpha, h_affine);
}

int gm_plonk_session_round4(gm_plonk_session* s, const void* zeta, void* lin_affine, void* claimed,
                            void* z_shifted_value, void* z_shifted_h_affine) {
  if (!s) return refuse_null("plonk session round 4");
  return plonk_session_round4(s, zeta, lin_affine, claimed, z_shifted_value, z_shifted_h_affine);
}

int gm_plonk_session_round5(gm_plonk_session* s, const void* kzg_gamma, void* batch_h_affine) {
  if (!s) return refuse_null("plonk session round 5");
  return plonk_session_round5(s, kzg_gamma, batch_h_affine);
}

int gm_plonk_session_free(gm_plonk_session* s) {
  if (!s) return refuse_null("plonk session free");
  gm::CtxLock g(s->ctx);
  GM_HIP(hipSetDevice(s->ctx->device));
  GM_HIP(hipStreamSynchronize(s->ctx->stream));
  plonk_session_release(s);
  return GM_OK;
}

// ---- PLONK session from the witness: resident wire tables (plonk_wires.hip) ----------
int gm_plonk_wires_upload(gm_ctx* ctx, size_t n, size_t nb_wires, const uint32_t* xa, const uint32_t* xb,
                          const uint32_t* xc, gm_plonk_wires** out) {
  if (!ctx || !xa || !xb || !xc || !out) return refuse_null("plonk wires upload");
  return plonk_wires_upload(ctx, n, nb_wires, xa, xb, xc, out);
}

int gm_plonk_wires_bytes(const gm_plonk_wires* w, size_t* resident_bytes) {
  if (!w || !resident_bytes) return refuse_null("plonk wires bytes");
  *resident_bytes = 3 * w->n * sizeof(uint32_t);
  return GM_OK;
}

int gm_plonk_wires_free(gm_ctx* ctx, gm_plonk_wires* w) {
  if (!ctx || !w) return refuse_null("plonk wires free");
  if (w->ctx != ctx) {
    set_error("plonk wires free: the tables were uploaded on another context");
    return GM_ERR_INVALID;
  }
  if (w->borrowed) {
    set_error("plonk wires free: the tables belong to a circuit (gm_plonk_scs_free frees them)");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  plonk_wires_release(w);
  return GM_OK;
}

int gm_plonk_gather_lro(gm_ctx* ctx, const gm_plonk_wires* w, const void* witness, void* l, void* r, void* o) {
  if (!ctx || !w || !witness || !l || !r || !o) return refuse_null("plonk gather lro");
  if (w->ctx != ctx) {
    set_error("plonk gather lro: the tables were uploaded on another context");
    return GM_ERR_INVALID;
  }
  // the kernel moves 16-byte halves; [witness), [l), [r), [o) pairwise disjoint
  const uintptr_t base[4] = {(uintptr_t)witness, (uintptr_t)l, (uintptr_t)r, (uintptr_t)o};
  const size_t len[4] = {32 * w->nb_wires, 32 * w->n, 32 * w->n, 32 * w->n};
  for (int a = 0; a < 4; a++) {
    if (base[a] % 16) {
      set_error("plonk gather lro: the buffers must be 16-byte aligned");
      return GM_ERR_INVALID;
    }
    for (int b = a + 1; b < 4; b++)
      if (base[a] < base[b] + len[b] && base[b] < base[a] + len[a]) {
        set_error(a == 0 ? "plonk gather lro: an output overlaps the witness"
                         : "plonk gather lro: two outputs overlap");
        return GM_ERR_INVALID;
      }
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  int rc;
  {
    ProfScope ps(ctx, "plonk_gather_lro_call");
    rc = plonk_gather_lro_device(ctx, w, witness, l, r, o);
  }
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return rc;
}

int gm_plonk_session_round1_witness(gm_plonk_session* s, const gm_plonk_wires* w,
                                    const gm_plonk_round1_witness_in* in, void* lro_affine) {
  if (!s || !w || !in) return refuse_null("plonk session round 1 from the witness");
  return plonk_session_round1_witness(s, w, in, lro_affine);
}

int gm_plonk_session_bsb22_sparse(gm_plonk_session* s, size_t j, const uint32_t* rows, const void* values,
                                  size_t count, void* digest_affine) {
  if (!s) return refuse_null("plonk session bsb22 sparse");
  return plonk_session_bsb22_sparse(s, j, rows, values, count, digest_affine);
}

// ---- PLONK setup on the device (plonk_setup.hip) --------------------------------------
int gm_kzg_srs_lagrange(gm_ctx* ctx, int curve, const void* srs_dev, size_t n, void* lagrange_dev) {
  if (int rc = check_curve(curve, CURVES_01, "gm_kzg_srs_lagrange")) return rc;
  if (!ctx || !srs_dev || !lagrange_dev) return refuse_null("kzg srs lagrange");
  // in place or disjoint: the last pass writes while other lanes may still read
  const uintptr_t a = (uintptr_t)srs_dev, b = (uintptr_t)lagrange_dev;
  const size_t len = 2 * fp_bytes(curve) * n;
  if (a != b && a < b + len && b < a + len) {
    set_error("kzg srs lagrange: the output overlaps the input without being the input");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE01(curve, kzg_srs_lagrange_device<C>(ctx, srs_dev, n, lagrange_dev));
}

int gm_plonk_sigma(gm_ctx* ctx, int curve, size_t n, const int64_t* perm_host, void* s1_dev, void* s2_dev,
                   void* s3_dev) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_sigma")) return rc;
  if (!ctx || !perm_host || !s1_dev || !s2_dev || !s3_dev) return refuse_null("plonk sigma");
  if (n == 0 || (n & (n - 1)) || n > (size_t(1) << 30)) {
    set_error("plonk sigma: n must be a power of two, 2 <= n <= 2^30");
    return GM_ERR_INVALID;
  }
  if (int rc = plonk_perm_check(n, perm_host)) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE01(curve, plonk_sigma_device<C>(ctx, n, perm_host, s1_dev, s2_dev, s3_dev));
}

int gm_plonk_pk_setup(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, unsigned flags, gm_plonk_pk** out,
                      void* vk_digests, void* srs_lagrange_out) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_pk_setup")) return rc;
  if (!ctx || !in || !out) return refuse_null("plonk pk setup");
  return plonk_pk_setup(ctx, curve, in, flags, out, vk_digests, srs_lagrange_out);
}

int gm_plonk_wires_permutation(gm_ctx* ctx, const gm_plonk_wires* w, int64_t* perm_dev) {
  if (!ctx || !w || !perm_dev) return refuse_null("plonk wires permutation");
  return plonk_wires_permutation(ctx, w, perm_dev);
}

int gm_plonk_sigma_wires(gm_ctx* ctx, int curve, const gm_plonk_wires* w, void* s1_dev, void* s2_dev, void* s3_dev) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_sigma_wires")) return rc;
  if (!ctx || !w || !s1_dev || !s2_dev || !s3_dev) return refuse_null("plonk sigma wires");
  if (w->ctx != ctx) {
    set_error("plonk sigma wires: the tables were uploaded on another context");
    return GM_ERR_INVALID;
  }
  if (w->n > (size_t(1) << 30)) {
    set_error("plonk sigma wires: n must be a power of two, 2 <= n <= 2^30");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE01(curve, plonk_sigma_wires_device<C>(ctx, w, s1_dev, s2_dev, s3_dev));
}

int gm_plonk_pk_setup_wires(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, const gm_plonk_wires* w,
                            unsigned flags, gm_plonk_pk** out, void* vk_digests, void* srs_lagrange_out) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_pk_setup_wires")) return rc;
  if (!ctx || !in || !w || !out) return refuse_null("plonk pk setup wires");
  return plonk_pk_setup_wires(ctx, curve, in, w, flags, out, vk_digests, srs_lagrange_out);
}

// ---- PLONK circuit on the device (plonk_scs.hip) --------------------------------------
int gm_plonk_scs_upload(gm_ctx* ctx, int curve, const gm_plonk_scs_host* in, gm_plonk_scs** out) {
  if (int rc = check_curve(curve, CURVES_01, "gm_plonk_scs_upload")) return rc;
  if (!ctx || !in || !out) return refuse_null("plonk scs upload");
  return plonk_scs_upload(ctx, curve, in, out);
}

int gm_plonk_scs_bytes(const gm_plonk_scs* scs, size_t* resident_bytes) {
  if (!scs || !resident_bytes) return refuse_null("plonk scs bytes");
  *resident_bytes = scs->bytes;
  return GM_OK;
}

int gm_plonk_scs_free(gm_ctx* ctx, gm_plonk_scs* scs) {
  if (!ctx || !scs) return refuse_null("plonk scs free");
  if (scs->ctx != ctx) {
    set_error("plonk scs free: the circuit was uploaded on another context");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  plonk_scs_release(scs);
  return GM_OK;
}

int gm_plonk_scs_wires(const gm_plonk_scs* scs, const gm_plonk_wires** out) {
  if (!scs || !out) return refuse_null("plonk scs wires");
  *out = &scs->wires;
  return GM_OK;
}

int gm_plonk_scs_selector(gm_ctx* ctx, const gm_plonk_scs* scs, unsigned which, void* out_dev) {
  if (!ctx || !scs || !out_dev) return refuse_null("plonk scs selector");
  return plonk_scs_selector(ctx, scs, which, out_dev);
}

int gm_plonk_pk_setup_scs(gm_ctx* ctx, const gm_plonk_scs* scs, const void* srs_canonical, size_t srs_canonical_len,
                          unsigned flags, gm_plonk_pk** out, void* vk_digests, void* srs_lagrange_out) {
  if (!ctx || !scs || !out) return refuse_null("plonk pk setup scs");
  return plonk_pk_setup_scs(ctx, scs, srs_canonical, srs_canonical_len, flags, out, vk_digests, srs_lagrange_out);
}

int gm_plonk_scs_check(gm_ctx* ctx, const gm_plonk_scs* scs, const void* witness_host, size_t* nb_unsatisfied,
                       size_t* first_unsatisfied) {
  if (!ctx || !scs || !witness_host || !nb_unsatisfied || !first_unsatisfied) return refuse_null("plonk scs check");
  return plonk_scs_check(ctx, scs, witness_host, nb_unsatisfied, first_unsatisfied);
}

// ---- NTT --------------------------------------------------------------------------
int gm_ntt(gm_ctx* ctx, int curve, void* data_dev, size_t n, int inverse, int dit, int coset) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_ntt")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  int rc = GM_CURVE(curve, ntt_device<C>(ctx, data_dev, n, inverse, dit, coset));
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return GM_OK;
}
int gm_poly_ops(gm_ctx* ctx, int curve, void* a, const void* b, const void* c, size_t n,
                const void* den_host) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_poly_ops")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  int rc = GM_CURVE(curve, poly_ops_device<C>(ctx, a, b, c, n, den_host));
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return GM_OK;
}
int gm_reverse_scalars(gm_ctx* ctx, int curve, void* data_dev, size_t n) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_reverse_scalars")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  int rc = GM_CURVE(curve, reverse_device<C>(ctx, data_dev, n));
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return GM_OK;
}
int gm_groth16_compute_h(gm_ctx* ctx, int curve, void* a, void* b, void* c, size_t len, size_t n) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_groth16_compute_h")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  int rc = GM_CURVE(curve, compute_h_device<C>(ctx, a, b, c, len, n));
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  prof_collect(ctx);
  return GM_OK;
}

// ---- host group helpers ---------------------------------------------------------------
extern "C++" {
template <class HF>
static void jac_add_t(const void* p, const void* q, void* out) {
  host::Jac<HF> a, b;
  memcpy(&a, p, sizeof(a));
  memcpy(&b, q, sizeof(b));
  host::Jac<HF> r = host::jadd(a, b);
  memcpy(out, &r, sizeof(r));
}
template <class HF>
static void jac_aff_t(const void* p, void* out) {
  host::Jac<HF> a;
  memcpy(&a, p, sizeof(a));
  host::Aff<HF> r = host::to_aff(a);
  memcpy(out, &r, sizeof(r));
}
}  // extern "C++"

int gm_jac_add(int curve, int g2, const void* p, const void* q, void* out) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_jac_add")) return rc;
  return GM_CURVE(curve, (g2 ? jac_add_t<typename C::HG2F>(p, q, out) : jac_add_t<typename C::HG1F>(p, q, out)),
                  (int)GM_OK);
}
int gm_jac_to_affine(int curve, int g2, const void* p, void* out) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_jac_to_affine")) return rc;
  return GM_CURVE(curve, (g2 ? jac_aff_t<typename C::HG2F>(p, out) : jac_aff_t<typename C::HG1F>(p, out)),
                  (int)GM_OK);
}

// ---- synthetic inputs -------------------------------------------------------------------
static const uint64_t GEN_BN_G1[] = GM_BN254_G1_GEN64;
static const uint64_t GEN_BN_G2[] = GM_BN254_G2_GEN64;
static const uint64_t GEN_BLS_G1[] = GM_BLS12377_G1_GEN64;
static const uint64_t GEN_BLS_G2[] = GM_BLS12377_G2_GEN64;
static const uint64_t GEN_BLS381_G1[] = GM_BLS12381_G1_GEN64;
static const uint64_t GEN_BLS381_G2[] = GM_BLS12381_G2_GEN64;

int gm_generator(int curve, int g2, void* out) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_generator")) return rc;
  static const uint64_t* const gens[CURVE_COUNT][2] = {
      {GEN_BN_G1, GEN_BN_G2}, {GEN_BLS_G1, GEN_BLS_G2}, {GEN_BLS381_G1, GEN_BLS381_G2}};
  const uint64_t* src = gens[curve][g2 ? 1 : 0];
  memcpy(out, src, fp_bytes(curve) * (g2 ? 4 : 2));
  return GM_OK;
}

int gm_random_scalars(gm_ctx* ctx, int curve, uint64_t seed, size_t n, void* scalars_dev) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_random_scalars")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  with_curve(
      curve,
      [&](auto tag_) {
        using Fr = typename decltype(tag_)::type::Fr;
        hipLaunchKernelGGL(k_random_scalars<Fr>, dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream,
                           (uint32_t*)scalars_dev, n, seed);
        return 0;
      },
      0);
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

extern "C++" {
template <class C, bool G2>
static int batch_mul_t(gm_ctx* ctx, const void* base, const void* sc, size_t n, void* out) {
  using DF = typename GroupSel<C, G2>::DF;
  GPoint<DF> b;
  memcpy(&b, base, sizeof(b));
  hipLaunchKernelGGL((k_batch_mul_base<typename C::Fr, DF>), dim3(blocks_for(n, 128)), dim3(128), 0,
                     ctx->stream, (const uint32_t*)sc, n, b, (uint32_t*)out);
  GM_HIP(hipGetLastError());
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}
}  // extern "C++"

int gm_batch_mul_base(gm_ctx* ctx, int curve, int g2, const void* base, const void* sc, size_t n,
                      void* out) {
  if (int rc = check_curve(curve, CURVES_01, "gm_batch_mul_base")) return rc;
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE01(curve, g2 ? batch_mul_t<C, true>(ctx, base, sc, n, out)
                               : batch_mul_t<C, false>(ctx, base, sc, n, out));
}

// ---- point validation (points_check.hip; the streamed entries: pk_io.hip) -------------
int gm_points_check(gm_ctx* ctx, int curve, int g2, const void* points_dev, size_t n, uint8_t* status_dev,
                    gm_points_report* out) {
  if (int rc = check_curve(curve, CURVES_ALL, "gm_points_check")) return rc;
  if (!ctx || !out || (n && !points_dev)) return refuse_null("gm_points_check");
  if (g2 != 0 && g2 != 1) {
    set_error("gm_points_check: g2 must be 0 or 1");
    return GM_ERR_INVALID;
  }
  if ((uintptr_t)points_dev % 16) {
    set_error("gm_points_check: the points must be 16-byte aligned");
    return GM_ERR_INVALID;
  }
  if (n == 0) {
    points_report_zero(out, 0);
    return GM_OK;
  }
  return points_check_device(ctx, curve, g2 != 0, points_dev, n, status_dev, out);
}

int gm_set_points_check_chunk(gm_ctx* ctx, size_t bytes) {
  if (!ctx) return refuse_null("gm_set_points_check_chunk");
  if (bytes > POINTS_CHECK_CHUNK_MAX) {
    set_error("gm_set_points_check_chunk: bytes must be 0 (the default) or at most 64 MiB");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  ctx->points_check_chunk = bytes;
  return GM_OK;
}

// ---- point encodings (points_codec.hip; the streamed entry: pk_io.hip) -----------------
static int codec_refuse(const char* entry, const char* what) {
  set_error(std::string(entry) + ": " + what);
  return GM_ERR_INVALID;
}
// [a, a + na) and [b, b + nb) share a byte
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na && nb && x < y + nb && y < x + na;
}

int gm_points_decode(gm_ctx* ctx, int curve, int g2, int encoding, unsigned flags, const void* enc_dev, size_t n,
                     void* points_dev, uint8_t* status_dev, gm_points_decode_report* out) {
  const char* me = "gm_points_decode";
  if (int rc = check_curve(curve, CURVES_ALL, me)) return rc;
  if (!ctx || !out || (n && (!enc_dev || !points_dev))) return refuse_null(me);
  if (g2 != 0 && g2 != 1) return codec_refuse(me, "g2 must be 0 or 1");
  if (encoding != GM_ENC_COMPRESSED && encoding != GM_ENC_RAW) return codec_refuse(me, "unknown encoding");
  if (flags & ~GM_DECODE_NO_SUBGROUP_CHECK) return codec_refuse(me, "unknown flags");
  if ((uintptr_t)enc_dev % 16 || (uintptr_t)points_dev % 16)
    return codec_refuse(me, "the records and the points must be 16-byte aligned");
  const size_t rb = codec_record_bytes(curve, g2 != 0, encoding == GM_ENC_RAW), pb = codec_point_bytes(curve, g2 != 0);
  if (n > (~size_t(0)) / pb) return codec_refuse(me, "n points do not fit the address space");
  if (ranges_overlap(enc_dev, n * rb, points_dev, n * pb) || ranges_overlap(status_dev, status_dev ? n : 0, points_dev, n * pb) ||
      ranges_overlap(status_dev, status_dev ? n : 0, enc_dev, n * rb))
    return codec_refuse(me, "the records, the points and the status bytes must not overlap");
  if (n == 0) {
    points_decode_report_zero(out, 0);
    return GM_OK;
  }
  return points_decode_device(ctx, curve, g2 != 0, encoding == GM_ENC_RAW, flags, enc_dev, n, points_dev, status_dev,
                              out);
}

int gm_points_encode(gm_ctx* ctx, int curve, int g2, int encoding, const void* points_dev, size_t n, void* enc_dev,
                     uint64_t* not_reduced) {
  const char* me = "gm_points_encode";
  if (int rc = check_curve(curve, CURVES_ALL, me)) return rc;
  if (!ctx || !not_reduced || (n && (!enc_dev || !points_dev))) return refuse_null(me);
  if (g2 != 0 && g2 != 1) return codec_refuse(me, "g2 must be 0 or 1");
  if (encoding != GM_ENC_COMPRESSED && encoding != GM_ENC_RAW) return codec_refuse(me, "unknown encoding");
  if ((uintptr_t)enc_dev % 16 || (uintptr_t)points_dev % 16)
    return codec_refuse(me, "the records and the points must be 16-byte aligned");
  const size_t rb = codec_record_bytes(curve, g2 != 0, encoding == GM_ENC_RAW), pb = codec_point_bytes(curve, g2 != 0);
  if (n > (~size_t(0)) / pb) return codec_refuse(me, "n points do not fit the address space");
  if (ranges_overlap(enc_dev, n * rb, points_dev, n * pb))
    return codec_refuse(me, "the records and the points must not overlap");
  *not_reduced = 0;
  if (n == 0) return GM_OK;
  return points_encode_device(ctx, curve, g2 != 0, encoding == GM_ENC_RAW, points_dev, n, enc_dev, not_reduced);
}

// ---- pairing-product checks and Groth16 verification (pairing.hip) -----------------------
static int pairing_refusals(const char* me, gm_ctx* ctx, int curve, const void* g1, const void* g2, size_t n_products,
                            size_t k, const uint8_t* ok_out, bool device) {
  if (int rc = check_curve(curve, CURVES_ALL, me)) return rc;
  if (!ctx || !g1 || !g2 || !ok_out) return refuse_null(me);
  if (k == 0) return codec_refuse(me, "k must be at least 1");
  if (device && ((uintptr_t)g1 % 16 || (uintptr_t)g2 % 16)) return codec_refuse(me, "the points must be 16-byte aligned");
  if (n_products && k > (~size_t(0)) / pairing_gt_bytes(curve) / n_products)
    return codec_refuse(me, "n_products * k pairs do not fit the address space");
  return GM_OK;
}

int gm_pairing_check(gm_ctx* ctx, int curve, const void* g1_host, const void* g2_host, size_t n_products, size_t k,
                     uint8_t* ok_out) {
  if (int rc = pairing_refusals("gm_pairing_check", ctx, curve, g1_host, g2_host, n_products, k, ok_out, false)) return rc;
  if (n_products == 0) return GM_OK;
  return pairing_check_host(ctx, curve, g1_host, g2_host, n_products, k, ok_out);
}

int gm_pairing_check_device(gm_ctx* ctx, int curve, const void* g1_dev, const void* g2_dev, size_t n_products,
                            size_t k, uint8_t* ok_out) {
  if (int rc = pairing_refusals("gm_pairing_check_device", ctx, curve, g1_dev, g2_dev, n_products, k, ok_out, true))
    return rc;
  if (n_products == 0) return GM_OK;
  return pairing_check_device(ctx, curve, g1_dev, g2_dev, n_products, k, ok_out);
}

int gm_g16_vk_upload(gm_ctx* ctx, int curve, const gm_g16_vk_host* vk, gm_g16_vk** out) {
  const char* me = "gm_g16_vk_upload";
  if (int rc = check_curve(curve, CURVES_ALL, me)) return rc;
  if (!ctx || !vk || !out) return refuse_null(me);
  *out = nullptr;
  if (!vk->alpha_g1 || !vk->beta_g2 || !vk->gamma_g2 || !vk->delta_g2 || !vk->k_g1) return refuse_null(me);
  if (vk->nb_k == 0) return codec_refuse(me, "nb_k must be at least 1 (K[0], the one wire)");
  return g16_vk_upload(ctx, curve, vk, out);
}

int gm_g16_vk_free(gm_ctx* ctx, gm_g16_vk* vk) {
  if (!ctx || !vk) return refuse_null("gm_g16_vk_free");
  if (vk->ctx != ctx) return codec_refuse("gm_g16_vk_free", "the key belongs to another context");
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  if (vk->g1) hipFree(vk->g1);
  if (vk->g2) hipFree(vk->g2);
  delete vk;
  return GM_OK;
}

int gm_g16_verify_batch(gm_ctx* ctx, const gm_g16_vk* vk, const void* proofs_host, const void* publics_host, size_t m,
                        uint8_t* status_out, size_t* nb_ok) {
  const char* me = "gm_g16_verify_batch";
  if (!ctx || !vk) return refuse_null(me);
  if (vk->ctx != ctx) return codec_refuse(me, "the key belongs to another context");
  if (m == 0) {
    if (nb_ok) *nb_ok = 0;
    return GM_OK;
  }
  if (!proofs_host || !status_out || (vk->nb_k > 1 && !publics_host)) return refuse_null(me);
  if (m > (~size_t(0)) / (16 * fp_bytes(vk->curve))) return codec_refuse(me, "m proofs do not fit the address space");
  return g16_verify_batch(ctx, vk, proofs_host, publics_host, m, status_out, nb_ok);
}

// ---- KZG and PLONK verification (plonk_verify.hip) ---------------------------------------
int gm_kzg_vk_upload(gm_ctx* ctx, int curve, const gm_kzg_vk_host* vk, gm_kzg_vk** out) {
  const char* me = "gm_kzg_vk_upload";
  if (int rc = check_curve(curve, CURVES_ALL, me)) return rc;
  if (!ctx || !vk || !out) return refuse_null(me);
  *out = nullptr;
  if (!vk->g1 || !vk->g2_0 || !vk->g2_1) return refuse_null(me);
  return kzg_vk_upload(ctx, curve, vk, out);
}

int gm_kzg_vk_free(gm_ctx* ctx, gm_kzg_vk* vk) {
  if (!ctx || !vk) return refuse_null("gm_kzg_vk_free");
  if (vk->ctx != ctx) return codec_refuse("gm_kzg_vk_free", "the key belongs to another context");
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  kzg_vk_release(vk);
  return GM_OK;
}

static int kzg_verify_entry(const char* me, gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* in, size_t m,
                            bool fold, uint8_t* status_out, size_t* nb_ok) {
  if (!ctx || !vk) return refuse_null(me);
  if (vk->ctx != ctx) return codec_refuse(me, "the key belongs to another context");
  if (m == 0) {
    if (nb_ok) *nb_ok = 0;
    return GM_OK;
  }
  if (!in || !status_out || !in->digests || !in->proofs || !in->points || !in->values || (fold && !in->lambda))
    return refuse_null(me);
  if (m > (~size_t(0)) / (16 * fp_bytes(vk->curve))) return codec_refuse(me, "m openings do not fit the address space");
  return kzg_verify_batch(ctx, vk, in, m, kzg_verify_chunk(m, fold), fold, status_out, nb_ok);
}

int gm_kzg_verify_batch(gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* openings, size_t m,
                        uint8_t* status_out, size_t* nb_ok) {
  return kzg_verify_entry("gm_kzg_verify_batch", ctx, vk, openings, m, false, status_out, nb_ok);
}

int gm_kzg_verify_folded(gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* openings, size_t m,
                         uint8_t* status_out) {
  return kzg_verify_entry("gm_kzg_verify_folded", ctx, vk, openings, m, true, status_out, nullptr);
}

int gm_plonk_vk_upload(gm_ctx* ctx, int curve, const gm_plonk_vk_host* vk, gm_plonk_vk** out) {
  const char* me = "gm_plonk_vk_upload";
  if (int rc = check_curve(curve, CURVES_ALL, me)) return rc;
  if (!ctx || !vk || !out) return refuse_null(me);
  *out = nullptr;
  if (!vk->ql || !vk->qr || !vk->qm || !vk->qo || !vk->qk || !vk->s1 || !vk->s2 || !vk->s3 || !vk->kzg_g1 ||
      !vk->kzg_g2_0 || !vk->kzg_g2_1 || (vk->nb_bsb && (!vk->qcp || !vk->commitment_row)))
    return refuse_null(me);
  if (vk->n < 8 || (vk->n & (vk->n - 1))) return codec_refuse(me, "n must be a power of two, at least 8");
  if (vk->nb_public > vk->n) return codec_refuse(me, "nb_public exceeds n");
  if (vk->nb_bsb > 1024) return codec_refuse(me, "nb_bsb exceeds 1024");
  for (size_t j = 0; j < vk->nb_bsb; j++)
    if (vk->commitment_row[j] >= vk->n)
      return codec_refuse(me, ("commitment_row[" + std::to_string(j) + "] is not below n").c_str());
  return plonk_vk_upload(ctx, curve, vk, out);
}

int gm_plonk_vk_free(gm_ctx* ctx, gm_plonk_vk* vk) {
  if (!ctx || !vk) return refuse_null("gm_plonk_vk_free");
  if (vk->ctx != ctx) return codec_refuse("gm_plonk_vk_free", "the key belongs to another context");
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  plonk_vk_release(vk);
  return GM_OK;
}

int gm_plonk_verify_batch(gm_ctx* ctx, const gm_plonk_vk* vk, const gm_plonk_proofs_host* proofs, size_t m,
                          uint8_t* status_out, size_t* nb_ok) {
  const char* me = "gm_plonk_verify_batch";
  if (!ctx || !vk) return refuse_null(me);
  if (vk->ctx != ctx) return codec_refuse(me, "the key belongs to another context");
  if (m == 0) {
    if (nb_ok) *nb_ok = 0;
    return GM_OK;
  }
  if (!proofs || !status_out || !proofs->points || !proofs->values || !proofs->challenges ||
      (vk->nb_public && !proofs->publics) || (vk->nb_bsb && !proofs->hashed_cmt))
    return refuse_null(me);
  if (m > (~size_t(0)) / (16 * fp_bytes(vk->curve) * pv_terms(vk->nb_bsb)))
    return codec_refuse(me, "m proofs do not fit the address space");
  return plonk_verify_run(ctx, vk, proofs, m, plonk_verify_chunk(vk, m), status_out, nb_ok);
}

// ---- Groth16 setup: fixed-base batch multiplication (g16_setup.hip) --------------------
int gm_set_fixed_base_window(gm_ctx* ctx, int c) {
  if (!ctx) return refuse_null("gm_set_fixed_base_window");
  if (c != 0 && (c < FIXED_BASE_C_MIN || c > FIXED_BASE_C_MAX)) {
    set_error("gm_set_fixed_base_window: c must be 0 (the model) or in [" + std::to_string(FIXED_BASE_C_MIN) + ", " +
              std::to_string(FIXED_BASE_C_MAX) + "]");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  ctx->fixed_base_c = c;
  return GM_OK;
}

int gm_batch_mul_fixed(gm_ctx* ctx, int curve, int g2, const void* base, const void* sc, size_t n, void* out) {
  if (int rc = check_curve(curve, CURVES_01, "gm_batch_mul_fixed")) return rc;
  if (!ctx || !base || (n && (!sc || !out))) return refuse_null("gm_batch_mul_fixed");
  if (n >= (size_t(1) << 32)) {
    set_error("gm_batch_mul_fixed: n must be below 2^32");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  return GM_CURVE01(curve, g2 ? batch_mul_fixed_device<C, true>(ctx, base, sc, n, out)
                               : batch_mul_fixed_device<C, false>(ctx, base, sc, n, out));
}

// ---- Groth16 setup: the scalar side and the points (g16_setup.hip) ------------------------
int gm_set_g16_setup_column_cut(gm_ctx* ctx, int t) {
  if (!ctx) return refuse_null("gm_set_g16_setup_column_cut");
  if (t < 0 || t > (1 << 30)) {
    set_error("gm_set_g16_setup_column_cut: t must be 0 (the default) or in [1, 2^30]");
    return GM_ERR_INVALID;
  }
  gm::CtxLock g(ctx);
  ctx->g16_column_cut = t;
  return GM_OK;
}

int gm_g16_setup_sizes(gm_ctx* ctx, const gm_r1cs* r1cs, const gm_g16_setup_in* in, size_t* nbA, size_t* nbB,
                       size_t* nbK) {
  if (!ctx || !r1cs || !in || !nbA || !nbB || !nbK) return refuse_null("gm_g16_setup_sizes");
  size_t sizes[3] = {0, 0, 0};
  if (int rc = g16_setup_run(ctx, "gm_g16_setup_sizes", r1cs, in, nullptr, sizes, 0, nullptr)) return rc;
  *nbA = sizes[0], *nbB = sizes[1], *nbK = sizes[2];
  return GM_OK;
}

int gm_g16_setup(gm_ctx* ctx, const gm_r1cs* r1cs, const gm_g16_setup_in* in, const gm_g16_setup_out* out) {
  if (!ctx || !r1cs || !in || !out) return refuse_null("gm_g16_setup");
  return g16_setup_run(ctx, "gm_g16_setup", r1cs, in, out, nullptr, 0, nullptr);
}

int gm_g16_pk_setup(gm_ctx* ctx, const gm_r1cs* r1cs, const gm_g16_setup_in* in, unsigned flags, gm_g16_pk** out,
                    const gm_g16_setup_out* host_copy) {
  if (!ctx || !r1cs || !in || !out) return refuse_null("gm_g16_pk_setup");
  if (flags & ~(unsigned)(GM_PK_PRECOMPUTE | GM_PK_PRECOMPUTE_AUTO)) {
    set_error("gm_g16_pk_setup: unknown flags");
    return GM_ERR_INVALID;
  }
  return g16_setup_run(ctx, "gm_g16_pk_setup", r1cs, in, host_copy, nullptr, flags, out);
}

}  // extern "C"
