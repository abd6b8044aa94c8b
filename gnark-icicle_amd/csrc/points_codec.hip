// Point codec, host side: dispatch by curve id, the device result and its
// report.  The kernels are points_codec_impl.hpp, instantiated per curve.
#include "points_codec.hpp"

#include "curves.hpp"

namespace gm {

int points_decode_queue(gm_ctx* ctx, int curve, bool g2, bool raw, unsigned flags, const void* enc_dev, size_t n,
                        size_t base, void* points_dev, uint8_t* status_dev, unsigned long long* res_dev) {
  return with_curve(
      curve,
      [&](auto tag_) {
        using C = typename decltype(tag_)::type;
        return g2 ? points_decode_launch<C, true>(ctx, enc_dev, n, base, raw, flags, points_dev, status_dev, res_dev)
                  : points_decode_launch<C, false>(ctx, enc_dev, n, base, raw, flags, points_dev, status_dev, res_dev);
      },
      (int)GM_ERR_INVALID);
}

int points_decode_reset(gm_ctx* ctx, unsigned long long* res_dev) {
  GM_HIP(hipMemsetAsync(res_dev, 0, CD_FIRST_KEY * sizeof(unsigned long long), ctx->stream));
  GM_HIP(hipMemsetAsync(res_dev + CD_FIRST_KEY, 0xff, sizeof(unsigned long long), ctx->stream));
  return GM_OK;
}

void points_decode_report_zero(gm_points_decode_report* out, size_t n) {
  memset(out, 0, sizeof(*out));
  out->n = n;
  out->first_bad = n;
  out->first_class = GM_POINT_OK;
}

int points_decode_read(gm_ctx* ctx, const unsigned long long* res_dev, size_t n, gm_points_decode_report* out) {
  unsigned long long got[CD_RES_WORDS];
  GM_HIP(hipMemcpyAsync(got, res_dev, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  points_decode_report_zero(out, n);
  out->infinities = got[CD_INFINITIES];
  out->not_reduced = got[GM_POINT_NOT_REDUCED];
  out->off_curve = got[GM_POINT_OFF_CURVE];
  out->off_subgroup = got[GM_POINT_OFF_SUBGROUP];
  out->bad_encoding = got[GM_POINT_BAD_ENCODING];
  out->no_root = got[GM_POINT_NO_ROOT];
  if (got[CD_FIRST_KEY] != ~0ull) {
    out->first_bad = got[CD_FIRST_KEY] >> 3;
    out->first_class = (uint32_t)(got[CD_FIRST_KEY] & 7);
  }
  return GM_OK;
}

int points_decode_device(gm_ctx* ctx, int curve, bool g2, bool raw, unsigned flags, const void* enc_dev, size_t n,
                         void* points_dev, uint8_t* status_dev, gm_points_decode_report* out) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  DevBuf res;
  if (int rc = res.alloc(arena, CD_RES_WORDS * sizeof(unsigned long long))) return rc;
  unsigned long long* r = res.as<unsigned long long>();
  if (int rc = points_decode_reset(ctx, r)) return rc;
  if (int rc = points_decode_queue(ctx, curve, g2, raw, flags, enc_dev, n, 0, points_dev, status_dev, r)) return rc;
  return points_decode_read(ctx, r, n, out);
}

int points_encode_device(gm_ctx* ctx, int curve, bool g2, bool raw, const void* points_dev, size_t n, void* enc_dev,
                         uint64_t* not_reduced) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  DevBuf res;
  if (int rc = res.alloc(arena, sizeof(unsigned long long))) return rc;
  unsigned long long* r = res.as<unsigned long long>();
  GM_HIP(hipMemsetAsync(r, 0, sizeof(unsigned long long), ctx->stream));
  const int rc = with_curve(
      curve,
      [&](auto tag_) {
        using C = typename decltype(tag_)::type;
        return g2 ? points_encode_launch<C, true>(ctx, points_dev, n, raw, enc_dev, r)
                  : points_encode_launch<C, false>(ctx, points_dev, n, raw, enc_dev, r);
      },
      (int)GM_ERR_INVALID);
  if (rc) return rc;
  unsigned long long got = 0;
  GM_HIP(hipMemcpyAsync(&got, r, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  *not_reduced = got;
  return GM_OK;
}

}  // namespace gm
