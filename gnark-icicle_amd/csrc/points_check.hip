// Point validation, host side: dispatch by curve id, the device result and its
// report.  The kernel is points_check_impl.hpp, instantiated per curve.
#include "points_check.hpp"

#include "curves.hpp"

namespace gm {

int points_check_queue(gm_ctx* ctx, int curve, bool g2, const void* pts_dev, size_t n, size_t base,
                       uint8_t* status_dev, unsigned long long* res_dev) {
  return with_curve(
      curve,
      [&](auto tag_) {
        using C = typename decltype(tag_)::type;
        return g2 ? points_check_launch<C, true>(ctx, pts_dev, n, base, status_dev, res_dev)
                  : points_check_launch<C, false>(ctx, pts_dev, n, base, status_dev, res_dev);
      },
      (int)GM_ERR_INVALID);
}

int points_check_reset(gm_ctx* ctx, unsigned long long* res_dev) {
  GM_HIP(hipMemsetAsync(res_dev, 0, PC_FIRST_KEY * sizeof(unsigned long long), ctx->stream));
  GM_HIP(hipMemsetAsync(res_dev + PC_FIRST_KEY, 0xff, sizeof(unsigned long long), ctx->stream));
  return GM_OK;
}

void points_report_zero(gm_points_report* out, size_t n) {
  memset(out, 0, sizeof(*out));
  out->n = n;
  out->first_bad = n;
  out->first_class = GM_POINT_OK;
}

int points_check_read(gm_ctx* ctx, const unsigned long long* res_dev, size_t n, gm_points_report* out) {
  unsigned long long got[PC_RES_WORDS];
  GM_HIP(hipMemcpyAsync(got, res_dev, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  points_report_zero(out, n);
  out->infinities = got[PC_INFINITIES];
  out->not_reduced = got[PC_NOT_REDUCED];
  out->off_curve = got[PC_OFF_CURVE];
  out->off_subgroup = got[PC_OFF_SUBGROUP];
  if (got[PC_FIRST_KEY] != ~0ull) {
    out->first_bad = got[PC_FIRST_KEY] >> 2;
    out->first_class = (uint32_t)(got[PC_FIRST_KEY] & 3);
  }
  return GM_OK;
}

int points_check_device(gm_ctx* ctx, int curve, bool g2, const void* pts_dev, size_t n, uint8_t* status_dev,
                        gm_points_report* out) {
  CtxLock g(ctx);
  GM_HIP(hipSetDevice(ctx->device));
  Arena arena(ctx);
  DevBuf res;
  if (int rc = res.alloc(arena, PC_RES_WORDS * sizeof(unsigned long long))) return rc;
  if (int rc = points_check_reset(ctx, res.as<unsigned long long>())) return rc;
  if (int rc = points_check_queue(ctx, curve, g2, pts_dev, n, 0, status_dev, res.as<unsigned long long>())) return rc;
  return points_check_read(ctx, res.as<unsigned long long>(), n, out);
}

}  // namespace gm
