// Point validation on the device: every point of a gnark-layout array is
// classed GM_POINT_OK / _NOT_REDUCED / _OFF_CURVE / _OFF_SUBGROUP (DESIGN.md
// section 3.9; include/gnark_mi355x.h "point validation").
#pragma once
#include "runtime.hpp"

namespace gm {

// Device result of one or more launches over one array: the four counts, then
// the smallest 4 * index + class over the failing points (~0 when none fails).
// the chunk of the streamed checks (pk_io.hip): 16 MiB slots of the dump loader's
// ring unless gm_set_points_check_chunk asks for another size, up to the loader's
// 64 MiB.  The ring is pinned per call, and pinning costs more than a chunk's copy:
// a 2^20-point BN254 G1 array took 39 ms through two 64 MiB slots
// (profiles/points_check_timing.json has the 16 MiB figures).
constexpr size_t POINTS_CHECK_CHUNK = size_t(16) << 20;
constexpr size_t POINTS_CHECK_CHUNK_MAX = size_t(64) << 20;

enum { PC_INFINITIES = 0, PC_NOT_REDUCED, PC_OFF_CURVE, PC_OFF_SUBGROUP, PC_FIRST_KEY, PC_RES_WORDS };

// Queues the check of the n points at pts_dev (16-byte aligned) on ctx->stream.
// Point j counts as index base + j; its class goes to status_dev[j] when
// status_dev is not NULL; the counts are added into res_dev (points_check_reset
// prepares it).  Instantiated per curve in points_check_<curve>.hip.
template <class C, bool G2>
int points_check_launch(gm_ctx* ctx, const void* pts_dev, size_t n, size_t base, uint8_t* status_dev,
                        unsigned long long* res_dev);

// The same by curve id (0, 1 or 2; the caller has checked it).
int points_check_queue(gm_ctx* ctx, int curve, bool g2, const void* pts_dev, size_t n, size_t base,
                       uint8_t* status_dev, unsigned long long* res_dev);
int points_check_reset(gm_ctx* ctx, unsigned long long* res_dev);
// Waits for ctx->stream and turns the device result of an array of n points into its report.
int points_check_read(gm_ctx* ctx, const unsigned long long* res_dev, size_t n, gm_points_report* out);
void points_report_zero(gm_points_report* out, size_t n);

// gm_points_check behind its refusals: points resident on the device.
int points_check_device(gm_ctx* ctx, int curve, bool g2, const void* pts_dev, size_t n, uint8_t* status_dev,
                        gm_points_report* out);

}  // namespace gm
