// gnark-crypto's point encodings on the device: records (compressed or raw,
// big-endian, flagged) to gnark-layout points and back (DESIGN.md section 3.10;
// include/gnark_mi355x.h "point encodings").
#pragma once
#include "runtime.hpp"

namespace gm {

// Device result of one or more decode launches over one array: the infinities,
// one count per failing class (indexed by the class), then the smallest
// 8 * index + class over the failing records (~0 when none fails).
enum { CD_INFINITIES = 0, CD_FIRST_KEY = GM_POINT_NO_ROOT + 1, CD_RES_WORDS };

// bytes of one record / of one gnark-layout point
inline size_t codec_record_bytes(int curve, bool g2, bool raw) { return (raw ? 2 : 1) * (g2 ? 2 : 1) * fp_bytes(curve); }
inline size_t codec_point_bytes(int curve, bool g2) { return 2 * (g2 ? 2 : 1) * fp_bytes(curve); }

// Queues the decode of the n records at enc_dev into points_dev (both 16-byte
// aligned) on ctx->stream.  Record j counts as index base + j; its class goes to
// status_dev[j] when status_dev is not NULL; the counts are added into res_dev
// (points_decode_reset prepares it).  Instantiated per curve in
// points_codec_<curve>.hip.
template <class C, bool G2>
int points_decode_launch(gm_ctx* ctx, const void* enc_dev, size_t n, size_t base, bool raw, unsigned flags,
                         void* points_dev, uint8_t* status_dev, unsigned long long* res_dev);
// The reverse; res_dev: one word, the points with a component >= p are added to it.
template <class C, bool G2>
int points_encode_launch(gm_ctx* ctx, const void* points_dev, size_t n, bool raw, void* enc_dev,
                         unsigned long long* res_dev);

// The same by curve id (0, 1 or 2; the caller has checked it).
int points_decode_queue(gm_ctx* ctx, int curve, bool g2, bool raw, unsigned flags, const void* enc_dev, size_t n,
                        size_t base, void* points_dev, uint8_t* status_dev, unsigned long long* res_dev);
int points_decode_reset(gm_ctx* ctx, unsigned long long* res_dev);
// Waits for ctx->stream and turns the device result of n records into the report.
int points_decode_read(gm_ctx* ctx, const unsigned long long* res_dev, size_t n, gm_points_decode_report* out);
void points_decode_report_zero(gm_points_decode_report* out, size_t n);

// gm_points_decode / gm_points_encode behind their refusals.
int points_decode_device(gm_ctx* ctx, int curve, bool g2, bool raw, unsigned flags, const void* enc_dev, size_t n,
                         void* points_dev, uint8_t* status_dev, gm_points_decode_report* out);
int points_encode_device(gm_ctx* ctx, int curve, bool g2, bool raw, const void* points_dev, size_t n, void* enc_dev,
                         uint64_t* not_reduced);

}  // namespace gm
