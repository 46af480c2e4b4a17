/* dvc_jpeg_rate.h - the rate target of the Motion-JPEG encoder (include/dvc.h,
 * dvc_jpeg_*): a handle made with a byte target per frame and a quality range
 * in place of one quality. An addition to the C-ABI of dvc.h, version 10,
 * exported by the same library; it is a header of its own because dvc.h's set of
 * prototypes is pinned. DESIGN.md "Motion-JPEG stream", "Rate target" is the
 * normative text.
 *
 * Every table group (a run of max_batch frames of one dvc_jpeg_encode or
 * dvc_jpeg_encode_stream call) is coded at one quality q*, found on the device
 * from the group's own coefficients: with B = frames * target_bytes and E(q)
 * the exact bytes of the group's samples at quality q with the fixed Huffman
 * tables before byte stuffing, E(q_min) > B makes the group a miss (q* =
 * q_min); otherwise lo = q_min, hi = q_max and, while lo < hi, mid =
 * (lo + hi + 1) >> 1, E(mid) <= B ? lo = mid : hi = mid - 1; q* = lo.
 *
 * What the target means: it bounds the unstuffed size with the fixed tables.
 * The 0x00 bytes stuffed behind 0xFF data bytes come on top (about 1 % on noisy
 * frames), and with DVC_FLAG_JPEG_OPT_HUFFMAN the written tables are the
 * group's own, so the real size differs from the estimate (usually below it);
 * the estimate never uses them. A target too small for q_min is not refused:
 * every group is then a miss. */
#ifndef DVC_JPEG_RATE_H
#define DVC_JPEG_RATE_H

#include "dvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most bytes in front of a rate handle's frame: DQT, DQT (138) and the
 * longest DHT + SOS of optimised tables. dvc_jpeg_bound(...) plus this always
 * fits a frame of a rate handle, with either kind of tables. */
#define DVC_JPEG_RATE_PREFIX_MAX (138 + DVC_JPEG_OPT_PREFIX_MAX)

/* Cumulative counters of a rate handle since its creation (a struct tag only:
 * the call below has the same name). */
struct dvc_jpeg_rate_stats {
    uint64_t groups;          /* table groups coded */
    uint64_t frames;          /* their frames */
    uint64_t missed_groups;   /* groups whose E(q_min) exceeded the budget */
    uint64_t est_bytes;       /* sum of E(q*) */
    uint64_t budget_bytes;    /* sum of B */
    uint64_t quality_frames;  /* sum of q* x frames of the group */
    uint64_t q_lowest;        /* the least, the greatest and the last q* (0 before the first group) */
    uint64_t q_highest;
    uint64_t q_last;
};

/* dvc_jpeg_create with target_bytes per frame and qualities q_min..q_max
 * (1 <= q_min <= q_max <= 100) in place of quality; every other argument and
 * every flag as there, DVC_FLAG_JPEG_OPT_HUFFMAN, DVC_FLAG_DEVICE_PTRS and
 * DVC_FLAG_JOIN_STREAM included; device < 0 gives a host-only handle for
 * dvc_jpeg_header. dvc_jpeg_header of the handle returns SOI, APP0, SOF0, the
 * two DHT segments (not with optimised tables) and DRI: no DQT and no SOS.
 * Every frame's bytes begin with DQT 0, DQT 1 of its group's q* (the IJG scaling
 * dvc_jpeg_create applies), then SOS - with optimised tables the group's DHT,
 * then SOS - and go on with the entropy data and EOI, so header + frame is a
 * complete baseline image. dvc_jpeg_encode, dvc_jpeg_encode_stream,
 * dvc_jpeg_sync and dvc_jpeg_destroy take the handle as any other; a
 * device-pointer call stays asynchronous.
 * DVC_E_INVALID for target_bytes == 0, a range outside 1 <= q_min <= q_max <=
 * 100 and whatever dvc_jpeg_create refuses. */
int dvc_jpeg_create_rate(int width, int height, int fmt, size_t target_bytes, int q_min, int q_max, int max_batch,
                         int device, void* hip_stream, uint32_t flags, dvc_jpeg** out);

/* Wait for the handle's stream and copy the counters. DVC_E_STATE on a handle
 * that dvc_jpeg_create made or that has no device. */
int dvc_jpeg_rate_stats(dvc_jpeg* h, struct dvc_jpeg_rate_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* DVC_JPEG_RATE_H */
