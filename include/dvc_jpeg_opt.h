/* dvc_jpeg_opt.h - the table builder of the Motion-JPEG encoder's optimised
 * Huffman tables (include/dvc.h, dvc_jpeg_*, DVC_FLAG_JPEG_OPT_HUFFMAN) on
 * counts of the caller's. An addition to the C-ABI of dvc.h, version 10,
 * exported by the same library; it is a header of its own because dvc.h's set of
 * prototypes is pinned. DESIGN.md "Motion-JPEG stream", "Optimised Huffman
 * tables" is the normative text. */
#ifndef DVC_JPEG_OPT_H
#define DVC_JPEG_OPT_H

#include "dvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Run the handle's table builder on caller-supplied counts (host pointer,
 * counts[4][256] in the order DC class 0, AC class 0, DC class 1, AC class 1;
 * DC rows use entries 0..11) and return the DHT segment it would write: *n
 * receives its length, dht may be NULL to query it, DVC_E_NOMEM when cap is
 * smaller. Synchronous, on the handle's stream behind what was enqueued there.
 * DVC_E_STATE on a handle without the flag or without a device;
 * DVC_E_INVALID for a non-zero count on a symbol the coder cannot emit
 * (DC size > 11; AC size 0 other than 0x00 / 0xF0; AC size > 10), for a class 1
 * count on a DVC_FMT_GRAY handle, for counts that are all zero and for counts
 * whose sum reaches 2^62. */
int dvc_jpeg_opt_tables(dvc_jpeg* h, const uint64_t* counts, uint8_t* dht, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif

#endif /* DVC_JPEG_OPT_H */
