/* dvc_quality_regions.h - the quality meter's figures (include/dvc.h, dvc_quality_*)
 * split into the regions the workers treat differently. An addition to the
 * C-ABI of dvc.h, version 10, exported by the same library; it is a header of
 * its own because dvc.h's set of prototypes is pinned. DESIGN.md "Quality
 * metrics", "Kept and static regions" is the normative text. */
#ifndef DVC_QUALITY_REGIONS_H
#define DVC_QUALITY_REGIONS_H

#include "dvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same figures split into the regions the workers treat differently: the
 * blocks they flattened (static) and the blocks they kept. A mask frame is one
 * byte a pixel (the DVC_FMT_GRAY layout). On the grid of block x block pixels
 * anchored at (0, 0) a block is static iff every mask byte of it inside the
 * frame is 0 (any other value counts), and a partial block on the right or
 * bottom edge obeys the same rule with partial_static = 1 (fd:117-120: the
 * slices are clipped and mean() == 0 is tested) and is always kept with
 * partial_static = 0 (of:156-161: partial blocks are skipped). A pixel has the
 * class of its block; an SSIM window is static or kept when all its 64 pixels
 * are, mixed otherwise. For every input sse[0][i] + sse[1][i], pixels[0] +
 * pixels[1], the sum of ssim_q32[] and the sum of windows[] equal
 * dvc_quality_frame's sse[i], pixels, ssim_q32 and windows. */
typedef struct dvc_quality_regions {
    uint64_t sse[2][4];    /* [class][B, G, R, luma]; class 0 kept, 1 static */
    int64_t  ssim_q32[3];  /* kept, static, mixed windows */
    uint32_t windows[3];
    uint32_t pixels[2];
    uint32_t reserved;     /* 0 */
} dvc_quality_regions;     /* 112 bytes */

/* dvc_quality_compare with mask frame t at mask + t*mask_stride in rows of
 * mask_pitch >= W bytes (any pitch and alignment, read once and in place), block
 * in 1..128 and partial_static 0 or 1; pointers, alignment of the records and the
 * stream are dvc_quality_compare's. The first call allocates the handle's class
 * bits and partial sums. */
int dvc_quality_compare_regions(dvc_quality* h, const uint8_t* ref, size_t ref_pitch, size_t ref_stride,
                                const uint8_t* test, size_t test_pitch, size_t test_stride, const uint8_t* mask,
                                size_t mask_pitch, size_t mask_stride, int block, int partial_static, int n,
                                dvc_quality_regions* results);

#ifdef __cplusplus
}
#endif

#endif /* DVC_QUALITY_REGIONS_H */
