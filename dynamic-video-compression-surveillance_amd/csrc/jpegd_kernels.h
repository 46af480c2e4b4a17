// jpegd_kernels.h — baseline-JPEG decoder kernels (DESIGN.md "Motion-JPEG
// decoder"). Internal launch interface; the C-ABI is in include/dvc.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpegd_core.h"

namespace dvc {

// Chunks a frame's bytes are split into to find its restart markers.
constexpr int kJpegdChunks = 32;

// Work buffers for max_batch frames of the handle's largest size (frame f's
// part at f * the per-frame count of the current geometry).
struct JpegdBufs {
    int16_t* coef;       // mcus * bpm * 64 levels, natural order, blocks in scan order
    uint32_t* chunkcnt;  // kJpegdChunks: the RSTn markers in each chunk of the frame's bytes
    uint32_t* markpos;   // nseg: byte offsets of the frame's RSTn markers (nseg - 1 used)
    uint8_t* planes;     // yw*yh luma, then cw*ch Cb and cw*ch Cr
    int32_t* first_err;  // one word: the first damaged frame's status since the last dvc_jpegd_sync
};

// Frame t's entropy data: data + t * stride, sizes[t] bytes; status[t] receives 0
// or a negative code. All pointers are device pointers.
hipError_t jpegd_launch(const uint8_t* data, size_t stride, const uint32_t* sizes, int n, const JpegdGeom& g,
                        const JpegdTables* tab, const JpegdBufs& b, uint8_t* out, size_t pitch, size_t fstride,
                        int32_t* status, hipStream_t st);

}  // namespace dvc
