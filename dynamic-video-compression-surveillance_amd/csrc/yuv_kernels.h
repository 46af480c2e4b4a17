// yuv_kernels.h — 4:2:0 YUV <-> packed BGR conversion kernels (video I/O,
// SURVEY.md §8f #1). Internal launch interface; the C-ABI is in include/dvc.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_frames.h"   // YuvLayout, yuv_layout, yuv_frame_bytes

namespace dvc {

// cvtColor COLOR_YUV2BGR_I420 / _NV12 of n W x H frames (W, H even) into
// packed BGR rows of dpitch bytes, frames dstride apart.
hipError_t launch_yuv420_to_bgr(const YuvLayout& s, int W, int H, int n, uint8_t* dst, size_t dpitch, size_t dstride,
                                hipStream_t st);

// cvtColor COLOR_BGR2YUV_I420 of n W x H packed BGR frames (rows of spitch,
// frames sstride apart) into I420 frames laid out as `d` (cstep 1).
hipError_t launch_bgr_to_i420(const uint8_t* src, size_t spitch, size_t sstride, int W, int H, int n,
                              const YuvLayout& d, hipStream_t st);

}  // namespace dvc
