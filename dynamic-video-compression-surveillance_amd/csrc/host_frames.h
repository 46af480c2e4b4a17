// host_frames.h — the frame contract of include/dvc.h in one place: what a
// frame handed to a prime / step / convert call spans, which pitches it may
// have, how a host frame is packed for its upload, when the kernels can read
// device frames in place, and how a bit plane reads back. Plain C++17 (no HIP):
// tools/host_frames_check.cc runs it under the host sanitizers. Internal.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/dvc.h"

namespace dvc {

// A batch of 4:2:0 frames: frame t's luma rows at base + t*fstride (ypitch
// bytes each), its chroma row r's U / V samples at base + t*fstride + uoff /
// voff + r*cpitch, cstep bytes apart (1: I420 planes, 2: NV12's UV plane).
struct YuvLayout {
    const uint8_t* base;
    size_t ypitch, uoff, voff, cpitch, fstride;
    int cstep;
};

// The YuvLayout of a DVC_FMT_I420 / DVC_FMT_NV12 frame (include/dvc.h): luma
// rows of `pitch` bytes, the chroma plane(s) after `crows` luma rows.
inline YuvLayout yuv_layout(const uint8_t* base, size_t pitch, int fmt, int crows, size_t fstride)
{
    YuvLayout L{};
    L.base = base;
    L.ypitch = pitch;
    L.fstride = fstride;
    L.uoff = pitch * (size_t)crows;
    if (fmt == DVC_FMT_NV12) {
        L.voff = L.uoff + 1;
        L.cpitch = pitch;
        L.cstep = 2;
    } else {
        L.cpitch = pitch / 2;
        L.voff = L.uoff + L.cpitch * (size_t)(crows / 2);
        L.cstep = 1;
    }
    return L;
}

// Bytes one such frame spans: pitch * crows * 3 / 2.
inline size_t yuv_frame_bytes(size_t pitch, int crows) { return pitch * (size_t)crows * 3 / 2; }

}  // namespace dvc

namespace dvc_host {

// Frames as a caller hands them over: DVC_FMT_*, w x h pixels, and for 4:2:0
// the luma rows before the chroma plane(s).
struct FrameFmt {
    int fmt, w, h, crows;
};

// BGR rows of `pitch` >= 3w, or 4:2:0 surfaces (luma pitch >= w; I420: even).
inline bool pitch_ok(const FrameFmt& f, size_t pitch)
{
    if (f.fmt == DVC_FMT_BGR) return pitch >= 3 * (size_t)f.w;
    return pitch >= (size_t)f.w && (f.fmt != DVC_FMT_I420 || pitch % 2 == 0);
}

// Bytes a frame spans (rows of `pitch`): BGR rows, the last one 3w bytes, or a
// 4:2:0 frame's luma + chroma planes.
inline size_t frame_span(const FrameFmt& f, size_t pitch)
{
    if (f.fmt == DVC_FMT_BGR) return pitch * ((size_t)f.h - 1) + 3 * (size_t)f.w;
    return dvc::yuv_frame_bytes(pitch, f.crows);
}

// Copy host frame `src` into pinned staging `dst` in the compact layout the
// staged device copy is read with: BGR rows of dst_bgr_pitch; 4:2:0: luma rows
// of w and the chroma plane(s) right after them.
inline void pack_host_frame(const FrameFmt& f, const uint8_t* src, size_t pitch, uint8_t* dst, size_t dst_bgr_pitch)
{
    const size_t w = f.w, h = f.h;
    if (f.fmt == DVC_FMT_BGR) {
        for (size_t y = 0; y < h; ++y) std::memcpy(dst + y * dst_bgr_pitch, src + y * pitch, 3 * w);
        return;
    }
    const dvc::YuvLayout L = dvc::yuv_layout(src, pitch, f.fmt, f.crows, 0);
    const dvc::YuvLayout C = dvc::yuv_layout(dst, w, f.fmt, (int)h, 0);
    for (size_t y = 0; y < h; ++y) std::memcpy(dst + y * w, src + y * pitch, w);
    const size_t cb = f.fmt == DVC_FMT_NV12 ? w : w / 2;   // chroma bytes per row and plane
    for (size_t y = 0; y < h / 2; ++y) {
        std::memcpy(dst + C.uoff + y * C.cpitch, src + L.uoff + y * L.cpitch, cb);
        if (f.fmt == DVC_FMT_I420) std::memcpy(dst + C.voff + y * C.cpitch, src + L.voff + y * L.cpitch, cb);
    }
}

// Can the kernels read n device frames in place? Dword rows (pitch % 4 == 0)
// of at least min_pitch bytes, aligned base and frame stride, and W % 4 == 0:
// a frame's last row then ends exactly at its last 4-px quad, so a buffer
// sized to the frame span is never read past its end.
inline bool readable_in_place(int W, const void* p, size_t pitch, size_t min_pitch, size_t fstride, int n)
{
    return W % 4 == 0 && pitch % 4 == 0 && pitch >= min_pitch && ((uintptr_t)p & 3) == 0 &&
           (n <= 1 || fstride % 4 == 0);
}

// A bit plane (H rows of WW 64-bit words, bit x % 64 of word x / 64) as a
// 0 / 255 byte plane of W x H.
inline void expand_bit_plane(const uint64_t* bits, size_t W, size_t H, size_t WW, uint8_t* dst)
{
    for (size_t y = 0; y < H; ++y)
        for (size_t x = 0; x < W; ++x) dst[y * W + x] = ((bits[y * WW + x / 64] >> (x % 64)) & 1) ? 255 : 0;
}

}  // namespace dvc_host
