// px_device.h — packed pixels on the device (gfx950): color_core.h's arithmetic on rows of packed BGR
// bytes and on 4:2:0 surfaces read in place, with their loads and stores. Users: fd_kernels.hip (k_gray,
// k_front, k_out, k_fix4, k_out_gen), of_kernels.hip (k_of_front0: load_quad / quad_gray; k_of_out), yuv_kernels.hip.
#pragma once
#include "../../include/dvc.h"
#include "color_core.h"
#include "fd_kernels.h"

namespace dvc {

// channel c (0 B, 1 G, 2 R) of pixel j of a row of packed BGR dwords
__device__ __forceinline__ uint32_t bgr_at(const uint32_t* px, int j, int c)
{
    return (px[(3 * j + c) >> 2] >> (8 * ((3 * j + c) & 3))) & 255;
}

// four bytes -> dword, little endian (pack4: the same from four u32 with v_perm)
__device__ __forceinline__ uint32_t pack_bytes(uint8_t b0, uint8_t b1, uint8_t b2, uint8_t b3)
{
    return b0 | (b1 << 8) | (b2 << 16) | ((uint32_t)b3 << 24);
}

// 4 packed BGR pixels (3 dwords, little endian) -> 4 packed gray bytes: gray_px of each on the v_dot4 unit (luma_dot)
__device__ __forceinline__ uint32_t gray4_dot(uint32_t d0, uint32_t d1, uint32_t d2)
{
    const uint32_t p1 = __builtin_amdgcn_alignbyte(d1, d0, 3), p2 = __builtin_amdgcn_alignbyte(d2, d1, 2);
    const uint32_t p3 = d2 >> 8;
    const uint32_t lo = __builtin_amdgcn_perm(luma_dot(p1), luma_dot(d0), 0x0c0c0400u);
    const uint32_t hi = __builtin_amdgcn_perm(luma_dot(p3), luma_dot(p2), 0x0c0c0400u);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

// 4 bytes v0..v3 (low byte of each u32) -> 4 gray pixels as the 3 dwords of packed BGR
__device__ __forceinline__ void gray_bgr4(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t* out)
{
    const uint32_t V = __builtin_amdgcn_perm(__builtin_amdgcn_perm(v3, v2, 0x0c0c0400u),
                                             __builtin_amdgcn_perm(v1, v0, 0x0c0c0400u), 0x05040100u);
    out[0] = __builtin_amdgcn_perm(V, V, 0x01000000u);
    out[1] = __builtin_amdgcn_perm(V, V, 0x02020101u);
    out[2] = __builtin_amdgcn_perm(V, V, 0x03030302u);
}

// One row of a B-pixel block (3 B / 4 dwords of packed BGR) through ycrcb_round_trip
template <int B>
__device__ __forceinline__ void ycrcb_round_trip_row(const uint32_t* px, uint32_t* cw)
{
    uint8_t ob[3 * B];
#pragma unroll
    for (int j = 0; j < B; ++j)
        ycrcb_round_trip((int)bgr_at(px, j, 0), (int)bgr_at(px, j, 1), (int)bgr_at(px, j, 2), ob + 3 * j);
#pragma unroll
    for (int d = 0; d < 3 * B / 4; ++d) cw[d] = pack_bytes(ob[4 * d], ob[4 * d + 1], ob[4 * d + 2], ob[4 * d + 3]);
}

namespace yuvpx {

// 4 px of one row (x even), chroma (u0, v0) for px 0-1 and (u1, v1) for px 2-3 -> 12 packed BGR bytes as 3 dwords
__device__ __forceinline__ void yuv4_bgr(uint32_t y4, int u0, int v0, int u1, int v1, uint32_t o[3])
{
    uint32_t p[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int b, g, r;
        yuv_px_bgr((int)((y4 >> (8 * j)) & 255), j < 2 ? u0 : u1, j < 2 ? v0 : v1, b, g, r);
        p[3 * j] = (uint32_t)b;
        p[3 * j + 1] = (uint32_t)g;
        p[3 * j + 2] = (uint32_t)r;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) o[d] = pack4(p[4 * d], p[4 * d + 1], p[4 * d + 2], p[4 * d + 3]);
}

}  // namespace yuvpx

// Reading a 4-px quad (x % 4 == 0) of a frame in place (SrcFmt, fd_kernels.h). chroma_off: byte offset in a 4:2:0
// frame of the chroma of pixel (x, y), x even — I420: its U sample (V: voff - uoff further); NV12: its UV pair.
template <int FMT>
__device__ __forceinline__ size_t chroma_off(const SrcFmt& sf, int y, int x)
{
    return sf.uoff + (size_t)(y >> 1) * sf.cpitch + (FMT == DVC_FMT_NV12 ? x : x >> 1);
}
// any x, the format at run time
__device__ __forceinline__ size_t chroma_off(const SrcFmt& sf, int y, int x)
{
    return sf.fmt == DVC_FMT_NV12 ? chroma_off<DVC_FMT_NV12>(sf, y, x & ~1) : chroma_off<DVC_FMT_I420>(sf, y, x);
}

// The quad as loaded: 12 packed BGR bytes at p (a, b, c), or a 4:2:0 quad — its luma dword at p (a) and its chroma at
// pc (chroma_off): I420 the u16 of U (b) and of V (c), dv = voff - uoff apart; NV12 the dword U0 V0 U1 V1 (b).
template <int FMT, typename O>
__device__ __forceinline__ void load_quad(const uint8_t* p, const uint8_t* pc, O dv, uint32_t& a, uint32_t& b, uint32_t& c)
{
    if constexpr (FMT == DVC_FMT_BGR) {
        const uint3 q = *reinterpret_cast<const uint3*>(p);
        a = q.x; b = q.y; c = q.z;
    } else if constexpr (FMT == DVC_FMT_NV12) {
        a = *reinterpret_cast<const uint32_t*>(p);
        b = *reinterpret_cast<const uint32_t*>(pc);
        c = 0;
    } else {
        a = *reinterpret_cast<const uint32_t*>(p);
        b = *reinterpret_cast<const uint16_t*>(pc);
        c = *reinterpret_cast<const uint16_t*>(pc + dv);
    }
}

// a loaded 4:2:0 quad -> 12 packed BGR bytes (cvtColor YUV2BGR)
template <int FMT>
__device__ __forceinline__ void quad_bgr(uint32_t y4, uint32_t c1, uint32_t c2, uint32_t o[3])
{
    if constexpr (FMT == DVC_FMT_NV12) yuvpx::yuv4_bgr(y4, c1 & 255, (c1 >> 8) & 255, (c1 >> 16) & 255, c1 >> 24, o);
    else yuvpx::yuv4_bgr(y4, c1 & 255, c2 & 255, (c1 >> 8) & 255, (c2 >> 8) & 255, o);
}

// gray of a loaded quad: 12 BGR bytes (v0..v2), or a 4:2:0 quad via quad_bgr
template <int FMT>
__device__ __forceinline__ uint32_t quad_gray(uint32_t v0, uint32_t v1, uint32_t v2)
{
    if constexpr (FMT == DVC_FMT_BGR) {
        return gray4_dot(v0, v1, v2);
    } else {
        uint32_t o[3];
        quad_bgr<FMT>(v0, v1, v2, o);
        return gray4_dot(o[0], o[1], o[2]);
    }
}

// One row of a BxB block of an output frame as the encoder's 4:2:0 input (cvtColor BGR2YUV_I420, include/dvc.h
// DVC_FLAG_OUT_I420): B luma bytes, and on even rows the B/2 chroma samples of the 2x2 quads (their top-left
// pixel). I420 frame at f: Y plane W x H, then U and V planes of W/2 x H/2.
template <int B>
__device__ __forceinline__ void store_i420_row(uint8_t* f, int W, int H, int y, int x, const uint32_t* w)
{
    using namespace yuvpx;
    uint32_t yv[B], uv[B / 2], vv[B / 2];
#pragma unroll
    for (int j = 0; j < B; ++j) {
        const int b = (int)bgr_at(w, j, 0), g = (int)bgr_at(w, j, 1), r = (int)bgr_at(w, j, 2);
        yv[j] = luma(b, g, r);
        if (!(j & 1)) {
            uv[j >> 1] = chroma_u(b, g, r);
            vv[j >> 1] = chroma_v(b, g, r);
        }
    }
    uint32_t* yo = reinterpret_cast<uint32_t*>(f + (size_t)y * W + x);
#pragma unroll
    for (int d = 0; d < B / 4; ++d)
        __builtin_nontemporal_store(pack4(yv[4 * d], yv[4 * d + 1], yv[4 * d + 2], yv[4 * d + 3]), yo + d);
    if (!(y & 1)) {
        const size_t c = (size_t)W * H + (size_t)(y >> 1) * (W >> 1) + (x >> 1), q = (size_t)(W >> 1) * (H >> 1);
        if constexpr (B == 4) {
            __builtin_nontemporal_store((uint16_t)(uv[0] | (uv[1] << 8)), reinterpret_cast<uint16_t*>(f + c));
            __builtin_nontemporal_store((uint16_t)(vv[0] | (vv[1] << 8)), reinterpret_cast<uint16_t*>(f + c + q));
        } else {
#pragma unroll
            for (int d = 0; d < B / 8; ++d) {
                __builtin_nontemporal_store(pack4(uv[4 * d], uv[4 * d + 1], uv[4 * d + 2], uv[4 * d + 3]),
                                            reinterpret_cast<uint32_t*>(f + c) + d);
                __builtin_nontemporal_store(pack4(vv[4 * d], vv[4 * d + 1], vv[4 * d + 2], vv[4 * d + 3]),
                                            reinterpret_cast<uint32_t*>(f + c + q) + d);
            }
        }
    }
}

// BGR2YUV_I420 luma of the 4 packed BGR pixels of a quad row (dwords d0..d2), as v_dot4 with the 20-bit coefficients
// split into bytes: the same integer as yuvpx::luma (no saturation needed: 16 <= Y <= 235 for every BGR).
__device__ __forceinline__ uint32_t luma4_i420(uint32_t d0, uint32_t d1, uint32_t d2)
{
    using namespace yuvpx;
    constexpr uint32_t K0 = (CBY & 255) | ((CGY & 255) << 8) | ((CRY & 255) << 16);
    constexpr uint32_t K1 = ((CBY >> 8) & 255) | (((CGY >> 8) & 255) << 8) | (((CRY >> 8) & 255) << 16);
    constexpr uint32_t K2 = (CBY >> 16) | ((CGY >> 16) << 8) | ((CRY >> 16) << 16);
    const uint32_t p[4] = {d0, __builtin_amdgcn_alignbyte(d1, d0, 3), __builtin_amdgcn_alignbyte(d2, d1, 2), d2 >> 8};
    uint32_t y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t t2 = __builtin_amdgcn_udot4(p[j] & 0x00ffffffu, K2, 0u, false);
        const uint32_t t1 = __builtin_amdgcn_udot4(p[j] & 0x00ffffffu, K1, t2 << 8, false);
        y[j] = __builtin_amdgcn_udot4(p[j] & 0x00ffffffu, K0, (t1 << 8) + (uint32_t)(HALF + (16 << SHIFT)), false) >> SHIFT;
    }
    return pack4(y[0], y[1], y[2], y[3]);
}
// chroma of pixels 0 and 2 of the quad row (top-left of its two 2x2 quads): U0 | U2 << 8 low half, V0 | V2 << 8 high half
__device__ __forceinline__ uint32_t chroma2_i420(uint32_t d0, uint32_t d1, uint32_t d2)
{
    using namespace yuvpx;
    const int b0 = d0 & 255, g0 = (d0 >> 8) & 255, r0 = (d0 >> 16) & 255;
    const int b2 = (d1 >> 16) & 255, g2 = d1 >> 24, r2 = d2 & 255;   // bytes 6, 7, 8
    return chroma_u(b0, g0, r0) | (chroma_u(b2, g2, r2) << 8) | (chroma_v(b0, g0, r0) << 16) |
           (chroma_v(b2, g2, r2) << 24);
}

}  // namespace dvc
