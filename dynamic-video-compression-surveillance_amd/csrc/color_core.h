// color_core.h — the one copy of the project's fixed-point colour arithmetic, as
// plain C++ for the device (px_device.h, quality_core.h) and for the host
// (tools/color_host_check.cc sweeps it over all 2^24 inputs against the oracle
// under the host sanitizers, tests/test_color.py): OpenCV's 14-bit BGR2GRAY /
// BGR2YCrCb / YCrCb2BGR (oracle/dvc_oracle.c), OpenCV 4.11's 20-bit BT.601
// cvtColor YUV2BGR_I420 / _NV12 and BGR2YUV_I420 (namespace yuvpx;
// oracle/yuv_oracle.c), and the gray of four packed pixels on the v_dot4 unit.
#pragma once
#include <stdint.h>

#ifndef DVC_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DVC_HD __host__ __device__ __forceinline__
#else
#define DVC_HD inline
#endif
#endif

namespace dvc {

// ------------------------------------------------ 14 bit: gray and YCrCb ----
constexpr int kB2Y = 1868, kG2Y = 9617, kR2Y = 4899;                           // BGR -> Y (= BGR2GRAY)
constexpr int kR2Cr = 11682, kB2Cb = 9241;                                     // (R - Y) -> Cr, (B - Y) -> Cb
constexpr int kCb2B = 29049, kCb2G = -5636, kCr2G = -11698, kCr2R = 22987;     // YCrCb -> BGR
static_assert(kB2Y + kG2Y + kR2Y == 1 << 14, "Y of a u8 pixel is in 0..255: no saturation");
static_assert(kB2Y < 65536 && kG2Y < 65536 && kR2Y < 65536, "luma coefficients: two bytes each (luma4)");

DVC_HD int descale14(int v) { return (v + 8192) >> 14; }
DVC_HD uint32_t satu8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// OpenCV BGR2GRAY 8U: (1868 B + 9617 G + 4899 R + 2^13) >> 14
DVC_HD uint32_t gray_px(uint32_t b, uint32_t g, uint32_t r)
{
    return (b * (uint32_t)kB2Y + g * (uint32_t)kG2Y + r * (uint32_t)kR2Y + 8192u) >> 14;
}

// BGR2YCrCb, YCrCb2BGR of a pixel, chroma centred (cr, cb in -128..127: what the inverse multiplies, the round trip composes)
DVC_HD void bgr_to_ycc(int b, int g, int r, int& y, int& cr, int& cb)
{
    y = (int)gray_px((uint32_t)b, (uint32_t)g, (uint32_t)r);
    cr = (int)satu8(descale14((r - y) * kR2Cr + (128 << 14))) - 128;
    cb = (int)satu8(descale14((b - y) * kB2Cb + (128 << 14))) - 128;
}
DVC_HD void ycc_to_bgr(int y, int cr, int cb, uint8_t* bgr)
{
    bgr[0] = (uint8_t)satu8(y + descale14(cb * kCb2B));
    bgr[1] = (uint8_t)satu8(y + descale14(cb * kCb2G + cr * kCr2G));
    bgr[2] = (uint8_t)satu8(y + descale14(cr * kCr2R));
}

// the same on bytes: y, cr, cb in 0..255
DVC_HD void bgr_to_ycrcb(int b, int g, int r, int& y, int& cr, int& cb)
{
    bgr_to_ycc(b, g, r, y, cr, cb);
    cr += 128, cb += 128;
}
DVC_HD void ycrcb_to_bgr(int y, int cr, int cb, uint8_t* bgr) { ycc_to_bgr(y, cr - 128, cb - 128, bgr); }

// the compressed frame's pixel where its block is not static (fd:115-130)
DVC_HD void ycrcb_round_trip(int b, int g, int r, uint8_t* bgr)
{
    int y, cr, cb;
    bgr_to_ycc(b, g, r, y, cr, cb);
    ycc_to_bgr(y, cr, cb, bgr);
}

// ------------------------------------------------------ 20 bit: BT.601 ------
namespace yuvpx {

constexpr int CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527;
constexpr int CRY = 269484, CGY = 528482, CBY = 102760, CRU = -155188, CGU = -305135, CBU = 460324, CGV = -385875,
              CBV = -74448;
constexpr int SHIFT = 20, HALF = 1 << (SHIFT - 1);
static_assert((CBY >> 24) == 0 && (CGY >> 24) == 0 && (CRY >> 24) == 0 && CBY > 0 && CGY > 0 && CRY > 0,
              "luma coefficients: three bytes each (luma4_i420)");
static_assert((255 * (CBY + CGY + CRY) + HALF + (16 << SHIFT)) >> SHIFT <= 255, "luma never saturates");
static_assert(CRU + CGU + CBU == 1 && CBU + CGV + CBV == 1, "a gray pixel (R = G = B) has U = V = 128");

// BGR2YUV_I420: luma of a pixel, chroma of the top-left pixel of a 2x2 quad
DVC_HD uint32_t luma(int b, int g, int r) { return satu8((CRY * r + CGY * g + CBY * b + HALF + (16 << SHIFT)) >> SHIFT); }
DVC_HD uint32_t chroma_u(int b, int g, int r) { return satu8((CRU * r + CGU * g + CBU * b + HALF + (128 << SHIFT)) >> SHIFT); }
DVC_HD uint32_t chroma_v(int b, int g, int r) { return satu8((CBU * r + CGV * g + CBV * b + HALF + (128 << SHIFT)) >> SHIFT); }

// YUV2BGR_I420 / _NV12 of one pixel: Y and its 2x2 quad's (u, v)
DVC_HD void yuv_px_bgr(int y, int u, int v, int& b, int& g, int& r)
{
    const int cu = u - 128, cv = v - 128, y16 = y - 16, yy = (y16 > 0 ? y16 : 0) * CY;
    b = (int)satu8((yy + HALF + CUB * cu) >> SHIFT);
    g = (int)satu8((yy + HALF + CVG * cv + CUG * cu) >> SHIFT);
    r = (int)satu8((yy + HALF + CVR * cv) >> SHIFT);
}

}  // namespace yuvpx

// ---- four packed pixels on the dot4 unit: luma4 and pack4 are written with three intrinsics, plain C++ on the host
#if defined(__HIPCC__)
#define DVC_DEV __device__ __forceinline__
DVC_DEV uint32_t px_udot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }
DVC_DEV uint32_t px_alignbyte(uint32_t hi, uint32_t lo, uint32_t n) { return __builtin_amdgcn_alignbyte(hi, lo, n); }
DVC_DEV uint32_t px_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#else
#define DVC_DEV inline
inline uint32_t px_udot4(uint32_t a, uint32_t b, uint32_t c)   // c + sum of the byte products
{
    for (int k = 0; k < 32; k += 8) c += ((a >> k) & 255u) * ((b >> k) & 255u);
    return c;
}
inline uint32_t px_alignbyte(uint32_t h, uint32_t l, uint32_t n) { return (uint32_t)((((uint64_t)h << 32) | l) >> (8 * (n & 3))); }
inline uint32_t px_perm(uint32_t hi, uint32_t lo, uint32_t sel)   // 0-3: lo, 4-7: hi, 0x0c: zero (v_perm's other selectors: unused, not modelled)
{
    uint32_t d = 0;
    for (int k = 0; k < 32; k += 8)
        d |= (((sel >> k) & 255u) < 8 ? (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * ((sel >> k) & 7))) & 255u : 0u) << k;
    return d;
}
#endif

// four bytes (each < 256) into a dword with v_perm: written as shifts and ORs, hipcc (ROCm 7.2) folds pairs of
// satu8(x >> 20) into v_ashr_pk_u8_i32, which keeps the upper half of its destination register, and the ORs
// then pick that garbage up (measured: every 4th converted pixel wrong)
DVC_DEV uint32_t pack4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3)
{
    const uint32_t lo = px_perm(b1, b0, 0x0c0c0400u);
    const uint32_t hi = px_perm(b3, b2, 0x0c0c0400u);
    return px_perm(hi, lo, 0x05040100u);
}

// gray_px of 4 packed BGR pixels (12 bytes = 3 dwords, little endian) with the v_dot4_u32_u8 unit: each
// coefficient split as 256 * hi + lo, so Y * 2^14 + 2^13 = (dot4(px, hi) << 8) + dot4(px, lo) + 2^13 per pixel
// (byte 3 of each operand is multiplied by 0); v_alignbyte puts pixel i's (b, g, r) at bytes 0..2.
DVC_DEV uint32_t luma_dot(uint32_t p)
{
    constexpr uint32_t LO = (kB2Y & 255) | ((kG2Y & 255) << 8) | ((kR2Y & 255) << 16);
    constexpr uint32_t HI = (kB2Y >> 8) | ((kG2Y >> 8) << 8) | ((kR2Y >> 8) << 16);
    return ((px_udot4(p, HI, 0u) << 8) + px_udot4(p, LO, 8192u)) >> 14;
}
DVC_DEV void luma4(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t (&y)[4])
{
    const uint32_t p[4] = {d0, px_alignbyte(d1, d0, 3), px_alignbyte(d2, d1, 2), d2 >> 8};
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = luma_dot(p[j]);
}

}  // namespace dvc
