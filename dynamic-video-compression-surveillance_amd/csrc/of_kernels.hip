// of_kernels.hip — gfx950 (MI355X / CDNA4) kernels of the optical-flow (OF)
// per-frame worker (reference: motion_compression_opt.py:65-101, 141-185).
//
// One batch of n consecutive frames = these launches (of_kernels.h):
//   k_of_front0   BGR->gray (of:71), level-0 smoothing (3 taps, sigma 0) and
//                 FarnebackPolyExp -> R of level 0 (5 floats / px)
//   k_pyr_h       level k > 0: horizontal Gaussian pass at the source columns
//                 the INTER_LINEAR resize reads
//   k_pyr_poly    level k > 0: vertical pass + resize + FarnebackPolyExp
//   k_flow        per level (coarse to fine) and iteration: the flow of the
//                 previous iteration (or the upsampled coarser flow) ->
//                 FarnebackUpdateMatrices over the tile + box halo in LDS ->
//                 box-filtered G, h (double, direct sums) -> flow = G^-1 h
//                 (FarnebackUpdateFlow_Blur); the finest level's last
//                 iteration emits |flow| > thr as bits (of:82-83)
//   k_vote        sliding 30-frame vote (of:84-86), frames in order per tile
//   k_of_band     MORPH_CLOSE + MORPH_OPEN with the 2x2 ellipse (of:89-90) on
//                 a band of rows, then its 8-connected runs + union-find in LDS
//   k_of_merge    band seams -> global unions
//   k_of_bbox     bounding box per component (of:93-96), roots compacted
//   k_of_rect     rectangles (x0..x1+1, y0..y1+1) OR-painted (of:97)
//   k_of_out      static 8x8 blocks: DCT quantisation of Y, Cr, Cb, YCrCb->BGR,
//                 BGR->gray->BGR (of:151-183), + the rectangle mask bytes
//
// Every float/double expression follows oracle/of_oracle.c operation by
// operation (compiled with -ffp-contract=off on both sides), so the flow, and
// with it every mask bit, is identical to the oracle's. No MFMA: nothing here
// is a dense contraction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <type_traits>
#include <cstdlib>
#include <cstring>

#include "../../include/dvc.h"
#include "dvc_device.h"
#include "of_kernels.h"
#include "dct_const.h"
#include "px_device.h"
#include "tune.h"

namespace dvc {

// R (5 floats a pixel, 20 B: only 4-B aligned) read with dwordx4/x2 loads
// (unaligned global access is on under ROCm): 2 loads for a pixel's 5
// channels, 3 for two adjacent pixels' 10, instead of 5 and 10 dword loads —
// the address rate (TA), not the bytes, bounds the M gathers.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ void ld5(const float* p, float* o)
{
    const f4u a = *reinterpret_cast<const f4u*>(p);
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w, o[4] = p[4];
}
__device__ __forceinline__ void ld10(const float* p, float* o)
{
    const f4u a = *reinterpret_cast<const f4u*>(p), b = *reinterpret_cast<const f4u*>(p + 4);
    const f2u c = *reinterpret_cast<const f2u*>(p + 8);
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w, o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w, o[8] = c.x,
    o[9] = c.y;
}

// FarnebackUpdateMatrices' border weights {0.14, 0.14, 0.4472, 0.4472, 0.4472}
// for distance d (0..4) from the image edge, as a select instead of a memory
// table (a table load is a vector memory op: waiting for it waits for every
// prefetch issued before it)
__device__ __forceinline__ float border_w(int d) { return d < 2 ? 0.14f : 0.4472f; }

namespace {

constexpr int PT_W = 64, PT_H = 16;   // poly-expansion tile (level pixels)
constexpr int FL_W = 32, FL_H = 16;   // flow tile (32 wide: <= 26 KB LDS, 6 workgroups per CU)

// Ring slot of frame number a. The launchers pass frame numbers through
// reduce_frame(), which keeps them below 2^31, so the modulo is 32-bit (a 64-bit
// one is a long VALU + SALU expansion per workgroup).
__device__ __forceinline__ int ring(long long a, int n)
{
    const int r = (int)a % n;
    return r < 0 ? r + n : r;
}

// ------------------------------------------------- polynomial expansion -----
// Steps C and D of FarnebackPolyExp (oc_poly_exp) for one tile whose smoothed
// level image I is in LDS at rows [y0-PN, y0+PT_H-1+PN], cols [x0-PN, ...]
// (in-image entries only), rows of SI floats. sv: PT_H x SV positions x 3
// floats. INT: the tile and its PN halo lie inside the image (no clamping;
// LDS offsets are constants). VEC (INT tiles, SI and SV multiples of 4): the
// vertical part over groups of 4 columns as float4 vectors — the same float
// operations per element in the same order (-ffp-contract=off), packed
// (v_pk_mul_f32 / v_pk_add_f32) and read / written 16 B at a time.
typedef float f4v __attribute__((ext_vector_type(4)));
template <int PN, bool INT, int SI = PT_W + 2 * PN, int SV = PT_W + 2 * PN, bool VEC = false>
__device__ __forceinline__ void poly_tile(const float* sI, float* sv, const PolyCoef& pc, int x0, int y0, int w,
                                          int h, float* __restrict__ R)
{
    constexpr int IW = PT_W + 2 * PN;
    static_assert(!VEC || (INT && SI % 4 == 0 && SV % 4 == 0 && SI >= IW + 3 - (IW + 3) % 4 && SV >= SI),
                  "vector rows: 16-B aligned, whole groups of 4");
    const int tid = threadIdx.x;
    if constexpr (VEC) {
        constexpr int NG = (IW + 3) / 4;   // column groups (the last one's extra columns are row padding)
        // the taps as scalar values (readfirstlane: otherwise the compiler
        // vectorises their kernel-argument loads through a private copy)
        auto tap = [](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); };
        for (int it = tid; it < PT_H * NG; it += 256) {
            const int i = it / NG, j = 4 * (it - i * NG), li = i + PN;
            f4v r0 = *reinterpret_cast<const f4v*>(sI + li * SI + j) * tap(pc.g[PN]);
            f4v r1 = 0.f, r2 = 0.f;
#pragma unroll
            for (int k = 1; k <= PN; ++k) {
                const float g0 = tap(pc.g[PN + k]), g1 = tap(pc.xg[PN + k]), g2 = tap(pc.xxg[PN + k]);
                const f4v a = *reinterpret_cast<const f4v*>(sI + (li - k) * SI + j);
                const f4v b = *reinterpret_cast<const f4v*>(sI + (li + k) * SI + j);
                const f4v p = a + b;
                r0 = r0 + g0 * p;
                r1 = r1 + g1 * (b - a);
                r2 = r2 + g2 * p;
            }
            f4v* v = reinterpret_cast<f4v*>(sv + (i * SV + j) * 3);   // positions j..j+3, 3 floats each
            v[0] = f4v{r0.x, r1.x, r2.x, r0.y};
            v[1] = f4v{r1.y, r2.y, r0.z, r1.z};
            v[2] = f4v{r2.z, r0.w, r1.w, r2.w};
        }
    } else {
        // vertical part, float (oc_poly_exp: r = s*g0; t += g_k*(a+b) ...)
        for (int idx = tid; idx < PT_H * IW; idx += 256) {
            const int i = idx / IW, j = idx - i * IW;
            const int y = y0 + i, x = x0 - PN + j;
            if (!INT && (y >= h || x < 0 || x >= w)) continue;
            const int li = i + PN;
            float r0 = sI[li * SI + j] * pc.g[PN];
            float r1 = 0.f, r2 = 0.f;
#pragma unroll
            for (int k = 1; k <= PN; ++k) {
                const float g0 = pc.g[PN + k], g1 = pc.xg[PN + k], g2 = pc.xxg[PN + k];
                const int ya = INT ? li - k : max(y - k, 0) - (y0 - PN), yb = INT ? li + k : min(y + k, h - 1) - (y0 - PN);
                const float a = sI[ya * SI + j], b = sI[yb * SI + j];
                const float p = a + b;
                const float t0 = r0 + g0 * p;
                const float t1 = r1 + g1 * (b - a);
                const float t2 = r2 + g2 * p;
                r0 = t0;
                r1 = t1;
                r2 = t2;
            }
            float* v = sv + (i * SV + j) * 3;
            v[0] = r0;
            v[1] = r1;
            v[2] = r2;
        }
    }
    __syncthreads();
    // horizontal part (oc_poly_exp): float sub-expressions widened into double
    // accumulators, only tg * g / tg * xxg double products; replicated row ends
    for (int idx = tid; idx < PT_H * PT_W; idx += 256) {
        const int i = idx / PT_W, jx = idx - i * PT_W;
        const int y = y0 + i, x = x0 + jx;
        if (!INT && (y >= h || x >= w)) continue;
        const float* c = sv + (i * SV + jx + PN) * 3;
        const float gc = pc.g[PN];
        double b1 = (double)(c[0] * gc), b2 = 0, b3 = (double)(c[1] * gc), b4 = 0;
        double b5 = (double)(c[2] * gc), b6 = 0;
#pragma unroll
        for (int k = 1; k <= PN; ++k) {
            const float* P = INT ? c + 3 * k : sv + (i * SV + (min(x + k, w - 1) - (x0 - PN))) * 3;
            const float* M = INT ? c - 3 * k : sv + (i * SV + (max(x - k, 0) - (x0 - PN))) * 3;
            const float gk = pc.g[PN + k], xgk = pc.xg[PN + k];
            const double tg = (double)(P[0] + M[0]);
            // tg and the taps are floats: their double product has <= 48
            // significant bits, so it is exact and fma(tg, g, b) rounds exactly
            // as b + tg * g (one v_fma_f64 instead of v_mul_f64 + v_add_f64)
            b1 = __builtin_fma(tg, (double)gk, b1);
            b4 = __builtin_fma(tg, (double)pc.xxg[PN + k], b4);
            b2 += (double)((P[0] - M[0]) * xgk);
            b3 += (double)((P[1] + M[1]) * gk);
            b6 += (double)((P[1] - M[1]) * xgk);
            b5 += (double)((P[2] + M[2]) * gk);
        }
        float* d = R + 5u * (uint32_t)(y * w + x);
        d[1] = (float)(b2 * pc.ig11);
        d[0] = (float)(b3 * pc.ig11);
        d[3] = (float)(b1 * pc.ig03 + b4 * pc.ig33);
        d[2] = (float)(b1 * pc.ig03 + b5 * pc.ig33);
        d[4] = (float)(b6 * pc.ig55);
    }
}

}  // namespace

// ----------------------------------------------------------- level 0 --------
// Tile PT_W x PT_H of the full-resolution frame. Gray (of:71) over the tile +
// (PN+1) halo, the level-0 smoothing (GaussianBlur 3x3, sigma 0 -> taps
// (0.25, 0.5, 0.25), BORDER_REFLECT_101) over tile + PN halo, then the
// polynomial expansion. blockIdx.z = frame of the batch.
// LDS rows of the level-0 tile: the smoothed image and the vertical sums padded
// to whole 16-B groups of 4 columns (IW = 74 -> 76 at poly_n 5), and the gray
// kept as bytes, so that the blur and the vertical polynomial part run 4
// columns a thread on float4 vectors (round 6: VERDICT r5 #3b)
template <int PN> constexpr int f0_row() { return (PT_W + 2 * PN + 3) & ~3; }

template <int PN, bool INT, int FMT>
__device__ __forceinline__ void front0_tile(const OfGeom& g, const Level& lv, uint8_t* __restrict__ gray_out,
                                            const uint8_t* __restrict__ bgr, int pitch, size_t fstride,
                                            const SrcFmt& sf, long long a0, float* sgv, float* sI)
{
    // gray tile: rows y0-HG .., columns from x0-GX in whole 4-px quads (GX = 8 >= HG
    // keeps each quad's 12 BGR bytes 4-byte aligned: x0 % 64 == 0, pitch % 4 == 0)
    constexpr int HG = PN + 1, GX = 8, GW = PT_W + 2 * GX, GH = PT_H + 2 * HG, NQ = GW / 4;
    constexpr int IW = PT_W + 2 * PN, IH = PT_H + 2 * PN, SR = f0_row<PN>();
    static_assert(HG <= GX, "halo wider than the quad pad");
    static_assert(GX - PN - 1 >= 0, "the blur's left tap inside the gray row");
    // LDS: gray bytes (GH x GW) and the horizontal blur (GH x SR floats) share
    // sgv with the vertical sums written after the blur (poly_tile)
    uint8_t* sgb = reinterpret_cast<uint8_t*>(sgv);
    float* sh = sgv + (GH * GW + 15) / 16 * 4;
    const int tid = threadIdx.x, t = blockIdx.z;
    const int W = g.W, H = g.H;
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
    const uint8_t* f = bgr + (size_t)t * fstride;
    uint8_t* go = gray_out + (size_t)t * g.GP * H;
    for (int idx = tid; idx < GH * NQ; idx += 256) {
        const int i = idx / NQ, q = idx - i * NQ;
        const int y = y0 - HG + i, px = x0 - GX + 4 * q;
        // the row's last quad may stick out past W: its bytes lie inside the row
        // (pitch >= 3 * roundup(W, 4)), its gray values land in the gray rows'
        // padding (GP) and in LDS columns the clamped / reflected taps never read
        if (!INT && (y < 0 || y >= H || px < 0 || px >= W)) continue;
        // of:71 BGR2GRAY of 4 px: 12 packed BGR bytes, or a 4:2:0 quad through cvtColor YUV2BGR
        uint32_t v0, v1, v2;
        load_quad<FMT>(f + (size_t)y * pitch + (FMT == DVC_FMT_BGR ? 3 * px : px), f + chroma_off<FMT>(sf, y, px),
                       sf.voff - sf.uoff, v0, v1, v2);
        const uint32_t gq = quad_gray<FMT>(v0, v1, v2);
        *reinterpret_cast<uint32_t*>(sgb + i * GW + 4 * q) = gq;
        if (i >= HG && i < HG + PT_H && px >= x0 && px < x0 + PT_W)
            *reinterpret_cast<uint32_t*>(go + (size_t)y * g.GP + px) = gq;
    }
    __syncthreads();
    // I = blur3(gray) (oc_blur_f32): the horizontal pass of every gray row the
    // vertical pass reads, then the vertical pass — the values the per-pixel
    // form computed (acc = kc * c; acc += ks * (l + r), per row, then the same
    // over the three rows), each horizontal sum once
    const float kc = lv.kf[1], ks = lv.kf[2];
    if constexpr (INT) {
        constexpr int NG = SR / 4;
        for (int it = tid; it < GH * NG; it += 256) {   // row r = gray row y0 - HG + r, columns x0 - PN + 4 m ..
            const int r = it / NG, m = it - r * NG;
            // px x0 - PN + 4m - 1 .. + 4 are bytes O + 4m .. + 5 of the row, O = GX - PN - 1
            // (2 at poly_n 5, 0 at 7): two aligned dwords hold them
            constexpr int O = GX - PN - 1;
            const uint32_t* wp = reinterpret_cast<const uint32_t*>(sgb + r * GW + 4 * m);
            const uint32_t d0 = wp[0], d1 = wp[1];
            auto px = [&](auto kc_) {
                constexpr int bi = O + decltype(kc_)::value;
                return (float)(((bi < 4 ? d0 : d1) >> (8 * (bi & 3))) & 255u);
            };
            using std::integral_constant;
            const f4v lft = f4v{px(integral_constant<int, 0>{}), px(integral_constant<int, 1>{}),
                                px(integral_constant<int, 2>{}), px(integral_constant<int, 3>{})};
            const f4v ctr = f4v{lft.y, lft.z, lft.w, px(integral_constant<int, 4>{})};
            const f4v rgt = f4v{lft.z, lft.w, ctr.w, px(integral_constant<int, 5>{})};
            f4v acc = kc * ctr;
            acc = acc + ks * (lft + rgt);
            *reinterpret_cast<f4v*>(sh + r * SR + 4 * m) = acc;
        }
        __syncthreads();
        for (int it = tid; it < IH * NG; it += 256) {   // image row i = y0 - PN + i: gray rows i, i+1, i+2 (HG = PN + 1)
            const int i = it / NG, m = it - i * NG;
            const f4v h0 = *reinterpret_cast<const f4v*>(sh + i * SR + 4 * m);
            const f4v h1 = *reinterpret_cast<const f4v*>(sh + (i + 1) * SR + 4 * m);
            const f4v h2 = *reinterpret_cast<const f4v*>(sh + (i + 2) * SR + 4 * m);
            f4v acc = kc * h1;
            acc = acc + ks * (h0 + h2);
            *reinterpret_cast<f4v*>(sI + i * SR + 4 * m) = acc;
        }
    } else {
        for (int idx = tid; idx < GH * IW; idx += 256) {
            const int r = idx / IW, j = idx - r * IW;
            const int yg = y0 - HG + r, x = x0 - PN + j;
            if (yg < 0 || yg >= H || x < 0 || x >= W) continue;
            const uint8_t* s = sgb + r * GW - (x0 - GX);
            float acc = kc * (float)s[x];
            acc += ks * ((float)s[reflect1(x - 1, W)] + (float)s[reflect1(x + 1, W)]);
            sh[r * SR + j] = acc;
        }
        __syncthreads();
        for (int idx = tid; idx < IH * IW; idx += 256) {
            const int i = idx / IW, j = idx - i * IW;
            const int y = y0 - PN + i, x = x0 - PN + j;
            if (y < 0 || y >= H || x < 0 || x >= W) continue;
            const float* c = sh + j - (y0 - HG) * SR;
            float acc = kc * c[y * SR];
            acc += ks * (c[reflect1(y - 1, H) * SR] + c[reflect1(y + 1, H) * SR]);
            sI[i * SR + j] = acc;
        }
    }
    __syncthreads();
    float* R = lv.R + (size_t)ring(a0 + t, g.RS) * W * H * 5;
    poly_tile<PN, INT, SR, SR, INT>(sI, sgv, g.pc, x0, y0, W, H, R);
}

// Interior tiles (the tile with its GX-px quad pad and HG-row halo inside the
// frame) take the unclamped, vectorised form: the same arithmetic on the same values.
template <int PN, int FMT>
__global__ void __launch_bounds__(256) k_of_front0(OfGeom g, Level lv, uint8_t* __restrict__ gray_out,
                                                   const uint8_t* __restrict__ bgr, int pitch, size_t fstride,
                                                   SrcFmt sf, long long a0)
{
    constexpr int HG = PN + 1, GX = 8, GW = PT_W + 2 * GX, GH = PT_H + 2 * HG;
    constexpr int IH = PT_H + 2 * PN, SR = f0_row<PN>();
    // the gray bytes + the horizontal blur (read by the vertical blur) and the
    // vertical sums (written after the blur's barrier) share one array
    constexpr int A = (GH * GW + 15) / 16 * 4 + GH * SR, B = PT_H * SR * 3;
    __shared__ __attribute__((aligned(16))) float sgv[A > B ? A : B];
    __shared__ __attribute__((aligned(16))) float sI[IH * SR];
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
    const bool interior = x0 >= GX && x0 + PT_W + GX <= g.W && y0 >= HG && y0 + PT_H + HG <= g.H;   // uniform
    if (interior) front0_tile<PN, true, FMT>(g, lv, gray_out, bgr, pitch, fstride, sf, a0, sgv, sI);
    else front0_tile<PN, false, FMT>(g, lv, gray_out, bgr, pitch, fstride, sf, a0, sgv, sI);
}

// ----------------------------------------------------------- level k > 0 ----
// Horizontal smoothing pass (oc_blur_f32, first loop) of the full-resolution
// gray at the 2w source columns the resize reads: tmpc[y][2dx] at xt[dx].s0,
// tmpc[y][2dx+1] at xt[dx].s1. One workgroup per PH_ROWS rows of a frame (a
// workgroup per row spent more on dispatch than on its work), each row staged
// in LDS (dynamic, 2 x GP bytes: whole dwords, double-buffered so row y+1's
// loads fly while row y is blurred).
constexpr int PH_ROWS = 4;
constexpr int PH_J = 8;   // column slots per thread (n2 <= 256 * PH_J: the taps' columns kept in registers)
// F32: rows staged as floats, double-buffered (8 x GP bytes of LDS); wide
// frames (8 x GP > PH_F32_LDS) stage each row as its GP bytes, single-buffered,
// and convert at the tap (the same float values: (float) of the byte).
constexpr size_t PH_F32_LDS = 64 * 1024;
template <bool F32>
__global__ void __launch_bounds__(256) k_pyr_h(OfGeom g, Level lv, const uint8_t* __restrict__ gray)
{
    // the row as floats in LDS (each tap one ds_read_b32, no byte convert), the
    // thread's source columns loaded once for the workgroup's rows
    extern __shared__ float srowf[];
    const int t = blockIdx.y, W = g.W, H = g.H, y0 = blockIdx.x * PH_ROWS, ye = min(y0 + PH_ROWS, H);
    const int nq = g.GP / 4, r = lv.r, n2 = 2 * lv.w;
    const uint8_t* fr = gray + (size_t)t * g.GP * H;
    int col[PH_J];
#pragma unroll
    for (int q = 0; q < PH_J; ++q) {
        const int j = threadIdx.x + 256 * q;
        col[q] = 0;
        if (j < n2) {
            const LinTap tp = lv.xt[j >> 1];
            col[q] = (j & 1) ? tp.s1 : tp.s0;
        }
    }
    for (int y = y0; y < ye; ++y) {
        float* buf = srowf + ((y - y0) & 1) * g.GP;
        uint32_t* bufb = reinterpret_cast<uint32_t*>(srowf);
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(fr + (size_t)y * g.GP);
        for (int i = threadIdx.x; i < nq; i += 256) {
            const uint32_t v = s32[i];
            if constexpr (F32)
                *reinterpret_cast<float4*>(buf + 4 * i) =
                    make_float4((float)(v & 255), (float)((v >> 8) & 255), (float)((v >> 16) & 255), (float)(v >> 24));
            else
                bufb[i] = v;
        }
        __syncthreads();   // (F32: also the buffer's previous row, two rows back, is consumed)
        auto px = [&](int c) -> float {
            if constexpr (F32) return buf[c];
            else return (float)reinterpret_cast<const uint8_t*>(bufb)[c];
        };
        float* out = lv.tmpc + (size_t)t * H * n2 + (size_t)y * n2;
#pragma unroll
        for (int q = 0; q < PH_J; ++q) {
            const int j = threadIdx.x + 256 * q;
            if (j >= n2) break;
            const int c = col[q];
            float acc = lv.kf[r] * px(c);
            if (c >= r && c + r < W)   // taps inside the row: reflect101 is the identity
                for (int i = 1; i <= r; ++i) acc += lv.kf[r + i] * (px(c - i) + px(c + i));
            else
                for (int i = 1; i <= r; ++i)
                    acc += lv.kf[r + i] * (px(reflect101(c - i, W)) + px(reflect101(c + i, W)));
            out[j] = acc;
        }
        for (int j = threadIdx.x + 256 * PH_J; j < n2; j += 256) {   // wide levels: taps per row
            const LinTap tp = lv.xt[j >> 1];
            const int c = (j & 1) ? tp.s1 : tp.s0;
            float acc = lv.kf[r] * px(c);
            if (c >= r && c + r < W)
                for (int i = 1; i <= r; ++i) acc += lv.kf[r + i] * (px(c - i) + px(c + i));
            else
                for (int i = 1; i <= r; ++i)
                    acc += lv.kf[r + i] * (px(reflect101(c - i, W)) + px(reflect101(c + i, W)));
            out[j] = acc;
        }
        if constexpr (!F32) __syncthreads();   // single buffer: every tap read before the next row lands
    }
}

// Vertical smoothing pass (oc_blur_f32, second loop) at the 2h source rows the
// resize reads: vtmp[2dy][j] at row yt[dy].s0, vtmp[2dy+1][j] at yt[dy].s1, for
// every column slot j of tmpc — each blurred value the resize needs, once. A
// workgroup = 256 column slots x PV_ROWS output rows of a frame. The two rows
// of a level row (s1 = s0 + 1 inside the image) walk their taps together: each
// step loads the two new outer values and reuses the previous step's (2 loads
// a tap pair instead of 4; the same sums in the same order).
constexpr int PV_ROWS = 8;
__global__ void __launch_bounds__(256) k_pyr_v(OfGeom g, Level lv)
{
    const int j = blockIdx.x * 256 + threadIdx.x, t = blockIdx.z;
    const int H = g.H, n2 = 2 * lv.w, r = lv.r, yy0 = blockIdx.y * PV_ROWS, yye = min(yy0 + PV_ROWS, 2 * lv.h);
    if (j >= n2) return;
    const float* T = lv.tmpc + (size_t)t * H * n2 + j;
    float* V = lv.vtmp + (size_t)t * 2 * lv.h * n2 + j;
    for (int yy = yy0; yy < yye; ++yy) {
        const LinTap ty = lv.yt[yy >> 1];
        if (!(yy & 1) && yy + 1 < yye && ty.s1 == ty.s0 + 1 && ty.s0 >= r && ty.s1 + r < H) {
            const float* C = T + (uint32_t)(ty.s0 * n2);
            float lo = C[0], hi = C[n2];   // row s0 - (i-1), row s1 + (i-1)
            float a0 = lv.kf[r] * lo, a1 = lv.kf[r] * hi;
            for (int i = 1; i <= r; ++i) {
                const float lo_i = C[-(int)(i * n2)], hi_i = C[(i + 1) * n2];
                a0 += lv.kf[r + i] * (lo_i + hi);   // T[s0 - i] + T[s0 + i]
                a1 += lv.kf[r + i] * (lo + hi_i);   // T[s1 - i] + T[s1 + i]
                lo = lo_i;
                hi = hi_i;
            }
            V[(size_t)yy * n2] = a0;
            V[(size_t)(yy + 1) * n2] = a1;
            ++yy;
            continue;
        }
        const int row = (yy & 1) ? ty.s1 : ty.s0;
        float acc = lv.kf[r] * T[(size_t)row * n2];
        if (row >= r && row + r < H) {
            const float* C = T + (uint32_t)(row * n2);
            for (int i = 1; i <= r; ++i) acc += lv.kf[r + i] * (C[-(int)(i * n2)] + C[i * n2]);
        } else {
            for (int i = 1; i <= r; ++i)
                acc += lv.kf[r + i] * (T[(size_t)reflect101(row - i, H) * n2] + T[(size_t)reflect101(row + i, H) * n2]);
        }
        V[(size_t)yy * n2] = acc;
    }
}

// The INTER_LINEAR combination (oc_resize_linear_f32) over tile + PN halo from
// vtmp, then the polynomial expansion of the level image. INT: tile + halo
// inside the level image (no skipped positions, no clamped taps).
template <int PN, bool INT>
__device__ __forceinline__ void pyr_poly_tile(const OfGeom& g, const Level& lv, long long a0, float* sI, float* sv)
{
    constexpr int IW = PT_W + 2 * PN, IH = PT_H + 2 * PN, SR = f0_row<PN>();
    const int tid = threadIdx.x, t = blockIdx.z;
    const int w = lv.w, h = lv.h, n2 = 2 * w;
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
    const float* V = lv.vtmp + (size_t)t * 2 * h * n2;
    for (int idx = tid; idx < IH * IW; idx += 256) {
        const int i = idx / IW, j = idx - i * IW;
        const int y = y0 - PN + i, x = x0 - PN + j;
        if (!INT && (y < 0 || y >= h || x < 0 || x >= w)) continue;
        const LinTap ty = lv.yt[y], tx = lv.xt[x];
        const float* v0 = V + (uint32_t)(2 * y * n2 + 2 * x);
        const float* v1 = v0 + n2;
        const float t0 = v0[0] * tx.w0 + v0[1] * tx.w1;
        const float t1 = v1[0] * tx.w0 + v1[1] * tx.w1;
        sI[i * SR + j] = t0 * ty.w0 + t1 * ty.w1;
    }
    __syncthreads();
    float* R = lv.R + (size_t)ring(a0 + t, g.RS) * w * h * 5;
    poly_tile<PN, INT, SR, SR, INT>(sI, sv, g.pc, x0, y0, w, h, R);   // rows padded to 16 B: the vector form
}

template <int PN>
__global__ void __launch_bounds__(256) k_pyr_poly(OfGeom g, Level lv, long long a0)
{
    constexpr int IH = PT_H + 2 * PN, SR = f0_row<PN>();
    __shared__ __attribute__((aligned(16))) float sI[IH * SR];
    __shared__ __attribute__((aligned(16))) float sv[PT_H * SR * 3];
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
    if (x0 >= PN && x0 + PT_W + PN <= lv.w && y0 >= PN && y0 + PT_H + PN <= lv.h)
        pyr_poly_tile<PN, true>(g, lv, a0, sI, sv);
    else
        pyr_poly_tile<PN, false>(g, lv, a0, sI, sv);
}

// -------------------------------------------------------------------- flow --
// One Farneback iteration of level `lv` for every frame of the batch
// (blockIdx.z). Tile FL_W x FL_H; LDS holds M (5 floats) over the tile + m halo
// (replicated borders), then — aliased over it — the vertical box sums.
//   src_mode 0: flow_in = 0 (coarsest level, first iteration)
//            1: flow_in = INTER_LINEAR upsample of the coarser level's final
//               flow, times (float)(1/pyr_scale)
//            2: flow_in = this level's previous iteration
//   last:    the finest level's last iteration: |flow| > thr bits -> mring
struct FlowArgs {
    OfGeom g;
    Level lv;
    const float* src;    // flow_in (mode 1: coarser level's, mode 2: this level's), n frames
    int sw, sh;          // dims of src (mode 1)
    float* dst;          // flow out, n frames (nullable when last)
    long long a0;
    int src_mode, last;
    uint64_t* mring;
    float* dbg_flow;     // last && nullable: frame n-1's flow
    int n;
};

// One tile of k_flow. MB > 0: box radius m known at compile time (the
// reference's winsize 9 -> 4): constant tile geometry, the vertical sums one
// thread per (column, channel) with the column's M converted to double once in
// registers. INT: an interior tile — tile + box halo inside the image and at
// least 5 px from its edges — so no coordinate is clamped, no position skipped
// and no border weight applied (the same arithmetic on the same values as the
// general form). MB = 0: any m, clamped everywhere, one thread per (row,
// column) re-reading M per tap.
template <int MB, bool INT>
__device__ __forceinline__ void flow_tile(const FlowArgs& A, double* lds_d)
{
    float* sM = reinterpret_cast<float*>(lds_d);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = blockIdx.z;
    const OfGeom& g = A.g;
    const int w = A.lv.w, h = A.lv.h;
    const int m = MB > 0 ? MB : g.m;
    const int RW = FL_W + 2 * m, RH = FL_H + 2 * m;
    const int x0 = blockIdx.x * FL_W, y0 = blockIdx.y * FL_H;
    const size_t lvpx = (size_t)w * h;
    const long long a = A.a0 + t;
    const float* __restrict__ R0 = A.lv.R + (size_t)ring(a - 1, g.RS) * lvpx * 5;
    const float* __restrict__ R1 = A.lv.R + (size_t)ring(a, g.RS) * lvpx * 5;
    const float* src = A.src ? A.src + (size_t)t * (A.src_mode == 1 ? (size_t)A.sw * A.sh : lvpx) * 2 : nullptr;

    // ---- FarnebackUpdateMatrices over tile + halo (oc_update_matrices).
    // Positions in groups of MQ per thread: every address is clamped into the
    // image and every load unconditional (results of out-of-image positions
    // are discarded), so a group's flow / R0 loads and then its bilinear R1
    // gathers are all in flight together instead of one dependent round trip
    // pair per position. Pixel offsets are 32-bit (a level plane < 2^31 floats).
    constexpr int MQ = 2;
    const int npos = RH * RW;
    for (int q0 = tid; q0 < npos; q0 += 256 * MQ) {
        int idx[MQ], xs[MQ], ys[MQ];
        bool ok[MQ];
        float dxv[MQ], dyv[MQ], r0v[MQ][5];
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            idx[u] = q0 + 256 * u;
            const int i = idx[u] / RW, j = idx[u] - i * RW;
            const int y = y0 - m + i, x = x0 - m + j;
            if constexpr (INT) {
                ok[u] = idx[u] < npos;
                ys[u] = ok[u] ? y : y0;
                xs[u] = x;
            } else {
                ok[u] = idx[u] < npos && y >= 0 && y < h && x >= 0 && x < w;
                ys[u] = min(max(y, 0), h - 1);
                xs[u] = min(max(x, 0), w - 1);
            }
            const uint32_t pix = (uint32_t)(ys[u] * w + xs[u]);
            dxv[u] = 0.f;
            dyv[u] = 0.f;
            if (A.src_mode == 2) {   // uniform
                const float2 f = *reinterpret_cast<const float2*>(src + 2u * pix);
                dxv[u] = f.x;
                dyv[u] = f.y;
            } else if (A.src_mode == 1) {
                const LinTap ty = A.lv.uy[ys[u]], tx = A.lv.ux[xs[u]];
                const float* ra = src + (uint32_t)(ty.s0 * A.sw) * 2u;
                const float* rb = src + (uint32_t)(ty.s1 * A.sw) * 2u;
                float v[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float t0 = ra[tx.s0 * 2 + c] * tx.w0 + ra[tx.s1 * 2 + c] * tx.w1;
                    const float t1 = rb[tx.s0 * 2 + c] * tx.w0 + rb[tx.s1 * 2 + c] * tx.w1;
                    v[c] = t0 * ty.w0 + t1 * ty.w1;
                }
                dxv[u] = v[0] * g.up;
                dyv[u] = v[1] * g.up;
            }
            const float* r0 = R0 + 5u * pix;
            ld5(r0, r0v[u]);
        }
        float pq[MQ][20];
        float fxv[MQ], fyv[MQ];
        bool inb[MQ];
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            float fx = (float)xs[u] + dxv[u], fy = (float)ys[u] + dyv[u];
            const int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
            fxv[u] = fx - (float)x1;
            fyv[u] = fy - (float)y1;
            inb[u] = (unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1);
            const int x1c = min(max(x1, 0), max(w - 2, 0)), y1c = min(max(y1, 0), max(h - 2, 0));
            const float* p = R1 + 5u * (uint32_t)(y1c * w + x1c);
            const float* q = p + 5u * (uint32_t)w;
            ld10(p, pq[u]);
            ld10(q, pq[u] + 10);
        }
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            if (!ok[u]) continue;
            const int x = xs[u], y = ys[u];
            const float dx = dxv[u], dy = dyv[u], fx = fxv[u], fy = fyv[u];
            const float* r0 = r0v[u];
            const float* p = pq[u];
            const float* q = pq[u] + 10;
            // channel pairs (r2, r3), (r4, r5) as packed f32x2 (v_pk_mul/add_f32,
            // each lane the same mul-then-add sequence as the scalar form), r6 scalar
            f32x2 R23, R45;
            float r6;
            const f32x2 R0_01 = {r0[0], r0[1]}, R0_23 = {r0[2], r0[3]};
            if (inb[u]) {
                const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
                const f32x2 A00 = a00, A01 = a01, A10 = a10, A11 = a11;
                const f32x2 P01 = {p[0], p[1]}, P23 = {p[2], p[3]}, P56 = {p[5], p[6]}, P78 = {p[7], p[8]};
                const f32x2 Q01 = {q[0], q[1]}, Q23 = {q[2], q[3]}, Q56 = {q[5], q[6]}, Q78 = {q[7], q[8]};
                R23 = A00 * P01 + A01 * P56 + A10 * Q01 + A11 * Q56;
                R45 = A00 * P23 + A01 * P78 + A10 * Q23 + A11 * Q78;
                r6 = a00 * p[4] + a01 * p[9] + a10 * q[4] + a11 * q[9];
                R45 = (R0_23 + R45) * (f32x2)0.5f;
                r6 = (r0[4] + r6) * 0.25f;
            } else {
                R23 = (f32x2)0.f;
                R45 = R0_23;
                r6 = r0[4] * 0.5f;
            }
            R23 = (R0_01 - R23) * (f32x2)0.5f;
            // r2 += r4 dy + r6 dx;  r3 += r6 dy + r5 dx
            R23 = R23 + ((f32x2){R45.x, r6} * (f32x2)dy + (f32x2){r6, R45.y} * (f32x2)dx);
            if constexpr (!INT) {
                if ((unsigned)(x - 5) >= (unsigned)(w - 10) || (unsigned)(y - 5) >= (unsigned)(h - 10)) {
                    const float scale = (x < 5 ? border_w(x) : 1.f) * (x >= w - 5 ? border_w(w - x - 1) : 1.f) *
                                        (y < 5 ? border_w(y) : 1.f) * (y >= h - 5 ? border_w(h - y - 1) : 1.f);
                    R23 = R23 * (f32x2)scale;
                    R45 = R45 * (f32x2)scale;
                    r6 *= scale;
                }
            }
            float* M = sM + (size_t)idx[u] * 5;
            const f32x2 G = R45 * R45 + (f32x2)(r6 * r6);                                   // (M0, M2)
            const f32x2 Hh = (f32x2){R45.x, r6} * (f32x2)R23.x + (f32x2){r6, R45.y} * (f32x2)R23.y;   // (M3, M4)
            M[0] = G.x;
            M[1] = (R45.x + R45.y) * r6;
            M[2] = G.y;
            M[3] = Hh.x;
            M[4] = Hh.y;
        }
    }
    __syncthreads();

    // ---- vertical box sums (double, rows in order) into sV, aliased over sM:
    // FL_H x RW x 5 doubles
    double* sV = lds_d;
    if constexpr (MB > 0) {
        constexpr int CR = FL_H + 2 * MB;   // M rows of a column
        const int j = tid / 5, c = tid - 5 * j;
        const int x = x0 - m + j;
        const bool colv = INT ? j < RW : (j < RW && x >= 0 && x < w);
        double col[CR];
#pragma unroll
        for (int r = 0; r < CR; ++r) {   // rows clamped into the image (replicated border)
            const int yy = INT ? r : min(max(y0 - m + r, 0), h - 1) - (y0 - m);
            col[r] = colv ? (double)sM[(yy * RW + j) * 5 + c] : 0.0;
        }
        __syncthreads();
        if (colv) {
#pragma unroll
            for (int i = 0; i < FL_H; ++i) {
                double sum = 0.0;
#pragma unroll
                for (int jj = 0; jj <= 2 * MB; ++jj) sum += col[i + jj];
                sV[(i * RW + j) * 5 + c] = sum;
            }
        }
        __syncthreads();
    } else {
        constexpr int VMAX = (FL_H * (FL_W + 2 * OF_MAX_BOX_M) + 255) / 256;
        double vs[VMAX][5];
        const int nv = FL_H * RW;
#pragma unroll
        for (int q = 0; q < VMAX; ++q) {
            const int idx = tid + 256 * q;
            if (idx >= nv) break;
            const int i = idx / RW, j = idx - i * RW;
            const int y = y0 + i, x = x0 - m + j;
#pragma unroll
            for (int c = 0; c < 5; ++c) vs[q][c] = 0.0;
            if (y >= h || x < 0 || x >= w) continue;
            double s[5] = {0, 0, 0, 0, 0};
            for (int jj = -m; jj <= m; ++jj) {
                const float* M = sM + (size_t)((min(max(y + jj, 0), h - 1) - (y0 - m)) * RW + j) * 5;
#pragma unroll
                for (int c = 0; c < 5; ++c) s[c] += (double)M[c];
            }
#pragma unroll
            for (int c = 0; c < 5; ++c) vs[q][c] = s[c];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < VMAX; ++q) {
            const int idx = tid + 256 * q;
            if (idx >= nv) break;
#pragma unroll
            for (int c = 0; c < 5; ++c) sV[(size_t)idx * 5 + c] = vs[q][c];
        }
        __syncthreads();
    }

    // ---- horizontal box sums, flow = G^-1 h (oc_update_flow_box); a wave covers
    // two 32-px rows (lanes 0-31 row i, 32-63 row i+1)
    float* dst = A.dst ? A.dst + (size_t)t * lvpx * 2 : nullptr;
    for (int i2 = wave; i2 < FL_H / 2; i2 += 4) {
        const int i = 2 * i2 + (lane >> 5);
        const int y = y0 + i, x = x0 + (lane & 31);
        const bool act = INT || (y < h && x < w);
        float fxo = 0.f, fyo = 0.f;
        if (act) {
            double hs[5] = {0, 0, 0, 0, 0};
            if constexpr (MB > 0) {
#pragma unroll
                for (int ii = -MB; ii <= MB; ++ii) {
                    const int xx = INT ? (lane & 31) + MB + ii : min(max(x + ii, 0), w - 1) - (x0 - m);
                    const double* v = sV + (i * RW + xx) * 5;
#pragma unroll
                    for (int c = 0; c < 5; ++c) hs[c] += v[c];
                }
            } else {
                for (int ii = -m; ii <= m; ++ii) {
                    const double* v = sV + (size_t)(i * RW + (min(max(x + ii, 0), w - 1) - (x0 - m))) * 5;
#pragma unroll
                    for (int c = 0; c < 5; ++c) hs[c] += v[c];
                }
            }
            const double g11 = hs[0] * g.box_scale, g12 = hs[1] * g.box_scale, g22 = hs[2] * g.box_scale;
            const double h1 = hs[3] * g.box_scale, h2 = hs[4] * g.box_scale;
            const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
            fxo = (float)((g11 * h2 - g12 * h1) * idet);
            fyo = (float)((g22 * h1 - g12 * h2) * idet);
        }
        if (!A.last) {
            if (act) *reinterpret_cast<float2*>(dst + 2u * (uint32_t)(y * w + x)) = make_float2(fxo, fyo);
        } else {
            // of:82-83: cartToPolar magnitude (float) > flow_threshold
            const float mag = sqrtf(fxo * fxo + fyo * fyo);
            const bool bit = act && mag > g.flow_thr;
            const unsigned long long word = __ballot(bit);
            uint32_t* mr = reinterpret_cast<uint32_t*>(A.mring + (size_t)ring(a, g.RB) * h * g.WW);
            const int half = (x0 >> 5) & 1;
            if ((lane & 31) == 0 && y < h) {
                mr[((size_t)y * g.WW + (x0 >> 6)) * 2 + half] = (uint32_t)(word >> (lane & 32));
                if (half == 0 && x0 + 32 >= w) mr[((size_t)y * g.WW + (x0 >> 6)) * 2 + 1] = 0u;   // no tile owns it
            }
            if (A.dbg_flow && t == A.n - 1 && act)
                *reinterpret_cast<float2*>(A.dbg_flow + ((size_t)y * w + x) * 2) = make_float2(fxo, fyo);
        }
    }
}

template <int MB>
__global__ void __launch_bounds__(256) k_flow(FlowArgs A)
{
    extern __shared__ __attribute__((aligned(16))) double lds_d[];
    if constexpr (MB > 0) {
        const int x0 = blockIdx.x * FL_W, y0 = blockIdx.y * FL_H;
        const bool interior = x0 - MB >= 5 && x0 + FL_W + MB <= A.lv.w - 5 && y0 - MB >= 5 &&
                              y0 + FL_H + MB <= A.lv.h - 5;   // uniform
        if (interior) flow_tile<MB, true>(A, lds_d);
        else flow_tile<MB, false>(A, lds_d);
    } else {
        flow_tile<0, false>(A, lds_d);
    }
}

// ------------------------------------------------------ flow: sliding sums --
// FarnebackUpdateFlow_Blur with OpenCV's own accumulation order
// (optflowgf.cpp; oracle/of_oracle.c oc_update_flow_box_sliding): per column a
// vertical running double sum fed with float row differences, per row a
// horizontal running double sum — recurrences whose rounding is part of the
// result, so they are walked in order. A work item is one strip of SC_W
// columns of one frame: its workgroup walks the level's rows in blocks of SC_R
//   1. FarnebackUpdateMatrices of the block's new M rows over the strip's
//      columns + the box halo (m + 1 left, m right), into an LDS ring of rows;
//   2. the vertical recurrence of every (column, channel) of the strip for the
//      block's rows, the state in registers across blocks, the sums in LDS;
//   3. the horizontal recurrence of every (row, channel) across the strip's
//      columns, started from the state the strip to its left published for
//      that row (strip 0: OpenCV's (m + 2) vsum[0] + vsum[1..m-1] start);
//      the state after the strip's last column is published for the right
//      neighbour (payload, release fence, flag — one wave);
//   4. flow = G^-1 h per pixel (or |flow| > thr bits on the finest level's
//      last iteration).
// Strips of a frame form a wavefront: strip s waits, block by block, for
// strip s-1's published state. Frames are dealt to SCAN_Q queues, frame t to
// queue t % SCAN_Q, whose items are dequeued in (frame, strip) order from the
// queue's counter; workgroup b starts at queue b % SCAN_Q — blocks b, b + 8, ..
// share an XCD (MI355X_MICROARCH.md § Workgroup dispatch), so a frame's strips
// and their hand-offs tend to stay in one XCD's L2 — and moves on to the next
// queues when its own is drained. The strip an item waits on was taken
// earlier from the same queue by a running workgroup: no residency or
// placement assumption, no deadlock. A wait that ever exceeds ~1 s sets
// `abort` (reported by the host as an error) instead of hanging.
struct ScanArgs {
    FlowArgs f;
    int S;                       // strips across the level
    int NB;                      // row blocks down the level
    uint32_t* gpub;              // n x S x NB x 64 slots of 16 B: {tag, lo, hi, tag} per (row, channel)
    unsigned int* next;          // SCAN_Q work-item counters, zeroed before the launch
    unsigned int* abort;         // a wait timed out (never in a correct run)
    unsigned int epoch;          // launch number >= 1: the tag of this launch's published slots
};

constexpr int SCAN_Q = 8;   // work queues (XCD groups of workgroups)

// strip width SW (columns) and rows per block RB; LDS: the M ring (RB + 2m + 1
// rows of SW + 2m + 1 columns x 5 floats) and the block's vertical sums (RB
// rows of SW + 2m + 1 columns x 5 doubles, rows padded to 5 mod 32 doubles so
// the horizontal chains' lanes (row i, channel c) fall on distinct LDS bank
// pairs, at most 2-way); the chains overwrite the consumed vertical sums with
// the horizontal ones in place
// The M ring holds RB + 2m + 1 rows, rounded up to a multiple of RB: a block's
// rows then start at one of RING / RB ring phases, and the vertical sums of an
// interior block (m == the variant's MM) read their ring rows at compile-time
// offsets of that phase (scan_vsum_rows) — no per-row slot arithmetic.
__host__ __device__ constexpr int scan_ring(int rb, int m) { return (rb + 2 * m + 1 + rb - 1) / rb * rb; }
__host__ __device__ constexpr int scan_nc(int sw, int m) { return sw + 2 * m + 1; }
__host__ __device__ constexpr int scan_vs(int sw, int m) { return scan_nc(sw, m) * 5 + ((5 - scan_nc(sw, m) * 5) % 32 + 32) % 32; }
inline size_t scan_lds_bytes(int sw, int rb, int m)
{
    return (size_t)scan_ring(rb, m) * scan_nc(sw, m) * 5 * 4 + (size_t)rb * scan_vs(sw, m) * 8;
}

// M of FarnebackUpdateMatrices (oc_update_matrices) at MQ positions (x, y)
// inside the level, in three stages so a caller can overlap each stage's
// loads with other work: (1) the flow loads, (2) the R0 loads and the
// displaced bilinear R1 loads (their address needs the flow), (3) the
// arithmetic and the LDS store of the 5 floats at off[u] of the M ring.
template <int MQ>
struct MatPos {
    int xs[MQ], ys[MQ], off[MQ];
    bool ok[MQ];
    float dx[MQ], dy[MQ], r0[MQ][5];   // stage 1
    float pq[MQ][20];                  // stage 2 (the bilinear fractions and the
                                       // in-bounds test are recomputed in stage 3
                                       // rather than held across the step)
};

// the displaced position (x + dx, y + dy) of FarnebackUpdateMatrices: its
// integer corner and fractions, and whether the 2x2 neighbourhood is inside
__device__ __forceinline__ bool mat_corner(int x, int y, float dx, float dy, int w, int h, int& x1, int& y1,
                                           float& fx, float& fy)
{
    const float px = (float)x + dx, py = (float)y + dy;
    x1 = (int)floorf(px);
    y1 = (int)floorf(py);
    fx = px - (float)x1;
    fy = py - (float)y1;
    return (unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1);
}

// stage 1: the flow loads (src_mode 2; the scan kernel's source flow is never
// the coarser level's: k_flow_up upsamples it to a flow buffer first)
template <int MQ, int SMODE>
__device__ __forceinline__ void mat_stage1(const FlowArgs& A, const float* src, MatPos<MQ>& P)
{
    const int w = A.lv.w;
#pragma unroll
    for (int u = 0; u < MQ; ++u) {
        const uint32_t pix = (uint32_t)(P.ys[u] * w + P.xs[u]);
        P.dx[u] = 0.f;
        P.dy[u] = 0.f;
        if constexpr (SMODE == 2) {
            const float2 f = *reinterpret_cast<const float2*>(src + 2u * pix);
            P.dx[u] = f.x;
            P.dy[u] = f.y;
        }
    }
}

template <int MQ, int U0 = 0, int U1 = MQ>
__device__ __forceinline__ void mat_stage2(const FlowArgs& A, const float* __restrict__ R0,
                                           const float* __restrict__ R1, MatPos<MQ>& P)
{
    const int w = A.lv.w, h = A.lv.h;
#pragma unroll
    for (int u = U0; u < U1; ++u) {
        ld5(R0 + 5u * (uint32_t)(P.ys[u] * w + P.xs[u]), P.r0[u]);   // (independent of the flow)
        int x1, y1;
        float fx, fy;
        (void)mat_corner(P.xs[u], P.ys[u], P.dx[u], P.dy[u], w, h, x1, y1, fx, fy);
        const int x1c = min(max(x1, 0), max(w - 2, 0)), y1c = min(max(y1, 0), max(h - 2, 0));
        const float* p = R1 + 5u * (uint32_t)(y1c * w + x1c);
        const float* q = p + 5u * (uint32_t)w;
        ld10(p, P.pq[u]);
        ld10(q, P.pq[u] + 10);
    }
}

// Branch-free up to the LDS store: every position's arithmetic runs (positions
// past the block are valid clamped ones), the out-of-range bilinear case is a
// select. A branch around the uses of the loaded values would let a whole wave
// skip them, after which the compiler must treat those loads as still in
// flight and waits for them at the next write of their registers (inside the
// scan's solve: s_waitcnt vmcnt in the middle of the division).
template <int MQ>
__device__ __forceinline__ void mat_stage3(const FlowArgs& A, const MatPos<MQ>& P, float* sM, bool store = true)
{
    const int w = A.lv.w, h = A.lv.h;
#pragma unroll
    for (int u = 0; u < MQ; ++u) {
        const int x = P.xs[u], y = P.ys[u];
        const float dx = P.dx[u], dy = P.dy[u];
        int x1, y1;
        float fx, fy;
        const bool inb = mat_corner(x, y, dx, dy, w, h, x1, y1, fx, fy);
        const float* r0 = P.r0[u];
        const float* p = P.pq[u];
        const float* q = P.pq[u] + 10;
        const f32x2 R0_01 = {r0[0], r0[1]}, R0_23 = {r0[2], r0[3]};
        // in range: the bilinear R1 (the oracle's inside branch)
        const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        const f32x2 A00 = a00, A01 = a01, A10 = a10, A11 = a11;
        const f32x2 P01 = {p[0], p[1]}, P23 = {p[2], p[3]}, P56 = {p[5], p[6]}, P78 = {p[7], p[8]};
        const f32x2 Q01 = {q[0], q[1]}, Q23 = {q[2], q[3]}, Q56 = {q[5], q[6]}, Q78 = {q[7], q[8]};
        const f32x2 I23 = A00 * P01 + A01 * P56 + A10 * Q01 + A11 * Q56;
        f32x2 I45 = A00 * P23 + A01 * P78 + A10 * Q23 + A11 * Q78;
        float i6 = a00 * p[4] + a01 * p[9] + a10 * q[4] + a11 * q[9];
        I45 = (R0_23 + I45) * (f32x2)0.5f;
        i6 = (r0[4] + i6) * 0.25f;
        // out of range: R1 terms zero
        f32x2 R23 = inb ? I23 : (f32x2)0.f;
        f32x2 R45 = inb ? I45 : R0_23;
        float r6 = inb ? i6 : r0[4] * 0.5f;
        R23 = (R0_01 - R23) * (f32x2)0.5f;
        R23 = R23 + ((f32x2){R45.x, r6} * (f32x2)dy + (f32x2){r6, R45.y} * (f32x2)dx);
        if ((unsigned)(x - 5) >= (unsigned)(w - 10) || (unsigned)(y - 5) >= (unsigned)(h - 10)) {
            const float scale = (x < 5 ? border_w(x) : 1.f) * (x >= w - 5 ? border_w(w - x - 1) : 1.f) *
                                (y < 5 ? border_w(y) : 1.f) * (y >= h - 5 ? border_w(h - y - 1) : 1.f);
            R23 = R23 * (f32x2)scale;
            R45 = R45 * (f32x2)scale;
            r6 *= scale;
        }
        const f32x2 G = R45 * R45 + (f32x2)(r6 * r6);
        const f32x2 Hh = (f32x2){R45.x, r6} * (f32x2)R23.x + (f32x2){r6, R45.y} * (f32x2)R23.y;
        const float m1 = (R45.x + R45.y) * r6;
        if (store && P.ok[u]) {
            float* M = sM + P.off[u];
            M[0] = G.x;
            M[1] = m1;
            M[2] = G.y;
            M[3] = Hh.x;
            M[4] = Hh.y;
        }
    }
}

// Hand-off between strips: per (frame, strip, row block) the state of every
// (row, channel) chain after the strip's last column, as one 16-byte slot
// {tag_a, lo, hi, tag_b} (the f64 as two dwords) written by one
// buffer_store_dwordx4 sc1 (write-through past the XCD's L2) and read by
// buffer_load_dwordx4 sc1 (past L1) polls. A slot is its own flag: no separate
// flag store, no drain of the payload stores before it, one round trip for the
// consumer instead of flag + payload. The tags carry the launch's epoch FOLDED
// WITH THE PAYLOAD (slot_tags): tag_a = epoch ^ lo ^ rotl(hi, 13), tag_b =
// epoch ^ hi ^ rotl(lo, 7), and a read is accepted only when both tags match the
// epoch and the lo / hi it read together. So the protocol does not rest on the
// 16-B store being untorn: a read that mixes dwords of this launch's store with
// an older launch's (or never-written memory) fails the check and is re-polled
// unless the mixed-in dwords equal the new ones anyway — accepting a wrong value
// needs both tags to collide, i.e. an old and a new payload whose XOR is one of
// 15 fixed bit patterns AND a torn read of exactly that slot. Every slot is
// written once per launch and a row block's 60 slots fill whole 128-B lines of
// their own. A poll that ever exceeds ~1 s sets `abort` (reported by the host
// as an error) instead of hanging.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int SCAN_RSRC_W3 = 0x00020000;   // gfx9 raw buffer descriptor word 3
constexpr int CPOL_SC1 = 16;               // gfx940+ cache policy bit: sc1

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// the slot of value bits (lo, hi) published in launch `epoch`
__device__ __forceinline__ u32x4 slot_tags(uint32_t epoch, uint32_t lo, uint32_t hi)
{
    return u32x4{epoch ^ lo ^ rotl32(hi, 13), lo, hi, epoch ^ hi ^ rotl32(lo, 7)};
}

__device__ __forceinline__ bool scan_poll(const ScanArgs& S, __amdgpu_buffer_rsrc_t r, uint32_t off, double& v)
{
    unsigned spins = 0;
    for (;;) {
        const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, CPOL_SC1);
        const u32x4 e = slot_tags(S.epoch, q.y, q.z);
        if (q.x == e.x && q.w == e.w) {
            v = __builtin_bit_cast(double, (unsigned long long)q.y | ((unsigned long long)q.z << 32));
            return true;
        }
        if (__hip_atomic_load(S.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1u << 24)) {      // ~1 s: never in a correct run
            __hip_atomic_store(S.abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
    }
}

// SMODE: 0 zero flow, 2 a flow buffer; MM: the largest box radius m served
// (sizes the per-thread M positions)
#ifdef DVC_SCAN_STAMPS
__device__ unsigned long long g_scan_stamps[32 * 96 * 8];
#ifndef DVC_SCAN_STAMP_TID
#define DVC_SCAN_STAMP_TID 0   // the thread whose timeline is stamped (64: wave 1, an M wave)
#endif
#define STAMP(k) do { if (tid == DVC_SCAN_STAMP_TID && t == 0 && w == A.g.W && s < 32 && yb < 96) \
    g_scan_stamps[(s * 96 + yb) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define STAMP(k) do {} while (0)
#endif
#ifndef DVC_SCAN_UF
#define DVC_SCAN_UF 8   // columns per register set of the horizontal chains
#endif
#ifndef DVC_SCAN_FG
#define DVC_SCAN_FG 2   // rows per group of the fast vertical sums' ring loads
#endif
#ifndef DVC_SCAN_VG
#define DVC_SCAN_VG 1   // rows per group of the generic vertical sums' ring loads
#endif
// Vertical running sums of one (column, channel) chain over an interior block
// of RB rows whose first row sits at ring phase PH (y0 % RING == PH * RB), box
// radius M: vsum += (double)(M[y+M] - M[y-M-1]) row by row, OpenCV's order.
// Every ring and sV offset is a constant: per row two ds_read_b32 and one
// ds_write_b64 with immediate offsets and the three VALU ops of the sum (the
// generic loop spends ~30 instructions a row on slot arithmetic, and a wave
// issues at most one instruction every ~4 cycles).
template <int SW, int RB, int M, int PH, int I0 = 0, int I1 = RB>
__device__ __forceinline__ void scan_vsum_rows(const float* mc, double* vc, double& v)
{
    constexpr int RING = scan_ring(RB, M), ROW = scan_nc(SW, M) * 5, VS = scan_vs(SW, M);
    constexpr int G = DVC_SCAN_FG;   // rows whose loads are issued together
#pragma unroll
    for (int i0 = I0; i0 < I1; i0 += G) {
        float fa[G], fb[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int i = i0 + u;
            if (i < I1) {
                fa[u] = mc[((PH * RB + M + i) % RING) * ROW];
                fb[u] = mc[((PH * RB + RING - M - 1 + i) % RING) * ROW];
            }
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int i = i0 + u;
            if (i < I1) {
                v += (double)(fa[u] - fb[u]);
                vc[i * VS] = v;
            }
        }
    }
}

template <int SW, int RB, int M, int PH = 0>
__device__ __forceinline__ void scan_vsum_phase(int ph, const float* mc, double* vc, double& v)
{
    if constexpr (PH < scan_ring(RB, M) / RB) {
        if (ph == PH) scan_vsum_rows<SW, RB, M, PH>(mc, vc, v);
        else scan_vsum_phase<SW, RB, M, PH + 1>(ph, mc, vc, v);
    }
}

// Phase 1 of an interior block for the M waves with one vertical chain each:
// the gathers of block b+1 position by position, each followed by a slice of
// the vertical sums, so the texture addresser drains one position's loads
// while the wave runs the next rows' LDS and VALU work (a burst of every
// gather at the start of the step queued ~0.9 us of vector-memory issue ahead
// of the sums). The ring phase is dispatched per slice: the uniform branch
// keeps each position's loads after the previous slice in program order.
template <int SW, int RB, int M, int I0, int I1, int PH = 0>
__device__ __forceinline__ void scan_vsum_slice(int ph, const float* mc, double* vc, double& v)
{
    if constexpr (PH < scan_ring(RB, M) / RB) {
        if (ph == PH) scan_vsum_rows<SW, RB, M, PH, I0, I1>(mc, vc, v);
        else scan_vsum_slice<SW, RB, M, I0, I1, PH + 1>(ph, mc, vc, v);
    }
}

template <int SW, int RB, int M, int MQ, int U = 0>
__device__ __forceinline__ void scan_phase1_ilv(int ph, const FlowArgs& A, const float* __restrict__ R0,
                                                const float* __restrict__ R1, MatPos<MQ>& P, const float* mc,
                                                double* vc, double& v)
{
    if constexpr (U < MQ) {
        mat_stage2<MQ, U, U + 1>(A, R0, R1, P);
        __builtin_amdgcn_sched_barrier(0);
        scan_vsum_slice<SW, RB, M, RB * U / MQ, RB * (U + 1) / MQ>(ph, mc, vc, v);
        __builtin_amdgcn_sched_barrier(0);
        scan_phase1_ilv<SW, RB, M, MQ, U + 1>(ph, A, R0, R1, P, mc, vc, v);
    }
}

template <int SW, int RB, int NT, int SMODE, int MM>
__device__ void scan_strip(const ScanArgs& S, int t, int s, float* sM, double* sV, int* s_alive)
{
    static_assert(RB * 5 <= 64, "the horizontal chains of a block fit one wave");
    const FlowArgs& A = S.f;
    const OfGeom& g = A.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = A.lv.w, h = A.lv.h, m = g.m;
    const int RING = scan_ring(RB, m), NC = scan_nc(SW, m), VS = scan_vs(SW, m);
    const int X0 = s * SW, X1 = min(X0 + SW, w), CX0 = X0 - m - 1, nx = X1 - X0;
    const size_t lvpx = (size_t)w * h;
    const long long a = A.a0 + t;
    const float* __restrict__ R0 = A.lv.R + (size_t)ring(a - 1, g.RS) * lvpx * 5;
    const float* __restrict__ R1 = A.lv.R + (size_t)ring(a, g.RS) * lvpx * 5;
    const float* src = SMODE == 2 ? A.src + (size_t)t * lvpx * 2 : nullptr;
    float* dst = A.dst ? A.dst + (size_t)t * lvpx * 2 : nullptr;
    // hand-off slots of (frame t, strip s): row block yb at + yb * 1 KB
    const uint32_t slot_bytes = (uint32_t)S.NB * 64u * 16u;
    uint32_t* gp_base = S.gpub + (size_t)(t * S.S + s) * (slot_bytes / 4);
    const __amdgpu_buffer_rsrc_t r_mine =
        __builtin_amdgcn_make_buffer_rsrc(gp_base, 0, (int)slot_bytes, SCAN_RSRC_W3);
    const __amdgpu_buffer_rsrc_t r_left =
        __builtin_amdgcn_make_buffer_rsrc(s > 0 ? gp_base - slot_bytes / 4 : gp_base, 0, (int)slot_bytes, SCAN_RSRC_W3);
    // M positions of rows [rlo, rhi] x the strip's NC columns, ring offsets;
    // the pipelined blocks' M is done by waves 1.. only (NP threads)
    constexpr int NP = NT - 64;
    constexpr int MQ = (RB * scan_nc(SW, MM) + NP - 1) / NP;
    auto place = [&](MatPos<MQ>& P, int q0, int rlo, int npos, int stride) {
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            const int idx = q0 + stride * u;
            P.ok[u] = idx < npos;
            const int ii = P.ok[u] ? idx : 0;
            const int r = rlo + ii / NC, j = ii - (ii / NC) * NC;
            P.xs[u] = min(max(CX0 + j, 0), w - 1);
            P.ys[u] = r;
            P.off[u] = ((r % RING) * NC + j) * 5;
        }
    };
    // the new M rows of the block at y0: rows 0..RB-1+m for the first (vsum's
    // start needs rows 0..m-1), then y0+m .. y0+RB-1+m, clipped to the level
    auto block_rows = [&](int y0, int& rlo, int& npos) {
        rlo = y0 == 0 ? 0 : (y0 + m <= h - 1 ? y0 + m : h);
        const int rhi = min(y0 + RB - 1 + m, h - 1);
        npos = rhi >= rlo ? (rhi - rlo + 1) * NC : 0;
    };
    {   // 1. M of the first block, unpipelined (all threads)
        int rlo, npos;
        block_rows(0, rlo, npos);
        for (int q0 = tid; q0 < npos; q0 += NT * MQ) {
            MatPos<MQ> P;
            place(P, q0, rlo, npos, NT);
            mat_stage1<MQ, SMODE>(A, src, P);
            mat_stage2<MQ>(A, R0, R1, P);
            mat_stage3<MQ>(A, P, sM);
        }
        __syncthreads();
    }
    // Per row block b, three phases separated by the workgroup's barriers, with
    // the roles split by wave (two loops, one per role, the same barriers):
    //   wave 0 (the hand-off wave): phase 1 polls the left strip's flag for b
    //     and loads its published state; phase 2 runs the horizontal chains of
    //     b and stores their final state (sc1) for the right strip; phase 3
    //     drains those stores and raises its own flag. Wave 0 issues no other
    //     vector-memory instruction, so no wait of its own queues behind a
    //     prefetch or a flow store (vmcnt is in order).
    //   waves 1.. (M waves): phase 1 issues block b+1's R loads and block b+2's
    //     flow loads, then the vertical recurrences of b; phase 2 writes block
    //     b+1's M into the ring (FarnebackUpdateMatrices); phase 3 solves b.
    const int slot_last = (h - 1) % RING;
    if (tid < 64) {
        for (int y0 = 0; y0 < h; y0 += RB) {
            const int yb = y0 / RB, nrow = min(RB, h - y0);
            STAMP(0);
            // phase 1: the left strip's state after its last column, lanes
            // (row i, channel c) of block b: poll the slot until published
            double acc = 0.0;
            if (s > 0 && tid < nrow * 5 && !scan_poll(S, r_left, (uint32_t)(yb * 64 + tid) * 16u, acc))
                *s_alive = 0;
            STAMP(2);
            STAMP(7);
            __syncthreads();   // A: the block's vertical sums are in sV
            STAMP(1);
            // phase 2: the horizontal recurrence, lanes (row i, channel c):
            // g += vsum[x+m] - vsum[x-m-1], from the left strip's state (strip 0:
            // OpenCV's (m+2) vsum[0] + vsum[1..m-1] start); g[x] overwrites the
            // consumed vsum[x-m-1] (column x - X0 of sV)
            if (tid < nrow * 5) {
                const int i = tid / 5, c = tid - 5 * i;
                double* v = sV + i * VS + c;   // column j at v[5 j]
                if (s == 0) {
                    acc = v[(0 - CX0) * 5] * (double)(m + 2);
                    for (int x = 1; x < m; ++x) acc += v[(x - CX0) * 5];
                }
                const int ahead = 2 * m + 1;   // column of vsum[x+m] relative to vsum[x-m-1]
                // two register sets of UF columns in turn: set B's LDS loads are
                // in flight while set A adds (they read columns >= x + UF, which
                // A's stores to columns x .. x+UF-1 never touch), and no register
                // copies between the sets, so the compiler's LDS waits count
                // exactly the older loads
                constexpr int UF = DVC_SCAN_UF;
                const double* va = v + ahead * 5;
                auto ld = [&](double (&da)[UF], double (&db)[UF], int x0) {
#pragma unroll
                    for (int u = 0; u < UF; ++u) {
                        da[u] = va[(x0 + u) * 5];
                        db[u] = v[(x0 + u) * 5];
                    }
                };
                auto add = [&](const double (&da)[UF], const double (&db)[UF], int x0) {
#pragma unroll
                    for (int u = 0; u < UF; ++u) {
                        acc += da[u] - db[u];
                        v[(x0 + u) * 5] = acc;
                    }
                };
                int xl = 0;
                if (nx >= 2 * UF) {
                    double a0[UF], b0[UF], a1[UF], b1[UF];
                    ld(a0, b0, 0);
                    for (; xl + 2 * UF <= nx; xl += 2 * UF) {
                        ld(a1, b1, xl + UF);
                        add(a0, b0, xl);
                        if (xl + 3 * UF <= nx) ld(a0, b0, xl + 2 * UF);   // uniform
                        add(a1, b1, xl + UF);
                    }
                }
                for (; xl < nx; ++xl) {
                    const double d = va[xl * 5] - v[xl * 5];
                    acc += d;
                    v[xl * 5] = acc;
                }
                if (s + 1 < S.S) {   // the state after the strip's last column, for the right strip
                    const unsigned long long bits = __builtin_bit_cast(unsigned long long, acc);
                    const u32x4 q = slot_tags(S.epoch, (uint32_t)bits, (uint32_t)(bits >> 32));
                    __builtin_amdgcn_raw_buffer_store_b128(q, r_mine, (uint32_t)(yb * 64 + tid) * 16u, 0, CPOL_SC1);
                }
            }
            STAMP(3);
            __syncthreads();   // B
            STAMP(4);
            const bool alive = *s_alive;   // uniform: written before barrier A
            // phase 3: nothing for wave 0 (the M waves solve the block)
            __syncthreads();   // C: the next block's vertical sums overwrite sV
            STAMP(5);
            if (!alive) break;   // an aborted launch drains
        }
        return;
    }
    // M waves. The pipelined blocks' M positions: P = block b+1 (its R loads in
    // flight from the start of block b's step, its M written in b's phase 2),
    // Q = block b+2 (its flow loads in flight across b's step). Every thread
    // issues its loads unconditionally from valid, clamped positions (positions
    // past the block are !ok and never stored): a load under a divergent branch
    // makes hipcc wait for it at the join, which would expose both global
    // latencies in every step.
    const int mt = tid - 64;   // 0 .. NP-1
    int prow[MQ], pcol[MQ], pidx[MQ];   // this thread's pipelined positions: row in block, column
#pragma unroll
    for (int u = 0; u < MQ; ++u) {
        pidx[u] = mt + NP * u;
        prow[u] = pidx[u] / NC;
        pcol[u] = pidx[u] - prow[u] * NC;
    }
    auto set_block = [&](MatPos<MQ>& Q, int yn) {   // positions of the block at row yn + stage 1
        int nlo, nnpos;
        block_rows(yn, nlo, nnpos);
        const int slo = nlo % RING;
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            Q.ok[u] = pidx[u] < nnpos;   // nnpos <= RB * NC <= NP * MQ
            const int r = Q.ok[u] ? nlo + prow[u] : min(nlo, h - 1), sl = slo + (Q.ok[u] ? prow[u] : 0);
            Q.xs[u] = min(max(CX0 + (Q.ok[u] ? pcol[u] : 0), 0), w - 1);
            Q.ys[u] = r;
            Q.off[u] = ((sl >= RING ? sl - RING : sl) * NC + pcol[u]) * 5;
        }
        mat_stage1<MQ, SMODE>(A, src, Q);
    };
    // vertical chains of this thread: (column, channel) ch = mt + NP k
    const int nch = NC * 5;
    constexpr int KV = (scan_nc(SW, MM) * 5 + NP - 1) / NP;
    double vsum[KV];
#pragma unroll
    for (int k = 0; k < KV; ++k) vsum[k] = 0.0;
    MatPos<MQ> P, Q;
    set_block(P, RB);
    for (int y0 = 0; y0 < h; y0 += RB) {
        const int nrow = min(RB, h - y0);
        const int yb = y0 / RB;
        (void)yb;
        STAMP(0);
        // phase 1: vertical recurrence for the block's rows: vsum += (float)(M[y+m] - M[y-m-1])
        const bool fast = m == MM && y0 - m - 1 >= 0 && y0 + RB - 1 + m <= h - 1;   // uniform
        if (KV == 1 && fast) {
            // every thread runs a chain (threads past the last one repeat it:
            // same values to the same sV words), so the block is straight-line
            const int chc = min(mt, nch - 1), jc = chc / 5, cc = chc - 5 * jc;
            scan_phase1_ilv<SW, RB, MM, MQ>((y0 % RING) / RB, A, R0, R1, P, sM + jc * 5 + cc, sV + chc, vsum[0]);
            set_block(Q, y0 + 2 * RB);   // block b+2: positions and flow loads
            STAMP(6);
        } else {
        mat_stage2<MQ>(A, R0, R1, P);   // 1'. block b+1: R0 and the displaced R1 loads
        set_block(Q, y0 + 2 * RB);      //     block b+2: positions and flow loads
        STAMP(6);
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            // threads past the last chain repeat it (same values to the same sV
            // words), so every thread's vsum is a valid chain state for the
            // straight-line interleaved path above
            const int ch = min(mt + NP * k, nch - 1);
            const int j = ch / 5, c = ch - 5 * j;
            if (y0 == 0) {   // vsum = row0 * (m+2) (a float product) + rows 1..m-1
                vsum[k] = (double)(sM[j * 5 + c] * (float)(m + 2));
                for (int r = 1; r < m; ++r) vsum[k] += (double)sM[((min(r, h - 1) % RING) * NC + j) * 5 + c];
            }
            const float* mc = sM + j * 5 + c;
            if (fast) {   // uniform: an interior block at the variant's radius
                scan_vsum_phase<SW, RB, MM>((y0 % RING) / RB, mc, sV + ch, vsum[k]);
                continue;
            }
            // ring slots of rows y+m (clamped to h-1) and y-m-1 (clamped to 0),
            // stepped (uniform); rows in groups of VG, the group's ring loads
            // issued together
            int sa = (y0 + m) % RING, sb = y0 - m - 1 >= 0 ? (y0 - m - 1) % RING : 0;
            constexpr int VG = DVC_SCAN_VG;
            for (int i0 = 0; i0 < nrow; i0 += VG) {
                float fa[VG], fb[VG];
#pragma unroll
                for (int u = 0; u < VG; ++u) {   // rows past the block read valid (clamped) slots, unused
                    const int y = y0 + i0 + u;
                    const int ta = y + m <= h - 1 ? sa : slot_last, tb = y - m - 1 >= 0 ? sb : 0;
                    fa[u] = mc[ta * NC * 5];
                    fb[u] = mc[tb * NC * 5];
                    sa = sa + 1 == RING ? 0 : sa + 1;
                    if (y - m - 1 >= 0) sb = sb + 1 == RING ? 0 : sb + 1;
                }
#pragma unroll
                for (int u = 0; u < VG; ++u) {
                    if (i0 + u < nrow) {
                        vsum[k] += (double)(fa[u] - fb[u]);
                        sV[(i0 + u) * VS + ch] = vsum[k];
                    }
                }
            }
        }
        }
        STAMP(7);
        __syncthreads();   // A: the M ring is free from here: no reader until the next block's phase 1
        STAMP(1);
        // phase 2: the next block's M into the ring (its loads were issued at
        // the start of the step), alongside wave 0's chains
        mat_stage3<MQ>(A, P, sM);
        STAMP(3);
        __syncthreads();   // B: the block's horizontal sums are in sV
        STAMP(4);
        const bool alive = *s_alive;   // uniform: written before barrier A
        // phase 3: flow = G^-1 h per pixel of the block (a wave = one row of 64 columns)
        // a thread's pixels unrolled and branch-free (clamped LDS rows, results
        // selected by `act`), so the scheduler interleaves their dependent
        // chains (LDS loads, the f64 division); a wave's `act` lanes are its
        // own, every wave runs the ballot of each of its pixels
        constexpr int NQS = (RB * SW + NP - 1) / NP;
        float fxs[NQS], fys[NQS];
#pragma unroll
        for (int q = 0; q < NQS; ++q) {
            const int e = mt + NP * q;
            const int i = e / SW, xl = e - i * SW;
            const double* gg = sV + min(i, RB - 1) * VS + xl * 5;
            const double g11 = gg[0] * g.box_scale, g12 = gg[1] * g.box_scale, g22 = gg[2] * g.box_scale;
            const double h1 = gg[3] * g.box_scale, h2 = gg[4] * g.box_scale;
            const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
            fxs[q] = (float)((g11 * h2 - g12 * h1) * idet);
            fys[q] = (float)((g22 * h1 - g12 * h2) * idet);
        }
#pragma unroll
        for (int q = 0; q < NQS; ++q) asm volatile("" ::"v"(fxs[q]), "v"(fys[q]));   // all solved before any store
#pragma unroll
        for (int q = 0; q < NQS; ++q) {
            const int e = mt + NP * q;
            const int i = e / SW, xl = e - i * SW;
            const int y = y0 + i, x = X0 + xl;
            const bool act = i < nrow && xl < nx;
            const float fxo = act ? fxs[q] : 0.f, fyo = act ? fys[q] : 0.f;
            if (!A.last) {
                if (act) *reinterpret_cast<float2*>(dst + 2u * (uint32_t)(y * w + x)) = make_float2(fxo, fyo);
            } else {
                const float mag = sqrtf(fxo * fxo + fyo * fyo);   // of:82-83
                const unsigned long long word = __ballot(act && mag > g.flow_thr);
                uint64_t* mr = A.mring + (size_t)ring(a, g.RB) * h * g.WW;
                if (lane == 0 && i < nrow) mr[(size_t)y * g.WW + (X0 >> 6)] = word;
                if (A.dbg_flow && t == A.n - 1 && act)
                    *reinterpret_cast<float2*>(A.dbg_flow + ((size_t)y * w + x) * 2) = make_float2(fxo, fyo);
            }
        }
        __syncthreads();   // C: the next block's phase 1 overwrites sV
        STAMP(5);
#pragma unroll
        for (int u = 0; u < MQ; ++u) {   // block b+2 becomes the next step's b+1
            P.ok[u] = Q.ok[u];
            P.xs[u] = Q.xs[u];
            P.ys[u] = Q.ys[u];
            P.off[u] = Q.off[u];
            P.dx[u] = Q.dx[u];
            P.dy[u] = Q.dy[u];
        }
        if (!alive) break;   // an aborted launch drains
    }
}

template <int SW, int RB, int NT, int SMODE, int MM, int OCC>
__global__ void __launch_bounds__(NT, OCC) k_flow_scan(ScanArgs S)
{
    static_assert(SW == 64, "a wave's mask ballot is one 64-column mask word");
    extern __shared__ __attribute__((aligned(16))) double lds_s[];
    const int m = S.f.g.m;
    double* sV = lds_s;
    float* sM = reinterpret_cast<float*>(sV + (size_t)RB * scan_vs(SW, m));
    __shared__ int item, alive;
    const int n = S.f.n;
    for (int k = 0; k < SCAN_Q; ++k) {
        const int q = (int)((blockIdx.x + k) % SCAN_Q);
        const int total = q < n ? ((n - 1 - q) / SCAN_Q + 1) * S.S : 0;   // frames q, q + SCAN_Q, ..
        for (;;) {
            if (threadIdx.x == 0) {
                item = (int)atomicAdd(S.next + q, 1u);
                alive = 1;
            }
            __syncthreads();
            const int it = item;
            __syncthreads();
            if (it >= total) break;
            scan_strip<SW, RB, NT, SMODE, MM>(S, q + SCAN_Q * (it / S.S), it % S.S, sM, sV, &alive);
        }
    }
}

// ------------------------------------------------- scan, pipelined (m == 4) --
// k_flow_scan2: the same FarnebackUpdateFlow_Blur order as k_flow_scan (the
// vertical running sums per column, the horizontal running sums per row, both
// double, OpenCV's order bit for bit), restructured so that the serial work of
// one strip item overlaps across row blocks instead of waiting at barriers.
// One 1024-thread workgroup per CU walks one strip (64 columns + the 2m+1 halo
// columns) of one frame down its row blocks of RB = 12 rows. Interval k (one
// barrier each) runs four stages of four different blocks side by side:
//   wave 0 (chain wave):  C(k)    horizontal sums of block k, in place in its sum buffer
//   M waves, vertical:    V(k+1)  vertical sums of block k+1 -> sum buffer (k+1) % 3
//   M waves, positions:   G(k+2)  M (FarnebackUpdateMatrices) of the rows block k+2's
//                                 vertical sums add -> transfer buffer (k+2) % 2
//   M waves, pixels:      S(k-1)  flow = G^-1 h of block k-1 from sum buffer (k-1) % 3
// The vertical chain of (column, channel) subtracts M[y-m-1], the value it
// added 2m+1 rows earlier: each vertical thread keeps those 9 values in
// registers (a ring whose phase, 12 b mod 9, is a compile-time constant per
// block), so the transfer buffer holds only the block's new rows and the M
// ring of k_flow_scan is gone. Sum buffers are laid out [row][channel][column]
// (74 doubles a line: conflict-free 16-B chain reads and writes), so the chain
// reads its operands as b128 pairs and issues ~2 instructions a column.
namespace scan2 {
constexpr int SW = 64, RB = 12, M = 4, HW = 2 * M + 1, NC = SW + HW;
constexpr int NT = 1024, NMT = NT - 64;
constexpr int P = 74;                   // doubles per (row, channel) line of a sum buffer
constexpr int SVB = RB * 5 * P;         // doubles per sum buffer
constexpr int TR = RB + M;              // rows of a transfer buffer (block 0 takes M rows more)
constexpr int TB = TR * NC * 5;         // floats per transfer buffer
constexpr size_t LDS = (size_t)3 * SVB * 8 + (size_t)2 * TB * 4;
constexpr int NV = NC * 5;              // vertical chains (column, channel)
// Role map of the M waves (wv = 1..15), a nibble per wave (15 = none): the
// wave's vertical-chain slot, solve slot and position slot. Waves w, w+4,
// w+8, w+12 share a SIMD (a workgroup's waves go to the SIMDs cyclically):
// V 1,2,3,5,6,7; S 9,10,11,13,14,15; the chain's mates 4, 8, 12 positions
// only (the partial and the empty position slot on 8 and 12). Other maps —
// solve waves on the chain's SIMD, one 3-row solve wave a SIMD, S and V
// swapped — measured −1.7 … +0.6 % (experiments/README.md, round 5).
constexpr unsigned long long S2_VTAB = 0xffffffff543f210full, S2_STAB = 0x543f210fffffffffull,
                             S2_GTAB = 0xba9e876d543c210full;
constexpr int SPX = 2;                  // solve pixels a thread: rows (SPX r .. SPX r + SPX-1) of a wave's 64 columns
static_assert(NV <= 6 * 64 && RB * NC <= 15 * 64 && RB == 6 * SPX && NT == 16 * 64, "thread roles (k_flow_scan2)");
__device__ __forceinline__ int s2_slot(unsigned long long tab, int wv)
{
    const int v = (int)((tab >> (4 * wv)) & 15ull);
    return v == 15 ? -1 : v;
}
static_assert(RB * 5 <= 64, "a block's horizontal chains fit one wave");
static_assert((2 * P) % 64 != 0 && ((2 * P) / 4) % 2 == 1 && (2 * P) % 4 == 0, "16-B lines on distinct banks");
}  // namespace scan2

// vertical sums of one block for the thread's chain (channel c, column j):
// rows i of the block add T[tr0 + i] (the transfer row of M[y+m]) and subtract
// the value added 9 rows earlier (hist slot (PH + i) % 9); vsum to the sum
// buffer line (i, c) at column j. PH = y0 % 9.
// the 9 values a vertical chain subtracts next: a vector value (constant
// element indices only), so it stays in registers (a float[9] passed by
// reference went to scratch memory)
typedef float Hist9 __attribute__((ext_vector_type(9)));

// row I of a block at ring phase PH (y0 % 9 == PH), then the rows after it up
// to I1: rows are loaded in groups of 3 (the group's LDS reads issued together)
template <int PH, int I, int I1>
__device__ __forceinline__ void scan2_vrows_from(const float* __restrict__ t, double* __restrict__ sv, Hist9& hist,
                                                 double& vsum)
{
    using namespace scan2;
    if constexpr (I < I1) {
        constexpr int N = (I1 - I) < 3 ? (I1 - I) : 3;
        float fa[3];
#pragma unroll
        for (int u = 0; u < N; ++u) fa[u] = t[(I + u) * NC * 5];
        auto row = [&](auto uc) {
            constexpr int u = decltype(uc)::value, i = I + u, S = (PH + i) % HW;
            const float d = fa[u] - hist[S];
            hist[S] = fa[u];
            vsum += (double)d;
            sv[i * 5 * P] = vsum;
        };
        row(std::integral_constant<int, 0>{});
        if constexpr (N > 1) row(std::integral_constant<int, 1>{});
        if constexpr (N > 2) row(std::integral_constant<int, 2>{});
        scan2_vrows_from<PH, I + N, I1>(t, sv, hist, vsum);
    }
}

template <int PH, int I0 = 0, int I1 = scan2::RB>
__device__ __forceinline__ void scan2_vrows(const float* __restrict__ t, double* __restrict__ sv, Hist9& hist,
                                            double& vsum)
{
    scan2_vrows_from<PH, I0, I1>(t, sv, hist, vsum);
}

// rows [I0, I1) of block b's vertical sums for the chain (vc, vj): t0 = the
// block's transfer buffer at (column vj, channel vc), svb = its sum buffer at
// line (0, vc), column vj. Block 0 starts the chain (OpenCV's init) and reads
// its rows M below the transfer buffer's first (rows 0 .. M-1 are the start).
template <int I0, int I1>
__device__ __forceinline__ void scan2_vpart(int b, const float* t0, double* svb, Hist9& hist, double& vsum)
{
    using namespace scan2;
    if (b == 0) {
        if constexpr (I0 == 0) {   // M[0] (m+2) (a float product) + M[1..m-1]; the values
            // subtracted at rows 0..8 are M[max(y-m-1, 0)]
            vsum = (double)(t0[0] * (float)(M + 2));
#pragma unroll
            for (int r = 1; r < M; ++r) vsum += (double)t0[r * NC * 5];
            static_assert(M == 4, "the start below is written out for m == 4");
            const float r0v = t0[0];
            hist = r0v;                   // rows 0..5 subtract M[0]
            hist[6] = t0[1 * NC * 5];     // rows 6..8: M[1..3]
            hist[7] = t0[2 * NC * 5];
            hist[8] = t0[3 * NC * 5];
        }
        scan2_vrows<0, I0, I1>(t0 + M * NC * 5, svb, hist, vsum);
    } else {
        const int ph = (b * RB) % HW;   // 0, 3 or 6
        if (ph == 0) scan2_vrows<0, I0, I1>(t0, svb, hist, vsum);
        else if (ph == 3) scan2_vrows<3, I0, I1>(t0, svb, hist, vsum);
        else scan2_vrows<6, I0, I1>(t0, svb, hist, vsum);
    }
}

#ifdef DVC_SCAN2_STAMPS
__device__ unsigned long long g_scan2_stamps[32 * 96 * 8];
#define STAMP2(tt, kk, j) do { if (t == 0 && A.lv.w == A.g.W && s < 32 && (kk) + 1 >= 0 && (kk) + 1 < 96) \
    g_scan2_stamps[(s * 96 + (kk) + 1) * 8 + (j)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define STAMP2(tt, kk, j) do {} while (0)
#endif
#ifndef DVC_STAMP_DETAIL
#define DVC_STAMP_DETAIL 0   // 1: stamps 4..7 trace wave 10 (S + G) through its interval
#endif
// One role's item loop (CHAIN: wave 0; else the M waves): both take the same
// items and run the same barriers; split at the top so that no value of one
// role is live in the other's code.
template <int SMODE, bool CHAIN>
__device__ __forceinline__ void scan2_role(const ScanArgs& S, double* sv0, float* tb0, int& s_item, int* s_alive)
{
    using namespace scan2;
    const FlowArgs& A = S.f;
    const OfGeom& g = A.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = A.lv.w, h = A.lv.h;
    const int NB = S.NB;
    const size_t lvpx = (size_t)w * h;
    const uint32_t slot_bytes = (uint32_t)NB * 64u * 16u;
    const int n = A.n;
    for (int kq = 0; kq < SCAN_Q; ++kq) {
        const int q = (int)((blockIdx.x + kq) % SCAN_Q);
        const int total = q < n ? ((n - 1 - q) / SCAN_Q + 1) * S.S : 0;
        for (;;) {
            if (tid == 0) s_item = (int)atomicAdd(S.next + q, 1u);
            __syncthreads();
            const int it = s_item;
            __syncthreads();
            // the abort flags of the item: s_alive[k & 1] is written (0) only in
            // interval k, by the chain wave, and read by every wave right after
            // interval k's barrier; the chain wave reaches interval k + 2 (the
            // next write of that flag) only after barrier k + 1, which every M
            // wave passes after its read. Reset here, after the item-start
            // barriers: every read of the previous item's flags came before them
            // (one flag let a wave see interval k+1's abort at k)
            if (tid == 0) {
                s_alive[0] = 1;
                s_alive[1] = 1;
            }
            if (it >= total) break;
            const int t = q + SCAN_Q * (it / S.S), s = it % S.S;
            const int X0 = s * SW, X1 = min(X0 + SW, w), CX0 = X0 - M - 1, nx = X1 - X0;
            const long long a = A.a0 + t;
            const float* __restrict__ R0 = A.lv.R + (size_t)ring(a - 1, g.RS) * lvpx * 5;
            const float* __restrict__ R1 = A.lv.R + (size_t)ring(a, g.RS) * lvpx * 5;
            const float* src = SMODE == 2 ? A.src + (size_t)t * lvpx * 2 : nullptr;
            float* dst = A.dst ? A.dst + (size_t)t * lvpx * 2 : nullptr;
            uint32_t* gp_base = S.gpub + (size_t)(t * S.S + s) * (slot_bytes / 4);
            if constexpr (CHAIN) {
                // ---------------------------------------------- chain wave
                __builtin_amdgcn_s_setprio(3);
                const __amdgpu_buffer_rsrc_t r_mine =
                    __builtin_amdgcn_make_buffer_rsrc(gp_base, 0, (int)slot_bytes, SCAN_RSRC_W3);
                const __amdgpu_buffer_rsrc_t r_left = __builtin_amdgcn_make_buffer_rsrc(
                    s > 0 ? gp_base - slot_bytes / 4 : gp_base, 0, (int)slot_bytes, SCAN_RSRC_W3);
                const bool act = lane < RB * 5;
                const int li = act ? lane : RB * 5 - 1;   // lanes 60..63 repeat lane 59 (same values, same words)
                __syncthreads();   // p0
                for (int k = -1; k <= NB; ++k) {
                    if (lane == 0) STAMP2(t, k, 0);
                    if (k >= 0 && k < NB) {
                        const int nrow = min(RB, h - k * RB);
                        double acc = 0.0;
                        // (lanes 60..63 poll lane 59's slot: they run its chain and
                        // store the same values to the same words)
                        if (s > 0 && li < nrow * 5 && !scan_poll(S, r_left, (uint32_t)(k * 64 + li) * 16u, acc))
                            s_alive[k & 1] = 0;
                        // line (i, c) of the block's sum buffer; column x' = x - CX0
                        double* v = sv0 + (size_t)(k % 3) * SVB + (li / 5) * 5 * P + (li % 5) * P;
                        if (s == 0) {   // OpenCV's start: vsum[0] (m+2) + vsum[1..m-1] (x' = x + m + 1)
                            acc = v[M + 1] * (double)(M + 2);
#pragma unroll
                            for (int x = 1; x < M; ++x) acc += v[x + M + 1];
                        }
                        // g[x] = g[x-1] + (V[x'+9] - V[x']), overwriting V[x'] (x' = xl).
                        // The line as 16-B pairs (pair p = columns 2p, 2p+1) in a
                        // register window: group gi (columns 8gi .. 8gi+7) reads pairs
                        // 4gi .. 4gi+8 and prefetches the 4 pairs group gi+2 adds. A
                        // pair is loaded before any g lands on its columns (g of group
                        // gi covers pairs 4gi .. 4gi+3, all loaded by then).
                        if (lane == 0) STAMP2(t, k, 1);
                        typedef double d2 __attribute__((ext_vector_type(2)));
                        constexpr int NPAIR = (SW + HW + 1) / 2;   // 37: columns 0 .. 73
                        d2* v2 = reinterpret_cast<d2*>(v);
                        d2 win[13];   // pairs 4gi .. 4gi+12 at group gi
#pragma unroll
                        for (int pp = 0; pp < 13; ++pp) win[pp] = v2[pp];
#pragma unroll
                        for (int gi = 0; gi < SW / 8; ++gi) {
                            d2 nxt[4];
                            if (13 + 4 * gi + 3 < NPAIR) {
#pragma unroll
                                for (int u = 0; u < 4; ++u) nxt[u] = v2[13 + 4 * gi + u];
                            }
                            double gv[8];
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                const int ch = u + HW;
                                const double lo = (u & 1) ? win[u >> 1].y : win[u >> 1].x;
                                const double hi = (ch & 1) ? win[ch >> 1].y : win[ch >> 1].x;
                                acc += hi - lo;
                                gv[u] = acc;
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u) v2[4 * gi + u] = d2{gv[2 * u], gv[2 * u + 1]};
#pragma unroll
                            for (int u = 0; u < 9; ++u) win[u] = win[u + 4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) win[9 + u] = nxt[u];
                        }
                        if (s + 1 < S.S && act && lane < nrow * 5) {   // state after column 63 (nx == 64 here)
                            const unsigned long long bits = __builtin_bit_cast(unsigned long long, acc);
                            const u32x4 qv = slot_tags(S.epoch, (uint32_t)bits, (uint32_t)(bits >> 32));
                            __builtin_amdgcn_raw_buffer_store_b128(qv, r_mine, (uint32_t)(k * 64 + lane) * 16u, 0,
                                                                   CPOL_SC1);
                        }
                    }
                    if (lane == 0) STAMP2(t, k, 2);
                    __syncthreads();
                    if (lane == 0) STAMP2(t, k, 3);
                    if (!s_alive[k & 1]) break;   // uniform: interval k's flag, read after its barrier
                }
                __builtin_amdgcn_s_setprio(0);
                continue;
            } else {
            // -------------------------------------------------- M waves
            const int mt = tid - 64;
            // Roles by wave (wv = 1..15). Waves 0, 4, 8, 12 share a SIMD (a
            // workgroup's waves go to the SIMDs cyclically), so the chain wave's
            // SIMD mates 4, 8, 12 take the light role (positions only) and the
            // position slots left over (RB x NC < 15 x 64) fall on waves 8 and 12:
            //   vertical chains + positions:   waves 1, 2, 3, 5, 6, 7
            //   solve (SPX rows) + positions:  waves 9, 10, 11, 13, 14, 15
            //   positions only:                waves 4, 8, 12
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int vslot = s2_slot(S2_VTAB, wv);   // 0..5
            const int sslot = s2_slot(S2_STAB, wv);   // 0 .. RB/SPX - 1
            const int gslot = s2_slot(S2_GTAB, wv);   // 0..14
            // vertical chain of this thread (channel-major: consecutive threads,
            // consecutive columns of one channel)
            const int vidx = vslot * 64 + lane;
            const bool vth = vslot >= 0 && vidx < NV;
            const int vc = (vth ? vidx : 0) / NC, vj = (vth ? vidx : 0) - vc * NC;
            Hist9 hist = 0.f;
            double vsum = 0.0;
            // position of this thread in a block's transfer rows: row pr, column pj
            const int gidx = gslot * 64 + lane;
            const int pr = gidx / NC, pj = gidx - pr * NC;
            const int px = min(max(CX0 + pj, 0), w - 1);
            // the rows whose M block b's vertical sums add: y0 + m .. y0 + m + RB - 1
            auto grow = [&](int b) { return min(b * RB + M + pr, h - 1); };
            // G(b)'s loads are spread over two intervals: its flow loads in
            // interval b-4, its R loads in b-3 (interleaved with that interval's
            // solve and vertical sums, so that the texture unit drains them
            // while the waves compute), its M into the transfer buffer at the
            // start of interval b-2
            // Two position sets in turn (no register copies between them: a copy of
            // a set whose loads are in flight makes the compiler wait for them):
            // at interval k, X holds G(k+2) (its R data arrived) and then takes
            // G(k+4)'s flow loads; Y holds G(k+3)'s flow and takes its R loads.
            MatPos<1> PA, PB;
            auto setpos = [&](MatPos<1>& Q, int b) {
                Q.xs[0] = px;
                Q.ys[0] = grow(b);
                Q.ok[0] = pr < RB;
                Q.off[0] = ((b & 1) * TB) + (pr * NC + pj) * 5;
            };
            auto flowld = [&](MatPos<1>& Q, int b) {
                setpos(Q, b);
                mat_stage1<1, SMODE>(A, src, Q);
            };
            auto ldR0 = [&](MatPos<1>& Q) { ld5(R0 + 5u * (uint32_t)(Q.ys[0] * w + Q.xs[0]), Q.r0[0]); };
            auto ldR1 = [&](MatPos<1>& Q, int row) {   // row 0 / 1 of the displaced 2 x 2 neighbourhood
                int x1, y1;
                float fx, fy;
                (void)mat_corner(Q.xs[0], Q.ys[0], Q.dx[0], Q.dy[0], w, h, x1, y1, fx, fy);
                const int x1c = min(max(x1, 0), max(w - 2, 0)), y1c = min(max(y1, 0), max(h - 2, 0));
                ld10(R1 + 5u * (uint32_t)((y1c + row) * w + x1c), Q.pq[0] + 10 * row);
            };
            {   // p0: M rows 0 .. RB + M - 1 (clamped) -> transfer buffer 0, two passes
                flowld(PB, 1);
                for (int p = mt; p < TR * NC; p += NMT) {
                    const int r = p / NC, j = p - r * NC;
                    MatPos<1> Q;
                    Q.xs[0] = min(max(CX0 + j, 0), w - 1);
                    Q.ys[0] = min(r, h - 1);
                    Q.ok[0] = true;
                    Q.off[0] = p * 5;
                    mat_stage1<1, SMODE>(A, src, Q);
                    mat_stage2<1>(A, R0, R1, Q);
                    mat_stage3<1>(A, Q, tb0);
                }
                mat_stage2<1>(A, R0, R1, PB);   // G(1)'s R loads
                flowld(PA, 2);
            }
            __syncthreads();   // p0
            auto interval = [&](int k, MatPos<1>& X, MatPos<1>& Y) -> bool {
                mat_stage3<1>(A, X, tb0, k + 2 < NB);   // G(k+2) -> transfer buffer (k+2) % 2 (always
                                                        // computed: the loads are consumed on every path)
                if (DVC_STAMP_DETAIL && tid == 640) STAMP2(t, k, 4);   // (detail stamps: wave 10's steps)
                // G(k+3): R loads this interval. Every load below is issued
                // unconditionally (positions are clamped, so always valid; past the
                // last block they are simply unused): a load under a branch makes
                // the compiler wait for it where the branch joins.
                ldR0(Y);
                __builtin_amdgcn_sched_barrier(0);
                // S(k-1) on the solve waves: a wave = SPX rows of 64 columns, the
                // lane's SPX pixels solved side by side (independent f64 chains);
                // their stores are issued at the end of the interval, after this
                // interval's gathers: vmcnt counts loads and stores in one queue,
                // so a store issued before a load makes the next wait for that
                // load wait for the store's completion too
                const bool sdo = k >= 1 && sslot >= 0;
                float fx[SPX], fy[SPX];
                if (sdo) {
                    const int b = k - 1;
                    const int i0 = sslot * SPX, xl = lane;
#pragma unroll
                    for (int q = 0; q < SPX; ++q) {
                        const double* gg = sv0 + (size_t)(b % 3) * SVB + (i0 + q) * 5 * P + xl;
                        const double g11 = gg[0] * g.box_scale, g12 = gg[P] * g.box_scale, g22 = gg[2 * P] * g.box_scale;
                        const double h1 = gg[3 * P] * g.box_scale, h2 = gg[4 * P] * g.box_scale;
                        const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
                        fx[q] = (float)((g11 * h2 - g12 * h1) * idet);
                        fy[q] = (float)((g22 * h1 - g12 * h2) * idet);
                    }
                }
                auto solve_store = [&]() {
                    if (!sdo) return;
                    const int b = k - 1, y0 = b * RB, nrow = min(RB, h - y0);
                    const int i0 = sslot * SPX, xl = lane;
#pragma unroll
                    for (int q = 0; q < SPX; ++q) {
                        const int i = i0 + q, y = y0 + i, x = X0 + xl;
                        const bool act = i < nrow && xl < nx;
                        if (!A.last) {
                            if (act) *reinterpret_cast<float2*>(dst + 2u * (uint32_t)(y * w + x)) = make_float2(fx[q], fy[q]);
                        } else {
                            const float fxo = act ? fx[q] : 0.f, fyo = act ? fy[q] : 0.f;
                            const float mag = sqrtf(fxo * fxo + fyo * fyo);   // of:82-83
                            const unsigned long long word = __ballot(act && mag > g.flow_thr);
                            uint64_t* mr = A.mring + (size_t)ring(a, g.RB) * h * g.WW;
                            if (lane == 0 && i < nrow) mr[(size_t)y * g.WW + (X0 >> 6)] = word;
                            if (A.dbg_flow && t == A.n - 1 && act)
                                *reinterpret_cast<float2*>(A.dbg_flow + ((size_t)y * w + x) * 2) = make_float2(fx[q], fy[q]);
                        }
                    }
                };
                __builtin_amdgcn_sched_barrier(0);
                if (DVC_STAMP_DETAIL && tid == 640) STAMP2(t, k, 5);
                ldR1(Y, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (DVC_STAMP_DETAIL && tid == 640) STAMP2(t, k, 6);
                // V(k+1), rows 0..5 / R row 1 / rows 6..11
                const int vb = k + 1;
                const float* t0 = tb0 + (size_t)(vb & 1) * TB + vj * 5 + vc;
                double* svb = sv0 + (size_t)(vb % 3) * SVB + vc * P + vj;
                if (vth && vb < NB) scan2_vpart<0, RB / 2>(vb, t0, svb, hist, vsum);
                __builtin_amdgcn_sched_barrier(0);
                ldR1(Y, 1);
                __builtin_amdgcn_sched_barrier(0);
                if (vth && vb < NB) scan2_vpart<RB / 2, RB>(vb, t0, svb, hist, vsum);
                flowld(X, k + 4);
                __builtin_amdgcn_sched_barrier(0);
                solve_store();
                if (!DVC_STAMP_DETAIL && tid == 64) STAMP2(t, k, 4);    // arrival at the barrier: wave 1 (V + G)
                if (!DVC_STAMP_DETAIL && tid == 256) STAMP2(t, k, 5);   // wave 4 (G, the chain's SIMD)
                if (!DVC_STAMP_DETAIL && tid == 640) STAMP2(t, k, 6);   // wave 10 (S + G)
                if (tid == (DVC_STAMP_DETAIL ? 640 : 960)) STAMP2(t, k, 7);   // wave 15 (S + G) / wave 10
                __syncthreads();
                return s_alive[k & 1] != 0;   // interval k's flag (k = -1: parity 1, never written)
            };
            // k = -1: X = G(1)'s set (PB), Y = G(2)'s (PA)
            for (int k = -1; k <= NB; k += 2) {
                if (!interval(k, PB, PA)) break;
                if (k + 1 > NB || !interval(k + 1, PA, PB)) break;
            }
            }
        }
    }
}

template <int SMODE>
__global__ void __launch_bounds__(1024, 1) k_flow_scan2(ScanArgs S)
{
    extern __shared__ __attribute__((aligned(16))) double lds_s2[];
    double* sv0 = lds_s2;                                             // 3 sum buffers
    float* tb0 = reinterpret_cast<float*>(lds_s2 + 3 * scan2::SVB);   // 2 transfer buffers
    __shared__ int s_item, s_alive[2];
    if (threadIdx.x < 64) scan2_role<SMODE, true>(S, sv0, tb0, s_item, s_alive);
    else scan2_role<SMODE, false>(S, sv0, tb0, s_item, s_alive);
}

// -------------------------------------------------------------------- vote --
// of:84-86: count of the last L = min(frames, window) raw masks (the deque),
// smoothed = count >= vthr[L]. One lane per 16 px (a u16 of a mask word), the
// counts of its 16 px as bytes in 4 registers, frames walked in order.
__global__ void __launch_bounds__(256) k_vote(OfGeom g, OfBufs b, long long a0, int window, int n)
{
    const int H = g.H, WW = g.WW;
    const size_t nchunk = (size_t)H * WW * 4;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool act = c < nchunk;
    const size_t cc = act ? c : 0;
    uint32_t cnt[4];
    const uint4 c4 = reinterpret_cast<const uint4*>(b.cnt)[cc];
    cnt[0] = c4.x; cnt[1] = c4.y; cnt[2] = c4.z; cnt[3] = c4.w;
    const uint16_t* mr = reinterpret_cast<const uint16_t*>(b.mring);
    uint16_t* sb = reinterpret_cast<uint16_t*>(b.sbits);
    const size_t plane16 = (size_t)H * WW * 4;
    unsigned long long nmot = 0;
    auto spread = [](uint32_t nib) {   // 4 bits -> 4 bytes of 0/1
        return (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
    };
    for (int t = 0; t < n; ++t) {
        const long long a = a0 + t;
        const uint32_t nw = mr[(size_t)ring(a, g.RB) * plane16 + cc];
        const uint32_t ow = a - window >= 1 ? mr[(size_t)ring(a - window, g.RB) * plane16 + cc] : 0u;
        const int L = (int)min<long long>(a, (long long)window);
        const uint32_t thr = b.vthr[L];
        // count >= thr per byte (counts and thresholds 0..255, window <= 255): the
        // even and the odd bytes as u16 lanes plus 256 - thr, bit 8 of each lane
        const uint32_t bias = (0x100u - thr) * 0x00010001u;
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // bytes stay exact: the u32 sum is linear and every final byte is a count <= window
            cnt[j] = cnt[j] + spread((nw >> (4 * j)) & 15u) - spread((ow >> (4 * j)) & 15u);
            const uint32_t ge = (cnt[j] & 0x00ff00ffu) + bias, go = ((cnt[j] >> 8) & 0x00ff00ffu) + bias;
            out |= (((ge >> 8) & 1u) | ((go >> 7) & 2u) | ((ge >> 22) & 4u) | ((go >> 21) & 8u)) << (4 * j);
        }
        nmot += (unsigned long long)__popc(nw);
        if (act) sb[(size_t)t * plane16 + c] = (uint16_t)out;
    }
    if (act) reinterpret_cast<uint4*>(b.cnt)[c] = make_uint4(cnt[0], cnt[1], cnt[2], cnt[3]);
    if (!act) nmot = 0;
    for (int d = 32; d >= 1; d >>= 1) nmot += __shfl_xor(nmot, d, 64);
    if ((threadIdx.x & 63) == 0 && nmot) atomicAdd(b.stats + STAT_SLOT(blockIdx.x) * 4 + 1, nmot);
}

// ---------------------------------------------------------- morphology + CCL
// One workgroup per band of BH rows (one wave per row) of frame blockIdx.y.
// MORPH_CLOSE then MORPH_OPEN with getStructuringElement(MORPH_ELLIPSE,
// (mk, mk)) (of:62,89-90), anchor (a, a), a = mk/2: every pass reads
// src(x + dx, y + dy) over the element's rows dy = -a .. mk-1-a and each row's
// column range; out-of-image neighbours are ignored (0 for dilate, 1 for
// erode). The reference's 2x2 element [[0,1],[1,1]] reads (x, y), (x-1, y),
// (x, y-1) and takes a shift-and-OR form. Four passes need 4a halo rows above
// the band and 4(mk-1-a) below. Then the run index of each row, union-find of
// the band's runs (8-connected) in LDS, band-local roots published as global
// ids (id = y*CAP + k), and every run's bounding box initialised to itself.
// Dynamic LDS: 2 x NRW x WW u64 morph rows (NRW = BH + 4(mk-1)) | run index
// (2 BH WW u64 + 2 BH (WW+1) u16) | BH*CAP u32 parents.

// Bits [start, start + 64) of a mask row of WW words (W valid bits); positions
// outside [0, W) read as `out` (all ones for erode, zeros for dilate).
__device__ __forceinline__ uint64_t row_bits64(const uint64_t* row, int WW, uint64_t lastmask, int start, uint64_t out)
{
    const int w0 = start >> 6, sh = start & 63;   // arithmetic shift: floor for negative starts
    auto word = [&](int i) -> uint64_t {
        if (i < 0 || i >= WW) return out;
        const uint64_t v = row[i];
        return i == WW - 1 ? (v & lastmask) | (out & ~lastmask) : v;
    };
    const uint64_t lo = word(w0);
    return sh ? (lo >> sh) | (word(w0 + 1) << (64 - sh)) : lo;
}

__global__ void __launch_bounds__(512) k_of_band(OfGeom g, OfBufs B, int BH)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const int WW = g.WW, W = g.W, H = g.H, CAP = g.CAP;
    const int t = blockIdx.y;
    const size_t plane = (size_t)H * WW, nr = (size_t)H * CAP;
    const uint64_t* sb = B.sbits + (size_t)t * plane;
    uint64_t* ob = B.obits + (size_t)t * plane;
    const int ma = g.mk / 2, mb = g.mk - 1 - ma;   // element rows above / below the anchor
    const int HA = 4 * ma, NRW = BH + 4 * (g.mk - 1);
    uint64_t* mA = lds;
    uint64_t* mB = mA + NRW * WW;
    uint64_t* l_st = mB + NRW * WW;
    uint64_t* l_en = l_st + BH * WW;
    uint16_t* l_ps = reinterpret_cast<uint16_t*>(l_en + BH * WW);
    uint16_t* l_pe = l_ps + BH * (WW + 1);
    uint32_t* lp = reinterpret_cast<uint32_t*>(l_pe + BH * (WW + 1));
    const int tid = threadIdx.x, nth = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int y0 = blockIdx.x * BH;
    const uint64_t lastmask = (W & 63) ? ((1ull << (W & 63)) - 1) : ~0ull;

    for (int idx = tid; idx < NRW * WW; idx += nth) {
        const int r = idx / WW, wi = idx - r * WW, y = y0 - HA + r;
        mA[idx] = (y >= 0 && y < H) ? sb[(size_t)y * WW + wi] : 0ull;
    }
    __syncthreads();
    // passes: dilate A->B, erode B->A, erode A->B, dilate B->A; pass p has
    // valid sources for buffer rows p*ma .. NRW-1-p*mb
#pragma unroll
    for (int p = 1; p <= 4; ++p) {
        const uint64_t* src = (p & 1) ? mA : mB;
        uint64_t* dst = (p & 1) ? mB : mA;
        const bool dil = p == 1 || p == 4;
        const int r0 = p * ma, r1 = NRW - p * mb;
        for (int idx = r0 * WW + tid; idx < r1 * WW; idx += nth) {
            const int r = idx / WW, wi = idx - r * WW, y = y0 - HA + r;
            if (y < 0 || y >= H) continue;
            uint64_t o;
            if (g.mk == 2) {   // [[0,1],[1,1]]: (x, y), (x-1, y), (x, y-1)
                const uint64_t v = src[idx];
                const uint64_t lb = wi > 0 ? (src[idx - 1] >> 63) : (dil ? 0ull : 1ull);
                const uint64_t left = (v << 1) | lb;
                const uint64_t up = y > 0 ? src[idx - WW] : (dil ? 0ull : ~0ull);
                o = dil ? (v | left | up) : (v & left & up);
            } else {
                const uint64_t outside = dil ? 0ull : ~0ull;
                o = outside;
                for (int i = 0; i < g.mk; ++i) {
                    const int dy = i - ma, lo = g.mlo[i], hi = g.mhi[i];
                    if (lo > hi || y + dy < 0 || y + dy >= H) continue;   // empty row / ignored pixels
                    const uint64_t* row = src + (r + dy) * WW;
                    for (int dx = lo; dx <= hi; ++dx) {
                        const uint64_t v = row_bits64(row, WW, lastmask, wi * 64 + dx, outside);
                        o = dil ? (o | v) : (o & v);
                    }
                }
            }
            if (wi == WW - 1) o &= lastmask;
            dst[idx] = o;
        }
        __syncthreads();
    }
    // morphed rows of the band -> global
    for (int idx = tid; idx < BH * WW; idx += nth) {
        const int r = idx / WW, wi = idx - r * WW, y = y0 + r;
        if (y < H) ob[(size_t)y * WW + wi] = mA[(r + HA) * WW + wi];
    }

    // run index + local union-find (fg, 8-connected)
    const int y = y0 + wave;
    const bool act = wave < BH && y < H;
    uint16_t* rs = B.rs + (size_t)t * nr;
    uint16_t* re = B.re + (size_t)t * nr;
    uint32_t* fpar = B.fpar + (size_t)t * nr;
    uint32_t* bx0 = B.bx0 + (size_t)t * nr;
    uint32_t* bx1 = B.bx1 + (size_t)t * nr;
    uint32_t* by0 = B.by0 + (size_t)t * nr;
    uint32_t* by1 = B.by1 + (size_t)t * nr;
    const uint32_t base = (uint32_t)y * CAP;
    uint64_t* st = l_st + wave * WW;
    uint64_t* en = l_en + wave * WW;
    uint16_t* ps = l_ps + wave * (WW + 1);
    uint16_t* pe = l_pe + wave * (WW + 1);
    int n = 0;
    if (act) {
        n = build_row_idx(mA + (wave + HA) * WW, WW, W, st, en, ps, pe, nullptr);
        for (int i = lane; i < WW; i += 64) {
            uint64_t s = st[i], e = en[i];
            int ks = ps[i], ke = pe[i];
            while (s) { rs[base + ks++] = (uint16_t)(i * 64 + __builtin_ctzll(s)); s &= s - 1; }
            while (e) { re[base + ke++] = (uint16_t)(i * 64 + __builtin_ctzll(e)); e &= e - 1; }
        }
        for (int k = lane; k < n; k += 64) lp[wave * CAP + k] = wave * CAP + k;
        if (lane == 0) B.nfg[(size_t)t * H + y] = (uint32_t)n;
    }
    __syncthreads();
    if (act && wave + 1 < BH && y + 1 < H) {
        const uint32_t f0 = wave * CAP, f1 = f0 + CAP;
        const RowIdx r0{st, en, ps, pe}, r1{st + WW, en + WW, ps + WW + 1, pe + WW + 1};
        for (int i = lane; i < n; i += 64) {
            const int a = select_k(r0.st, r0.ps, WW, i), b = select_k(r0.en, r0.pe, WW, i);
            const int j0 = rank_le(r1.en, r1.pe, WW, a - 2), j1 = rank_le(r1.st, r1.ps, WW, b + 1);
            for (int j = j0; j < j1; ++j) lunion(lp, f0 + i, f1 + j);
        }
    }
    __syncthreads();
    if (act) {
        for (int k = lane; k < n; k += 64) {
            const uint32_t r = lfind(lp, wave * CAP + k);
            fpar[base + k] = (uint32_t)(y0 + r / CAP) * CAP + r % CAP;
            const uint32_t s = rs[base + k], e = re[base + k];
            bx0[base + k] = s;
            bx1[base + k] = e;
            by0[base + k] = (uint32_t)y;
            by1[base + k] = (uint32_t)y;
        }
    }
}

// One wave per band seam (rows b*BH-1, b*BH) of frame blockIdx.y: global
// unions of the runs that touch (8-connected) across it.
__global__ void __launch_bounds__(64) k_of_merge(OfGeom g, OfBufs B, int BH)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const int WW = g.WW, t = blockIdx.y;
    const int y = (blockIdx.x + 1) * BH - 1;
    if (y + 1 >= g.H) return;
    const size_t plane = (size_t)g.H * WW, nr = (size_t)g.H * g.CAP;
    const uint64_t* ob = B.obits + (size_t)t * plane;
    uint32_t* fpar = B.fpar + (size_t)t * nr;
    uint64_t* st = lds;
    uint64_t* en = st + 2 * WW;
    uint16_t* ps = reinterpret_cast<uint16_t*>(en + 2 * WW);
    uint16_t* pe = ps + 2 * (WW + 1);
    const int n0 = build_row_idx(ob + (size_t)y * WW, WW, g.W, st, en, ps, pe, nullptr);
    build_row_idx(ob + (size_t)(y + 1) * WW, WW, g.W, st + WW, en + WW, ps + WW + 1, pe + WW + 1, nullptr);
    __syncthreads();
    const uint32_t b0 = (uint32_t)y * g.CAP, b1 = b0 + g.CAP;
    const int lane = threadIdx.x;
    for (int i = lane; i < n0; i += 64) {
        const int a = select_k(st, ps, WW, i), b = select_k(en, pe, WW, i);
        const int j0 = rank_le(en + WW, pe + WW + 1, WW, a - 2), j1 = rank_le(st + WW, ps + WW + 1, WW, b + 1);
        for (int j = j0; j < j1; ++j) uf_union(fpar, b0 + i, b1 + j);
    }
}

// One wave per row: every run's root (path-compressed), its extents folded
// into the root's bounding box; roots appended to the frame's root list.
__global__ void __launch_bounds__(64) k_of_bbox(OfGeom g, OfBufs B)
{
    const int y = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const size_t nr = (size_t)g.H * g.CAP;
    uint32_t* fpar = B.fpar + (size_t)t * nr;
    const uint16_t* rs = B.rs + (size_t)t * nr;
    const uint16_t* re = B.re + (size_t)t * nr;
    const int n = (int)B.nfg[(size_t)t * g.H + y];
    const uint32_t base = (uint32_t)y * g.CAP;
    int comps = 0;
    for (int k = lane; k < n; k += 64) {
        const uint32_t id = base + k;
        const uint32_t r = uf_find(fpar, id);
        atomicMin(fpar + id, r);
        if (r == id) {
            const uint32_t pos = atomicAdd(B.nroots + t, 1u);
            B.roots[(size_t)t * nr + pos] = id;
            ++comps;
        } else {
            atomicMin(B.bx0 + (size_t)t * nr + r, (uint32_t)rs[id]);
            atomicMax(B.bx1 + (size_t)t * nr + r, (uint32_t)re[id]);
            atomicMin(B.by0 + (size_t)t * nr + r, (uint32_t)y);
            atomicMax(B.by1 + (size_t)t * nr + r, (uint32_t)y);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) comps += __shfl_xor(comps, d, 64);
    if (lane == 0 && comps) atomicAdd(B.stats + STAT_SLOT(y) * 4 + 2, (unsigned long long)comps);
}

// of:93-97: cv2.rectangle(mask, (x, y), (x+w, y+h), 255, -1) of every
// component's bounding rectangle, i.e. rows y0..y1+1 x cols x0..x1+1 (clipped),
// OR-painted as bits. One wave per root (grid-stride), lanes over (row, word).
__global__ void __launch_bounds__(256) k_of_rect(OfGeom g, OfBufs B)
{
    const int t = blockIdx.y, lane = threadIdx.x & 63;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), nwv = gridDim.x * 4;
    const size_t nr = (size_t)g.H * g.CAP;
    const uint32_t cnt = B.nroots[t];
    uint64_t* rb = B.rbits + (size_t)t * g.H * g.WW;
    for (uint32_t i = wv; i < cnt; i += nwv) {
        const uint32_t r = B.roots[(size_t)t * nr + i];
        const int xa = (int)B.bx0[(size_t)t * nr + r], xb = min((int)B.bx1[(size_t)t * nr + r] + 1, g.W - 1);
        const int ya = (int)B.by0[(size_t)t * nr + r], yb = min((int)B.by1[(size_t)t * nr + r] + 1, g.H - 1);
        const int ws = xa >> 6, we = xb >> 6, nw = we - ws + 1;
        const int tot = (yb - ya + 1) * nw;
        for (int q = lane; q < tot; q += 64) {
            const int row = ya + q / nw, wi = ws + q % nw;
            uint64_t mk = ~0ull;
            if (wi == ws) mk &= ~0ull << (xa & 63);
            if (wi == we) mk &= ~0ull >> (63 - (xb & 63));
            atomicOr(reinterpret_cast<unsigned long long*>(rb + (size_t)row * g.WW + wi), (unsigned long long)mk);
        }
    }
}

// k_of_out: one group of 8 lanes per 8x8 block (lane r = row r of the block),
// 8 blocks side by side per wave (64 px x 8 rows), 4 waves = 4 block rows.
// Per static full block and channel (of:156-168) the separable DCT, quantiser
// and IDCT of block_dct_quant<8> — same dot products, same operation order —
// with row passes in the lane's registers and column passes after 8x8
// transposes through LDS (rows padded to 9 floats: conflict-free); a group
// only ever exchanges data within its own wave, so wave-level ordering suffices.
// Small per-lane state: many waves per SIMD instead of one 270-VGPR wave.
__device__ __forceinline__ void dct_rows8(const float (&x)[8], const DctMat& M, float (&y)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // y[k] = sum_n x[n] M[k][n]
        float t = x[0] * M.m[k * 8];
#pragma unroll
        for (int n = 1; n < 8; ++n) t = __builtin_fmaf(x[n], M.m[k * 8 + n], t);
        y[k] = t;
    }
}

__device__ __forceinline__ void idct_rows8(const float (&x)[8], const DctMat& M, float (&y)[8])
{
#pragma unroll
    for (int n = 0; n < 8; ++n) {   // y[n] = sum_l x[l] M[l][n]
        float t = x[0] * M.m[n];
#pragma unroll
        for (int l = 1; l < 8; ++l) t = __builtin_fmaf(x[l], M.m[l * 8 + n], t);
        y[n] = t;
    }
}

// S: the group's 8 x 9 tile. Lane r stores v as row r and returns column r.
__device__ __forceinline__ void transpose8(float* S, int r, const float (&v)[8], float (&out)[8])
{
    wave_sync_lds();
#pragma unroll
    for (int k = 0; k < 8; ++k) S[r * 9 + k] = v[k];
    wave_sync_lds();
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = S[i * 9 + r];
}

// OI: the compressed frame as the encoder's I420 input (DVC_FLAG_OUT_I420,
// cvtColor BGR2YUV_I420 of the BGR frame: color_core.h) as a template parameter, so
// the BGR instantiation carries none of it. The lane's 8 luma bytes go out as
// two dwords; lanes of even rows hold the top-left pixel of each 2x2 quad at
// j = 0, 2, 4, 6 and store its 4 U and 4 V samples — no cross-lane traffic.
// (A static block is grey, so its chroma is 128: the general form gives that.)
template <bool OI>
__global__ void __launch_bounds__(256) k_of_out(OfGeom g, OfBufs B, OfOutArgs o)
{
    __shared__ float sT[4][8][72];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = blockIdx.z;
    const int W = g.W, H = g.H, WW = g.WW;
    const int gb = lane >> 3, r = lane & 7;
    const int bx = (blockIdx.x * 8 + gb) * 8, by = (blockIdx.y * 4 + wave) * 8, y = by + r;
    const bool act = bx < W && y < H;
    // px of this lane's row segment inside the frame: 8, or fewer in the
    // partial block column at the right edge (any W, of:159,177 skip those
    // blocks; their pixels still take the YCrCb round trip, of:170-171)
    const int np = act ? min(8, W - bx) : 0;
    float* S = sT[wave][gb];
    const uint64_t* rb = o.mbits ? o.mbits + (size_t)t * o.mbstride : B.rbits + (size_t)t * H * WW;
    const uint32_t mrow = act ? (uint32_t)(rb[(size_t)y * WW + (bx >> 6)] >> (bx & 63)) & 0xffu : 0u;
    uint32_t any = mrow;
    any |= __shfl_xor(any, 1, 8);
    any |= __shfl_xor(any, 2, 8);
    any |= __shfl_xor(any, 4, 8);
    if (o.mask && act) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo |= ((mrow >> j) & 1u) ? (255u << (8 * j)) : 0u;
            hi |= ((mrow >> (j + 4)) & 1u) ? (255u << (8 * j)) : 0u;
        }
        uint8_t* mp = o.mask + (size_t)t * o.mstride + (size_t)y * W + bx;
        if (np == 8 && ((uintptr_t)mp & 7) == 0) {
            *reinterpret_cast<uint2*>(mp) = make_uint2(lo, hi);
        } else {   // rows of W bytes: any W
            for (int j = 0; j < np; ++j) mp[j] = (uint8_t)((j < 4 ? lo >> (8 * j) : hi >> (8 * (j - 4))) & 255u);
        }
    }
    if (!o.compressed) return;
    // this lane's row of the block: BGR -> YCrCb (of:156)
    int ch[3][8];
    {
        const uint8_t* src8 = o.bgr + (size_t)t * o.fstride + (size_t)(act ? y : 0) * o.pitch + 3 * (act ? bx : 0);
        uint32_t px[6];
        if (o.sf.fmt != DVC_FMT_BGR) {
            // a 4:2:0 surface read in place: the 8 px's luma (2 dwords, aligned:
            // pitch % 4 == 0, bx % 8 == 0) and the 4 chroma pairs of their 2x2
            // quads, cvtColor YUV2BGR (px_device.h) into the 24 BGR bytes
            const uint8_t* f = o.bgr + (size_t)t * o.fstride;
            const uint8_t* yr = f + (size_t)(act ? y : 0) * o.pitch + (act ? bx : 0);
            const size_t dv = o.sf.voff - o.sf.uoff;
            const int cst = o.sf.fmt == DVC_FMT_NV12 ? 2 : 1;   // bytes between chroma samples
            const uint8_t* cu = f + chroma_off(o.sf, act ? y : 0, act ? bx : 0);
            uint32_t y8[2] = {0, 0};
            int us[4] = {0, 0, 0, 0}, vs[4] = {0, 0, 0, 0};
            if (np == 8) {
                y8[0] = reinterpret_cast<const uint32_t*>(yr)[0];
                y8[1] = reinterpret_cast<const uint32_t*>(yr)[1];
            } else {
                for (int k = 0; k < np; ++k) y8[k >> 2] |= (uint32_t)yr[k] << (8 * (k & 3));
            }
            for (int k = 0; k < (np + 1) / 2; ++k) {   // sides even (4:2:0): whole pairs
                us[k] = cu[k * cst];
                vs[k] = cu[dv + (size_t)k * cst];
            }
            yuvpx::yuv4_bgr(y8[0], us[0], vs[0], us[1], vs[1], px);
            yuvpx::yuv4_bgr(y8[1], us[2], vs[2], us[3], vs[3], px + 3);
        } else if (np == 8) {   // 24 bytes, dword aligned (pitch, fstride % 4 == 0; 3 bx % 24 == 0)
            const uint32_t* src = reinterpret_cast<const uint32_t*>(src8);
#pragma unroll
            for (int d = 0; d < 6; ++d) px[d] = src[d];
        } else {
#pragma unroll
            for (int d = 0; d < 6; ++d) px[d] = 0;
            for (int k = 0; k < 3 * np; ++k) px[k >> 2] |= (uint32_t)src8[k] << (8 * (k & 3));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            bgr_to_ycrcb((int)bgr_at(px, j, 0), (int)bgr_at(px, j, 1), (int)bgr_at(px, j, 2), ch[0][j], ch[1][j], ch[2][j]);
    }
    const bool sfull = any == 0 && bx + 8 <= W && by + 8 <= H;   // uniform per group
    if (sfull) {   // of:158-168, Y, Cr and Cb
        auto channel = [&](int (&cc)[8]) {
            float x[8], v[8], u[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = (float)cc[j] - 128.0f;
            dct_rows8(x, kDct8, v);            // T row r
            transpose8(S, r, v, u);          // T column r: u[i] = T[i][r]
#pragma unroll
            for (int k = 0; k < 8; ++k) {    // X[k][r] = rint(sum_i M[k][i] T[i][r] / q) q
                float tt = kDct8.m[k * 8] * u[0];
#pragma unroll
                for (int i = 1; i < 8; ++i) tt = __builtin_fmaf(kDct8.m[k * 8 + i], u[i], tt);
                v[k] = __builtin_rintf(div_rn(tt, o.qinv)) * o.quant;
            }
            transpose8(S, r, v, x);          // X row r
            idct_rows8(x, kDct8, v);           // T2 row r
            transpose8(S, r, v, u);          // T2 column r
#pragma unroll
            for (int i = 0; i < 8; ++i) {    // X[i][r] = sum_k M[k][i] T2[k][r]
                float tt = kDct8.m[i] * u[0];
#pragma unroll
                for (int k = 1; k < 8; ++k) tt = __builtin_fmaf(kDct8.m[k * 8 + i], u[k], tt);
                v[i] = tt;
            }
            transpose8(S, r, v, x);          // row r of the reconstruction
#pragma unroll
            for (int j = 0; j < 8; ++j) {    // np.clip + truncating uint8 assignment
                float f = x[j] + 128.0f;
                f = f < 0.f ? 0.f : (f > 255.f ? 255.f : f);
                cc[j] = (int)((uint32_t)f & 255u);
            }
        };
        channel(ch[0]);
        channel(ch[1]);
        channel(ch[2]);
    }
    if (!act) return;
    if constexpr (OI) {
        uint32_t yo[8], uo[4], vo[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {   // as below, then BGR2YUV_I420 of the pixel
            uint8_t p[3];
            ycrcb_to_bgr(ch[0][j], ch[1][j], ch[2][j], p);
            int b = p[0], gg = p[1], rr = p[2];
            if (sfull) b = gg = rr = (int)gray_px(b, gg, rr);
            yo[j] = yuvpx::luma(b, gg, rr);
            if (!(j & 1)) {
                uo[j >> 1] = yuvpx::chroma_u(b, gg, rr);
                vo[j >> 1] = yuvpx::chroma_v(b, gg, rr);
            }
        }
        // frame t: Y plane W x H, then U and V planes of W/2 x H/2 (W, H even: np is even)
        uint8_t* f = o.compressed + (size_t)t * o.ostride;
        uint8_t* yp = f + (size_t)y * W + bx;
        if (np == 8 && ((uintptr_t)yp & 3) == 0) {
            uint32_t* d = reinterpret_cast<uint32_t*>(yp);
            d[0] = pack4(yo[0], yo[1], yo[2], yo[3]);
            d[1] = pack4(yo[4], yo[5], yo[6], yo[7]);
        } else {   // rows of W bytes: W % 4 != 0 leaves odd rows unaligned
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < np) yp[j] = (uint8_t)yo[j];
        }
        if (y & 1) return;
        uint8_t* up = f + (size_t)W * H + (size_t)(y >> 1) * (W >> 1) + (bx >> 1);
        uint8_t* vp = up + (size_t)(W >> 1) * (H >> 1);
        if (np == 8 && (((uintptr_t)up | (uintptr_t)vp) & 3) == 0) {
            *reinterpret_cast<uint32_t*>(up) = pack4(uo[0], uo[1], uo[2], uo[3]);
            *reinterpret_cast<uint32_t*>(vp) = pack4(vo[0], vo[1], vo[2], vo[3]);
        } else {   // chroma rows of W/2 bytes: W % 8 != 0
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (2 * k < np) {
                    up[k] = (uint8_t)uo[k];
                    vp[k] = (uint8_t)vo[k];
                }
        }
        return;
    }
    uint8_t ob[24];
#pragma unroll
    for (int j = 0; j < 8; ++j) {   // YCrCb -> BGR (of:170-171); static blocks -> gray -> BGR (of:174-183)
        uint8_t p[3];
        ycrcb_to_bgr(ch[0][j], ch[1][j], ch[2][j], p);
        uint32_t b = p[0], gg = p[1], rr = p[2];
        if (sfull) b = gg = rr = gray_px(b, gg, rr);
        ob[3 * j] = (uint8_t)b;
        ob[3 * j + 1] = (uint8_t)gg;
        ob[3 * j + 2] = (uint8_t)rr;
    }
    uint8_t* d8 = o.compressed + (size_t)t * o.ostride + (size_t)y * 3 * W + 3 * bx;
    if (np == 8 && ((uintptr_t)d8 & 3) == 0) {
        uint32_t* d = reinterpret_cast<uint32_t*>(d8);
#pragma unroll
        for (int q = 0; q < 6; ++q)
            d[q] = pack_bytes(ob[4 * q], ob[4 * q + 1], ob[4 * q + 2], ob[4 * q + 3]);
    } else {   // rows of 3W bytes: W % 4 != 0 leaves odd rows unaligned
        for (int k = 0; k < 3 * np; ++k) d8[k] = ob[k];
    }
}

// compress_with_motion's gate from a decoded mask frame (of:141-149): a
// 3-channel mask (what VideoCapture returns for mask.mp4) is cvtColor'd to
// gray first, exactly — a coloured pixel can gray to 0 — then "nonzero" is the
// motion bit the block test `block_mask.mean() == 0` reads. One lane per
// pixel, a wave per 64-px mask word (ballot), 4 words per workgroup.
__global__ void __launch_bounds__(256) k_mask_bits(const uint8_t* __restrict__ mask, size_t mpitch, size_t mstride,
                                                   int channels, int W, int H, int WW, uint64_t* __restrict__ bits)
{
    const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6), y = blockIdx.y, t = blockIdx.z;
    if (wi >= WW) return;   // uniform per wave
    const int x = wi * 64 + lane;
    bool on = false;
    if (x < W) {
        const uint8_t* m = mask + (size_t)t * mstride + (size_t)y * mpitch;
        on = channels == 3 ? gray_px(m[3 * x], m[3 * x + 1], m[3 * x + 2]) != 0 : m[x] != 0;
    }
    const unsigned long long word = __ballot(on);
    if (lane == 0) bits[((size_t)t * H + y) * WW + wi] = word;
}

hipError_t of_launch_mask_bits(const uint8_t* mask, size_t mpitch, size_t mstride, int channels, int W, int H, int n,
                               uint64_t* bits, hipStream_t s)
{
    const int WW = (W + 63) / 64;
    hipLaunchKernelGGL(k_mask_bits, dim3((WW + 3) / 4, H, n), dim3(256), 0, s, mask, mpitch, mstride, channels, W, H,
                       WW, bits);
    return hipGetLastError();
}

// Static-block counter (separate tiny pass keeps k_of_out's exits simple).
__global__ void __launch_bounds__(256) k_of_count_static(OfGeom g, OfBufs B, int n)
{
    const int W = g.W, H = g.H, WW = g.WW;
    const int nbx = W / 8, nby = H / 8;
    const size_t tot = (size_t)nbx * nby * n;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool st = false;
    if (i < tot) {
        const int t = (int)(i / ((size_t)nbx * nby));
        const int rem = (int)(i % ((size_t)nbx * nby));
        const int byi = rem / nbx, bxi = rem % nbx;
        const uint64_t* rb = B.rbits + (size_t)t * H * WW;
        uint32_t any = 0;
        for (int r = 0; r < 8; ++r) any |= (uint32_t)(rb[(size_t)(byi * 8 + r) * WW + (bxi * 8 >> 6)] >> ((bxi * 8) & 63)) & 0xffu;
        st = any == 0;
    }
    const unsigned long long bal = __ballot(st);
    if ((threadIdx.x & 63) == 0 && bal)
        atomicAdd(B.stats + STAT_SLOT(blockIdx.x) * 4 + 3, (unsigned long long)__popcll(bal));
}

// --------------------------------------------------------------- launchers --
// k_of_band's dynamic LDS at `bh` rows a workgroup: the morph rows with their
// 4 (mk - 1) halo rows, the run index, the parents
static size_t of_band_lds(const OfGeom& g, int bh)
{
    return (size_t)16 * (bh + 4 * (g.mk - 1)) * g.WW + (size_t)16 * bh * g.WW + (size_t)4 * bh * (g.WW + 1) +
           (size_t)4 * bh * g.CAP + 16;
}

size_t of_mask_min_lds(const OfGeom& g) { return of_band_lds(g, 1); }

static int of_band_rows(const OfGeom& g, size_t* lds)
{
    static const int bh0 = [] {   // DVC_OF_BH (experiments): rows per k_of_band workgroup, 8 / 4 / 2 / 1
        const char* e = dvc::tune_env("DVC_OF_BH");
        const int v = e ? atoi(e) : 8;
        return v == 4 || v == 2 || v == 1 ? v : 8;
    }();
    int bh = bh0;
    for (;;) {
        const size_t b = of_band_lds(g, bh);
        if (b <= 150 * 1024 || bh == 1) {
            *lds = b;
            return bh;
        }
        bh >>= 1;
    }
}

// Frame numbers as the kernels see them: a0 itself up to RED_K (so the vote's
// `a - window >= 1` and `min(a, window)` read the true values; window <= 255),
// beyond it RED_K + (a0 - RED_K) mod lcm(RS, RB) — the same slot in both rings.
static constexpr long long RED_K = 256;
static long long reduce_frame(const OfGeom& g, long long a0)
{
    if (a0 <= RED_K) return a0;
    const long long p = std::lcm((long long)g.RS, (long long)g.RB);
    return RED_K + (a0 - RED_K) % p;
}

hipError_t of_launch_pyramid(const OfGeom& g, const Level* lv, const OfBufs& b, const uint8_t* bgr, int pitch,
                             size_t fstride, const SrcFmt& sf, long long a0, int n, hipStream_t s, hipStream_t s2,
                             hipEvent_t ev_gray, hipEvent_t ev_side)
{
    a0 = reduce_frame(g, a0);
    if (n <= 0) return hipSuccess;
    {
        dim3 grid((g.W + PT_W - 1) / PT_W, (g.H + PT_H - 1) / PT_H, n);
#define DVC_FRONT0(PNv, FMTv) \
    hipLaunchKernelGGL((k_of_front0<PNv, FMTv>), grid, dim3(256), 0, s, g, lv[0], b.gray, bgr, pitch, fstride, sf, a0)
        const bool p5 = g.pc.n == 5;
        switch (sf.fmt) {
        case DVC_FMT_I420: if (p5) DVC_FRONT0(5, DVC_FMT_I420); else DVC_FRONT0(7, DVC_FMT_I420); break;
        case DVC_FMT_NV12: if (p5) DVC_FRONT0(5, DVC_FMT_NV12); else DVC_FRONT0(7, DVC_FMT_NV12); break;
        default: if (p5) DVC_FRONT0(5, DVC_FMT_BGR); else DVC_FRONT0(7, DVC_FMT_BGR); break;
        }
#undef DVC_FRONT0
    }
    // Levels 1..L each smooth and resize the full-resolution gray (OpenCV's
    // pyramid, not a recursive one), so they are independent: with a side
    // stream, levels 2..L run beside level 1 (their latency-bound blur passes
    // overlap), and s waits for them at the end
    const bool side = s2 && ev_gray && ev_side && g.L >= 2;
    if (side) {
        hipError_t e = hipEventRecord(ev_gray, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(s2, ev_gray, 0);
        if (e != hipSuccess) return e;
    }
    for (int k = 1; k <= g.L; ++k) {
        hipStream_t sk = side && k >= 2 ? s2 : s;
        if ((size_t)8 * g.GP <= PH_F32_LDS)
            hipLaunchKernelGGL(k_pyr_h<true>, dim3((g.H + PH_ROWS - 1) / PH_ROWS, n), dim3(256), (size_t)8 * g.GP, sk, g,
                               lv[k], b.gray);
        else   // wide frames: byte rows (GP <= 65520 B of LDS)
            hipLaunchKernelGGL(k_pyr_h<false>, dim3((g.H + PH_ROWS - 1) / PH_ROWS, n), dim3(256), (size_t)g.GP, sk, g,
                               lv[k], b.gray);
        hipLaunchKernelGGL(k_pyr_v, dim3((2 * lv[k].w + 255) / 256, (2 * lv[k].h + PV_ROWS - 1) / PV_ROWS, n), dim3(256),
                           0, sk, g, lv[k]);
        dim3 gp((lv[k].w + PT_W - 1) / PT_W, (lv[k].h + PT_H - 1) / PT_H, n);
        if (g.pc.n == 5) hipLaunchKernelGGL(k_pyr_poly<5>, gp, dim3(256), 0, sk, g, lv[k], a0);
        else hipLaunchKernelGGL(k_pyr_poly<7>, gp, dim3(256), 0, sk, g, lv[k], a0);
    }
    if (side) {
        hipError_t e = hipEventRecord(ev_side, s2);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ev_side, 0);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// The coarser level's final flow bilinearly upsampled (the taps ux/uy of
// the level, x g.up) into a flow buffer of this level: the value the direct
// kernel computes inline per position (src_mode 1), same products, same order.
// Four pixels per lane (two 16-B stores): the kernel writes 8 B/px and reads
// the coarse flow from L2, so it is store-issue / HBM bound.
// LDS-staged form (lv.up_rows > 0): the workgroup's coarse rows are loaded
// once as 16-B words and the four taps of every output pixel read from LDS —
// the gather form spent four 8-B vector-memory loads per pixel, texture-
// addresser bound (~4x the time of its 8-B/px stores). Same products, same
// order, so the same bits.
// Shared by both kernels below: one output pixel from its four coarse neighbours (a0, a1 of the upper
// source row, b0, b1 of the lower) and its taps into v[0..1]; a lane's four pixels (x0 % 4 == 0) out to o.
__device__ __forceinline__ void flow_up_px(float2 a0, float2 a1, float2 b0, float2 b1, const LinTap& tx,
                                           const LinTap& ty, float up, float* v)
{
    const float t0x = a0.x * tx.w0 + a1.x * tx.w1, t1x = b0.x * tx.w0 + b1.x * tx.w1;
    const float t0y = a0.y * tx.w0 + a1.y * tx.w1, t1y = b0.y * tx.w0 + b1.y * tx.w1;
    v[0] = (t0x * ty.w0 + t1x * ty.w1) * up;
    v[1] = (t0y * ty.w0 + t1y * ty.w1) * up;
}
__device__ __forceinline__ void flow_up_store(float* o, const float (&v)[8], int x0, int w)
{
    if (x0 + 4 <= w && !(w & 1)) {   // 16-B aligned: x0 % 4 == 0 and rows of an even width
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {   // the row's last lane, or rows of an odd width (8-B aligned only)
        const int np = min(4, w - x0);
        for (int k = 0; k < np; ++k) *reinterpret_cast<float2*>(o + 2 * k) = make_float2(v[2 * k], v[2 * k + 1]);
    }
}

__global__ void __launch_bounds__(256) k_flow_up_lds(FlowArgs A, float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float2 sup[];
    const int w = A.lv.w, h = A.lv.h, sw = A.sw;
    const int y0 = blockIdx.y * A.lv.up_per, ye = min(y0 + A.lv.up_per, h), t = blockIdx.z;
    const float* src = A.src + (size_t)t * sw * A.sh * 2;
    const int r0 = A.lv.uy[y0].s0, nr = A.lv.uy[ye - 1].s1 - r0 + 1;   // <= lv.up_rows (host)
    {   // rows r0 .. r0+nr-1: contiguous floats r0*sw*2 ..
        const float* s0p = src + (size_t)r0 * sw * 2;
        const int nf = nr * sw * 2;
        const bool al = (((uintptr_t)s0p) & 15u) == 0;
        if (al) {
            for (int i = threadIdx.x; 4 * i + 3 < nf; i += 256)
                reinterpret_cast<float4*>(sup)[i] = reinterpret_cast<const float4*>(s0p)[i];
            for (int i = (nf & ~3) + threadIdx.x; i < nf; i += 256) reinterpret_cast<float*>(sup)[i] = s0p[i];
        } else {
            for (int i = threadIdx.x; i < nf; i += 256) reinterpret_cast<float*>(sup)[i] = s0p[i];
        }
    }
    __syncthreads();
    for (int x0 = 4 * (int)threadIdx.x; x0 < w; x0 += 1024) {
        LinTap tx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) tx[k] = A.lv.ux[min(x0 + k, w - 1)];
        for (int y = y0; y < ye; ++y) {
            const LinTap ty = A.lv.uy[y];
            const float2* ra = sup + (ty.s0 - r0) * sw;
            const float2* rb = sup + (ty.s1 - r0) * sw;
            float v[8];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                flow_up_px(ra[tx[k].s0], ra[tx[k].s1], rb[tx[k].s0], rb[tx[k].s1], tx[k], ty, A.g.up, v + 2 * k);
            flow_up_store(out + ((size_t)t * w * h + (size_t)y * w + x0) * 2, v, x0, w);
        }
    }
}

__global__ void __launch_bounds__(256) k_flow_up(FlowArgs A, float* __restrict__ out)
{
    // a workgroup = FU_ROWS rows of one frame (a few hundred thousand one-row
    // workgroups cost more in dispatch than their loads and stores); a lane's
    // column taps are loaded once for the rows
    const int w = A.lv.w, h = A.lv.h;
    const int y0 = blockIdx.y * FU_ROWS, t = blockIdx.z;
    const float* src = A.src + (size_t)t * A.sw * A.sh * 2;
    for (int x0 = 4 * (int)threadIdx.x; x0 < w; x0 += 1024) {
        LinTap tx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) tx[k] = A.lv.ux[min(x0 + k, w - 1)];
        for (int y = y0; y < min(y0 + FU_ROWS, h); ++y) {
            const LinTap ty = A.lv.uy[y];
            const float* ra = src + (uint32_t)(ty.s0 * A.sw) * 2u;
            const float* rb = src + (uint32_t)(ty.s1 * A.sw) * 2u;
            float v[8];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                flow_up_px(*reinterpret_cast<const float2*>(ra + tx[k].s0 * 2), *reinterpret_cast<const float2*>(ra + tx[k].s1 * 2),
                           *reinterpret_cast<const float2*>(rb + tx[k].s0 * 2), *reinterpret_cast<const float2*>(rb + tx[k].s1 * 2),
                           tx[k], ty, A.g.up, v + 2 * k);
            flow_up_store(out + ((size_t)t * w * h + (size_t)y * w + x0) * 2, v, x0, w);
        }
    }
}

// k_flow_scan's blocks of rows: 12 for box radius m <= 4 (winsize <= 9, the
// reference's), 8 above; strips of 64 columns, 512 threads (the launch switch
// in of_launch_flow)
static int scan_rb(const OfGeom& g) { return g.m <= 4 ? 12 : 8; }

size_t of_scan_slots(const OfGeom& g, int w, int h)
{
    const int rb = scan_rb(g);
    return (size_t)((w + 63) / 64) * (size_t)((h + rb - 1) / rb) * 64;
}

hipError_t of_launch_flow(const OfGeom& g, const Level* lv, const OfBufs& b, long long a0, int n, int k_hi, int k_lo,
                          hipStream_t s, unsigned int* epoch, hipEvent_t ev_it0, int* kernel)
{
    a0 = reduce_frame(g, a0);
    static const int cus = [] {
        int dev = 0, c = 256;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c = 256;
        return c;
    }();
    const size_t lds = std::max((size_t)(FL_H + 2 * g.m) * (FL_W + 2 * g.m) * 5 * 4,
                                (size_t)FL_H * (FL_W + 2 * g.m) * 5 * 8);
    // every scan launch of this call takes its own set of SCAN_Q work-queue
    // counters, all zeroed by one fill here: one fill kernel a call instead of
    // one before each launch (each a dependent launch on the flow stream)
    int set = 0;
    if (g.sliding) {
        const hipError_t e = hipMemsetAsync(b.scan_ctr, 0, 4 * SCAN_Q * (size_t)(k_hi - k_lo + 1) * g.iters, s);
        if (e != hipSuccess) return e;
    }
    for (int k = k_hi; k >= k_lo; --k) {
        const Level& L = lv[k];
        dim3 grid((L.w + FL_W - 1) / FL_W, (L.h + FL_H - 1) / FL_H, n);
        for (int it = 0; it < g.iters; ++it) {
            FlowArgs A{};
            A.g = g;
            A.lv = L;
            A.a0 = a0;
            A.n = n;
            if (it > 0) {
                A.src_mode = 2;
                A.src = L.flow[(it - 1) & 1];
            } else if (k < g.L) {
                A.src_mode = 1;
                A.src = lv[k + 1].flow[(g.iters - 1) & 1];
                A.sw = lv[k + 1].w;
                A.sh = lv[k + 1].h;
            } else {
                A.src_mode = 0;
                A.src = nullptr;
            }
            A.last = (k == 0 && it == g.iters - 1);
            A.dst = A.last ? nullptr : L.flow[it & 1];
            A.mring = b.mring;
            A.dbg_flow = b.dbg_flow;
            if (g.sliding) {   // OpenCV's running box sums: strip wavefront
                const int sw = 64, rb = scan_rb(g);
                ScanArgs S{};
                S.f = A;
                S.S = (L.w + sw - 1) / sw;
                S.NB = (L.h + rb - 1) / rb;
                S.gpub = b.scan_g;
                S.next = b.scan_ctr + SCAN_Q * set++;
                S.abort = b.scan_abort;
                S.epoch = ++*epoch;
                if (A.src_mode == 1) {   // upsample into the level's other flow buffer (unused
                    // until iteration 1 writes it), then read it as a flow buffer
                    float* up = L.flow[1];
                    if (L.up_rows > 0)   // the coarse rows fit in LDS (of_api.hip; 0 = the gather form)
                        hipLaunchKernelGGL(k_flow_up_lds, dim3(1, (L.h + L.up_per - 1) / L.up_per, n), dim3(256),
                                           (size_t)L.up_rows * A.sw * 8, s, A, up);
                    else
                        hipLaunchKernelGGL(k_flow_up, dim3(1, (L.h + FU_ROWS - 1) / FU_ROWS, n), dim3(256), 0, s, A, up);
                    S.f.src_mode = 2;
                    S.f.src = up;
                }
                // the pipelined scan for the reference's winsize 9 (m == 4);
                // g.sliding == 1 (DVC_OF_SCAN2=0 at create) selects the
                // barrier-phased k_flow_scan
                const bool use2 = g.m == scan2::M && rb == scan2::RB && g.sliding == 2;
                if (kernel && k == k_lo) *kernel = use2 ? DVC_KTIME_FLOW_SCAN2 : DVC_KTIME_FLOW_SCAN;
                if (use2) {
                    const int items = S.S * n, grid_s = std::max(1, std::min(items, cus));
                    if (S.f.src_mode == 2)
                        hipLaunchKernelGGL(k_flow_scan2<2>, dim3(grid_s), dim3(scan2::NT), scan2::LDS, s, S);
                    else
                        hipLaunchKernelGGL(k_flow_scan2<0>, dim3(grid_s), dim3(scan2::NT), scan2::LDS, s, S);
                    if (ev_it0 && k == k_lo && it == 0) {
                        const hipError_t e = hipEventRecord(ev_it0, s);
                        if (e != hipSuccess) return e;
                    }
                    continue;
                }
                const size_t lds_b = scan_lds_bytes(sw, rb, g.m);
                const int per_cu = std::max(1, std::min(8, (int)(160 * 1024 / lds_b)));
                const int items = S.S * n, grid_s = std::max(1, std::min(items, per_cu * cus));
                const bool sm2 = S.f.src_mode == 2;
#define DVC_SCAN_LAUNCH(RBv, SM, MMv, OCCv) \
    hipLaunchKernelGGL((k_flow_scan<64, RBv, 512, SM, MMv, OCCv>), dim3(grid_s), dim3(512), lds_b, s, S)
                if (g.m > 4 && sm2) DVC_SCAN_LAUNCH(8, 2, OF_MAX_BOX_M, 2);
                else if (g.m > 4) DVC_SCAN_LAUNCH(8, 0, OF_MAX_BOX_M, 2);
                else if (sm2) DVC_SCAN_LAUNCH(12, 2, 4, 4);
                else DVC_SCAN_LAUNCH(12, 0, 4, 4);
#undef DVC_SCAN_LAUNCH
            } else if (g.m == 4) {
                if (kernel && k == k_lo) *kernel = DVC_KTIME_FLOW;
                hipLaunchKernelGGL(k_flow<4>, grid, dim3(256), lds, s, A);
            } else {
                if (kernel && k == k_lo) *kernel = DVC_KTIME_FLOW;
                hipLaunchKernelGGL(k_flow<0>, grid, dim3(256), lds, s, A);
            }
            if (ev_it0 && k == k_lo && it == 0) {   // the caller schedules other work after it
                const hipError_t e = hipEventRecord(ev_it0, s);
                if (e != hipSuccess) return e;
            }
        }
    }
    return hipGetLastError();
}

hipError_t of_launch_mask(const OfGeom& g, const OfBufs& b, long long a0, int window, int n, hipStream_t s)
{
    a0 = reduce_frame(g, a0);
    const size_t nchunk = (size_t)g.H * g.WW * 4;
    hipLaunchKernelGGL(k_vote, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, s, g, b, a0, window, n);
    size_t lds = 0;
    const int BH = of_band_rows(g, &lds);
    const int nb = (g.H + BH - 1) / BH;
    hipError_t e = hipMemsetAsync(b.nroots, 0, 4 * (size_t)n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_of_band, dim3(nb, n), dim3(64 * std::max(BH, 4)), lds, s, g, b, BH);
    if (nb > 1) hipLaunchKernelGGL(k_of_merge, dim3(nb - 1, n), dim3(64), 32 * g.WW + 8 * (g.WW + 1), s, g, b, BH);
    hipLaunchKernelGGL(k_of_bbox, dim3(g.H, n), dim3(64), 0, s, g, b);
    if ((e = hipMemsetAsync(b.rbits, 0, 8 * (size_t)g.H * g.WW * n, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_of_rect, dim3(64, n), dim3(256), 0, s, g, b);
    const size_t nblk = (size_t)(g.W / 8) * (g.H / 8) * n;
    if (nblk) hipLaunchKernelGGL(k_of_count_static, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, g, b, n);
    return hipGetLastError();
}

hipError_t of_launch_out(const OfGeom& g, const OfBufs& b, const OfOutArgs& o, int n, hipStream_t s, bool i420)
{
    if (!o.mask && !o.compressed) return hipSuccess;
    if (!dct8_is_const(o.M)) return hipErrorInvalidValue;   // k_of_out's constant basis
    const int nbx = (g.W + 7) / 8, nby = (g.H + 7) / 8;   // partial edge blocks included (pixels, not DCT)
    dim3 grid((nbx + 7) / 8, (nby + 3) / 4, n);
    if (i420 && ((g.W | g.H) & 1)) return hipErrorInvalidValue;   // 4:2:0: whole 2x2 quads (refused at create)
    if (i420)
        hipLaunchKernelGGL(k_of_out<true>, grid, dim3(256), 0, s, g, b, o);
    else
        hipLaunchKernelGGL(k_of_out<false>, grid, dim3(256), 0, s, g, b, o);
    return hipGetLastError();
}

}  // namespace dvc

#ifdef DVC_SCAN2_STAMPS
extern "C" int dvc_debug_scan2_stamps(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(dvc::g_scan2_stamps), sizeof(dvc::g_scan2_stamps)) == hipSuccess ? 0 : -2;
}
#endif
#ifdef DVC_SCAN_STAMPS
extern "C" int dvc_debug_scan_stamps(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(dvc::g_scan_stamps), sizeof(dvc::g_scan_stamps)) == hipSuccess ? 0 : -2;
}
#endif
