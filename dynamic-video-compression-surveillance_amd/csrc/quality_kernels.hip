// quality_kernels.hip — the quality meter (DESIGN.md "Quality metrics"): per
// frame pair the squared error of B, G, R and luma and the integer 8x8 SSIM of
// the luma, both as exact integers.
//   k_quality_tile   one workgroup per 128 x 32 tile: a lane reads one 4x4 cell of
//                    both frames (three dwords a row where rows are 4-byte
//                    aligned, bytes with bounds otherwise; any pitch in place),
//                    adds its squared errors and leaves the cell's luma sums in
//                    LDS; then one lane per window adds its 2 x 2 cells and
//                    evaluates it; a wave and a workgroup reduction leave five
//                    64-bit partials per tile
//   k_quality_fold   one workgroup per frame adds the tiles' partials and writes
//                    the frame record
// The arithmetic is quality_core.h's. Ordinary vector loads and stores only.
#include "quality_kernels.h"

namespace dvc {
namespace {

// LDS row of cell sums: the tile's 32 cells and the halo column. 33 is odd, so
// the four cells of a window fall in different banks across a wave.
constexpr int kLW = kQualityTileCX + 1;
constexpr int kLH = kQualityTileCY + 1;
constexpr int kHalo = kQualityTileCY + kLW;   // cells of the halo column and the halo row

__device__ __forceinline__ void px4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2,
                                    uint32_t (&sse)[4], QualityCell& c)
{
    quality_px(a0 & 255, (a0 >> 8) & 255, (a0 >> 16) & 255, b0 & 255, (b0 >> 8) & 255, (b0 >> 16) & 255, sse, c);
    quality_px(a0 >> 24, a1 & 255, (a1 >> 8) & 255, b0 >> 24, b1 & 255, (b1 >> 8) & 255, sse, c);
    quality_px((a1 >> 16) & 255, a1 >> 24, a2 & 255, (b1 >> 16) & 255, b1 >> 24, b2 & 255, sse, c);
    quality_px((a2 >> 8) & 255, (a2 >> 16) & 255, a2 >> 24, (b2 >> 8) & 255, (b2 >> 16) & 255, b2 >> 24, sse, c);
}

// The pixels of cell (cx, cy) that lie inside the frame.
__device__ __forceinline__ void cell(const uint8_t* __restrict__ fa, size_t pa, const uint8_t* __restrict__ fb, size_t pb,
                                     int cx, int cy, int W, int H, int aligned, uint32_t (&sse)[4], QualityCell& c)
{
    const int x0 = 4 * cx, y0 = 4 * cy;
    if (aligned && x0 + 4 <= W && y0 + 4 <= H) {
        uint32_t da[4][3], db[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(fa + (size_t)(y0 + r) * pa + 12 * (size_t)cx);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(fb + (size_t)(y0 + r) * pb + 12 * (size_t)cx);
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                da[r][w] = p[w];
                db[r][w] = q[w];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) px4(da[r][0], da[r][1], da[r][2], db[r][0], db[r][1], db[r][2], sse, c);
    } else {
        for (int r = 0; r < 4 && y0 + r < H; ++r) {
            const uint8_t* p = fa + (size_t)(y0 + r) * pa + 3 * (size_t)x0;
            const uint8_t* q = fb + (size_t)(y0 + r) * pb + 3 * (size_t)x0;
            for (int i = 0; i < 4 && x0 + i < W; ++i)
                quality_px(p[3 * i], p[3 * i + 1], p[3 * i + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2], sse, c);
        }
    }
}

__global__ __launch_bounds__(256) void k_quality_tile(const uint8_t* __restrict__ a, size_t pa, size_t sa,
                                                      const uint8_t* __restrict__ b, size_t pb, size_t sb,
                                                      QualityGeom g, uint64_t* __restrict__ partials, int aligned)
{
    __shared__ int s_c[4][kLH * kLW];   // s1, s2, ss, s12 of every cell
    __shared__ uint32_t s_sse[4][4];
    __shared__ long long s_q[4];
    const int t = threadIdx.x, lx = t & (kQualityTileCX - 1), ly = t / kQualityTileCX;
    const int ty = blockIdx.x / g.tiles_x, tx = blockIdx.x - ty * g.tiles_x;
    const int cx0 = tx * kQualityTileCX, cy0 = ty * kQualityTileCY;
    const uint8_t* fa = a + (size_t)blockIdx.y * sa;
    const uint8_t* fb = b + (size_t)blockIdx.y * sb;

    uint32_t sse[4] = {0, 0, 0, 0};
    QualityCell c{0, 0, 0, 0};
    const int cx = cx0 + lx, cy = cy0 + ly;
    if (cx < g.cells_x && cy < g.cells_y) cell(fa, pa, fb, pb, cx, cy, g.W, g.H, aligned, sse, c);
    s_c[0][ly * kLW + lx] = c.s1;
    s_c[1][ly * kLW + lx] = c.s2;
    s_c[2][ly * kLW + lx] = c.ss;
    s_c[3][ly * kLW + lx] = c.s12;
    if (t < kHalo) {   // the cells right of and below the tile: their sums only, and only whole cells
        const int hx = t < kQualityTileCY ? kQualityTileCX : t - kQualityTileCY;
        const int hy = t < kQualityTileCY ? t : kQualityTileCY;
        uint32_t unused[4] = {0, 0, 0, 0};
        QualityCell h{0, 0, 0, 0};
        if (cx0 + hx < g.full_x && cy0 + hy < g.full_y)
            cell(fa, pa, fb, pb, cx0 + hx, cy0 + hy, g.W, g.H, aligned, unused, h);
        s_c[0][hy * kLW + hx] = h.s1;
        s_c[1][hy * kLW + hx] = h.s2;
        s_c[2][hy * kLW + hx] = h.ss;
        s_c[3][hy * kLW + hx] = h.s12;
    }
    __syncthreads();

    long long q = 0;
    if (cx + 1 < g.full_x && cy + 1 < g.full_y) {   // the window whose first cell is this lane's
        const int o = ly * kLW + lx;
        QualityCell w;
        w.s1 = s_c[0][o] + s_c[0][o + 1] + s_c[0][o + kLW] + s_c[0][o + kLW + 1];
        w.s2 = s_c[1][o] + s_c[1][o + 1] + s_c[1][o + kLW] + s_c[1][o + kLW + 1];
        w.ss = s_c[2][o] + s_c[2][o + 1] + s_c[2][o + kLW] + s_c[2][o + kLW + 1];
        w.s12 = s_c[3][o] + s_c[3][o + 1] + s_c[3][o + kLW] + s_c[3][o + kLW + 1];
        q = quality_window_q32(w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sse[k] += __shfl_down(sse[k], o);
        q += __shfl_down(q, o);
    }
    const int wave = t >> 6;
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_sse[wave][k] = sse[k];
        s_q[wave] = q;
    }
    __syncthreads();
    if (t < 5) {
        uint64_t v = 0;
        for (int w = 0; w < 4; ++w) v += t < 4 ? (uint64_t)s_sse[w][t] : (uint64_t)s_q[w];
        partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 5 + t] = v;
    }
}

__global__ __launch_bounds__(256) void k_quality_fold(const uint64_t* __restrict__ partials, int tiles, QualityGeom g,
                                                      QualityFrame* __restrict__ results)
{
    __shared__ unsigned long long s_v[4][5];
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    const uint64_t* p = partials + (size_t)blockIdx.x * tiles * 5;
    for (int i = threadIdx.x; i < tiles; i += 256)
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += p[(size_t)i * 5 + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += __shfl_down(v[k], o);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) s_v[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        QualityFrame r;
        for (int k = 0; k < 5; ++k) {
            const unsigned long long sum = s_v[0][k] + s_v[1][k] + s_v[2][k] + s_v[3][k];
            if (k < 4)
                r.sse[k] = sum;
            else
                r.ssim_q32 = (int64_t)sum;
        }
        r.windows = (uint32_t)(g.full_x - 1) * (uint32_t)(g.full_y - 1);
        r.pixels = (uint32_t)g.W * (uint32_t)g.H;
        results[blockIdx.x] = r;
    }
}

}  // namespace

hipError_t quality_launch(const uint8_t* a, size_t a_pitch, size_t a_stride, const uint8_t* b, size_t b_pitch,
                          size_t b_stride, int n, const QualityGeom& g, uint64_t* partials, QualityFrame* results,
                          hipStream_t st)
{
    const int aligned = a_pitch % 4 == 0 && b_pitch % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 3) == 0 &&
                        (n <= 1 || (a_stride % 4 == 0 && b_stride % 4 == 0));
    const int tiles = g.tiles_x * g.tiles_y;
    hipLaunchKernelGGL(k_quality_tile, dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, st, a, a_pitch, a_stride, b,
                       b_pitch, b_stride, g, partials, aligned);
    hipLaunchKernelGGL(k_quality_fold, dim3((unsigned)n), dim3(256), 0, st, partials, tiles, g, results);
    return hipGetLastError();
}

}  // namespace dvc
