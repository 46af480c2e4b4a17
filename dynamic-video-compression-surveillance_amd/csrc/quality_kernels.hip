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
//   k_quality_class, k_quality_tile_regions, k_quality_fold_regions
//                    the same figures split by a mask into the kept and the static
//                    region ("Kept and static regions"), further down
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

// ---- kept and static regions ------------------------------------------------------

constexpr int kClassStrip = 1024;   // columns of one block row a workgroup classifies
// dwords of four column ORs: the strip, the rest of the blocks it cuts at either end, alignment
constexpr int kClassQuads = kClassStrip / 4 + kQualityMaxBlock / 2 + 2;

// Mask frames -> class bits (quality_kernels.h). Grid (strips, block rows, n).
// A lane ORs four columns down the block row's pixel rows, a dword a row where
// rows are 4-byte aligned and bytes with bounds otherwise, from the first
// column of the strip's first block to the last column of its last block; a
// lane per block ORs the block's columns and applies the block rule; a ballot
// per 64 columns makes the words.
__global__ __launch_bounds__(256) void k_quality_class(const uint8_t* __restrict__ mask, size_t pm, size_t sm, int W, int H,
                                                       int B, uint32_t magic, int partial_static, int aligned,
                                                       uint32_t* __restrict__ cls)
{
    __shared__ uint32_t s_or[kClassQuads];
    __shared__ uint8_t s_static[kClassStrip + 2];
    const int t = threadIdx.x, by = blockIdx.y, cw = (W + 31) >> 5;
    const int s0 = blockIdx.x * kClassStrip, s1 = min(s0 + kClassStrip, W);
    const int y0 = by * B, y1 = min(y0 + B, H);
    const int b0 = s0 / B, b1 = (s1 - 1) / B;   // the blocks that hold a column of the strip
    const int e0 = (b0 * B) & ~3, e1 = min((b1 + 1) * B, W);
    const uint8_t* fm = mask + (size_t)blockIdx.z * sm;

    for (int q = t; 4 * q < e1 - e0; q += 256) {
        const int x = e0 + 4 * q;
        uint32_t v = 0;
        if (aligned && x + 4 <= W) {
            for (int y = y0; y < y1; ++y) v |= *reinterpret_cast<const uint32_t*>(fm + (size_t)y * pm + x);
        } else {
            for (int y = y0; y < y1; ++y)
                for (int i = 0; i < 4 && x + i < W; ++i) v |= (uint32_t)fm[(size_t)y * pm + x + i] << 8 * i;
        }
        s_or[q] = v;
    }
    __syncthreads();
    for (int j = t; j <= b1 - b0; j += 256) {
        const int x0 = (b0 + j) * B, x1 = min(x0 + B, W);
        uint32_t any = 0;
        for (int x = x0 - e0; x < x1 - e0; ++x) any |= (s_or[x >> 2] >> 8 * (x & 3)) & 255;
        s_static[j] = (uint8_t)quality_block_static(any, x0 + B > W || y0 + B > H, partial_static);
    }
    __syncthreads();
    uint32_t* row = cls + ((size_t)blockIdx.z * gridDim.y + by) * cw;
    for (int p = s0; p < s1; p += 256) {   // (the same trips in every lane: the ballot needs them all)
        const int x = p + t;
        const unsigned long long bits = __ballot(x < W && s_static[quality_block_of((uint32_t)x, magic) - b0]);
        const int lane = t & 63, word = ((p + (t & ~63)) >> 5) + lane;
        if (lane < 2 && word < cw) row[word] = (uint32_t)(bits >> 32 * lane);
    }
}

// The class bits of the pixels of cell (cx, cy), which holds a pixel: bit
// 4 r + i is set where pixel (4 cx + i, 4 cy + r) is static. Its rows may lie in
// two or more block rows; rows below the frame give 0, and columns right of it
// are 0 in cls.
__device__ __forceinline__ uint32_t cell_bits(const uint32_t* __restrict__ cls, int cw, int B, uint32_t magic, int cx,
                                              int cy, int H)
{
    const int x0 = 4 * cx, y0 = 4 * cy, sh = x0 & 31;
    const int by = (int)quality_block_of((uint32_t)y0, magic);
    int rem = y0 - by * B;
    const uint32_t* p = cls + (size_t)by * cw + (x0 >> 5);
    uint32_t nib = (*p >> sh) & 15, m = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (y0 + r < H) m |= nib << 4 * r;
        if (r < 3 && ++rem == B && y0 + r + 1 < H) {
            rem = 0;
            p += cw;
            nib = (*p >> sh) & 15;
        }
    }
    return m;
}

// The squared errors of the pixels of cell (cx, cy) whose bit is set in m (all inside the frame).
__device__ void cell_masked(const uint8_t* __restrict__ fa, size_t pa, const uint8_t* __restrict__ fb, size_t pb, int cx,
                            int cy, uint32_t m, uint32_t (&sse)[4])
{
    for (int r = 0; r < 4; ++r)
        for (int i = 0; i < 4; ++i)
            if ((m >> (4 * r + i)) & 1) {
                const uint8_t* p = fa + (size_t)(4 * cy + r) * pa + 3 * (size_t)(4 * cx + i);
                const uint8_t* q = fb + (size_t)(4 * cy + r) * pb + 3 * (size_t)(4 * cx + i);
                quality_px_sse(p[0], p[1], p[2], q[0], q[1], q[2], sse);
            }
}

// A lane's counts, packed for one reduction: pixels kept and static (a tile has
// 4096), windows kept, static and mixed (a tile starts 256).
constexpr int kCntStatic = 13, kCntWindows = 26, kCntWindowBits = 9;

// k_quality_tile with a class per pixel: a cell that holds one class gives its
// squared errors to that class as they are, a cell that holds both (block
// edges inside cells) reads its static pixels again; every cell, the halo's
// too, leaves which classes it holds in LDS beside its sums, and a window's
// class follows from its four cells. Sixteen partials per tile and frame:
// sse[2][4], pixels[2], ssim_q32[3], windows[3].
__global__ __launch_bounds__(256) void k_quality_tile_regions(const uint8_t* __restrict__ a, size_t pa, size_t sa,
                                                              const uint8_t* __restrict__ b, size_t pb, size_t sb,
                                                              const uint32_t* __restrict__ cls, size_t cls_frame, int B,
                                                              uint32_t magic, QualityGeom g, uint64_t* __restrict__ partials, int aligned)
{
    __shared__ int s_c[4][kLH * kLW];
    __shared__ uint8_t s_has[kLH * kLW];
    __shared__ uint32_t s_sse[4][8];
    __shared__ long long s_q[4][3];
    __shared__ unsigned long long s_n[4];
    const int t = threadIdx.x, lx = t & (kQualityTileCX - 1), ly = t / kQualityTileCX;
    const int ty = blockIdx.x / g.tiles_x, tx = blockIdx.x - ty * g.tiles_x;
    const int cx0 = tx * kQualityTileCX, cy0 = ty * kQualityTileCY;
    const uint8_t* fa = a + (size_t)blockIdx.y * sa;
    const uint8_t* fb = b + (size_t)blockIdx.y * sb;
    const uint32_t* fc = cls + (size_t)blockIdx.y * cls_frame;
    const int cw = (g.W + 31) >> 5;

    uint32_t sse[4] = {0, 0, 0, 0}, sst[4] = {0, 0, 0, 0};   // all pixels; the static ones
    QualityCell c{0, 0, 0, 0};
    uint32_t has = 0;
    unsigned long long cnt = 0;
    const int cx = cx0 + lx, cy = cy0 + ly;
    if (cx < g.cells_x && cy < g.cells_y) {
        cell(fa, pa, fb, pb, cx, cy, g.W, g.H, aligned, sse, c);
        const uint32_t inside = quality_cell_inside(4 * cx, 4 * cy, g.W, g.H);
        const uint32_t m = cell_bits(fc, cw, B, magic, cx, cy, g.H) & inside;
        has = quality_cell_has(m, inside);
        if (has == kQualityHasStatic) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sst[k] = sse[k];
        } else if (has != kQualityHasKept) {
            cell_masked(fa, pa, fb, pb, cx, cy, m, sst);
        }
        cnt = (unsigned long long)__popc(inside & ~m) | (unsigned long long)__popc(m) << kCntStatic;
    }
    s_c[0][ly * kLW + lx] = c.s1;
    s_c[1][ly * kLW + lx] = c.s2;
    s_c[2][ly * kLW + lx] = c.ss;
    s_c[3][ly * kLW + lx] = c.s12;
    s_has[ly * kLW + lx] = (uint8_t)has;
    if (t < kHalo) {
        const int hx = t < kQualityTileCY ? kQualityTileCX : t - kQualityTileCY;
        const int hy = t < kQualityTileCY ? t : kQualityTileCY;
        uint32_t unused[4] = {0, 0, 0, 0}, hh = 0;
        QualityCell h{0, 0, 0, 0};
        if (cx0 + hx < g.full_x && cy0 + hy < g.full_y) {
            cell(fa, pa, fb, pb, cx0 + hx, cy0 + hy, g.W, g.H, aligned, unused, h);
            hh = quality_cell_has(cell_bits(fc, cw, B, magic, cx0 + hx, cy0 + hy, g.H), 0xffffu);
        }
        s_c[0][hy * kLW + hx] = h.s1;
        s_c[1][hy * kLW + hx] = h.s2;
        s_c[2][hy * kLW + hx] = h.ss;
        s_c[3][hy * kLW + hx] = h.s12;
        s_has[hy * kLW + hx] = (uint8_t)hh;
    }
    __syncthreads();

    long long q[3] = {0, 0, 0};
    if (cx + 1 < g.full_x && cy + 1 < g.full_y) {
        const int o = ly * kLW + lx;
        QualityCell w;
        w.s1 = s_c[0][o] + s_c[0][o + 1] + s_c[0][o + kLW] + s_c[0][o + kLW + 1];
        w.s2 = s_c[1][o] + s_c[1][o + 1] + s_c[1][o + kLW] + s_c[1][o + kLW + 1];
        w.ss = s_c[2][o] + s_c[2][o + 1] + s_c[2][o + kLW] + s_c[2][o + kLW + 1];
        w.s12 = s_c[3][o] + s_c[3][o + 1] + s_c[3][o + kLW] + s_c[3][o + kLW + 1];
        const long long v = quality_window_q32(w);
        const int k = quality_window_class((uint32_t)(s_has[o] | s_has[o + 1] | s_has[o + kLW] | s_has[o + kLW + 1]));
#pragma unroll
        for (int j = 0; j < 3; ++j) q[j] = k == j ? v : 0;
        cnt += 1ull << (kCntWindows + kCntWindowBits * k);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sse[k] += __shfl_down(sse[k], o);
            sst[k] += __shfl_down(sst[k], o);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) q[j] += __shfl_down(q[j], o);
        cnt += __shfl_down(cnt, o);
    }
    const int wave = t >> 6;
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s_sse[wave][k] = sse[k] - sst[k];
            s_sse[wave][4 + k] = sst[k];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) s_q[wave][j] = q[j];
        s_n[wave] = cnt;
    }
    __syncthreads();
    if (t < kQualityRegionParts) {
        uint64_t v = 0;
        if (t < 8) {
            for (int w = 0; w < 4; ++w) v += s_sse[w][t];
        } else if (t >= 10 && t < 13) {
            for (int w = 0; w < 4; ++w) v += (uint64_t)s_q[w][t - 10];
        } else {
            const unsigned long long n = s_n[0] + s_n[1] + s_n[2] + s_n[3];
            v = t == 8    ? n & ((1u << kCntStatic) - 1)
                : t == 9 ? (n >> kCntStatic) & ((1u << kCntStatic) - 1)
                         : (n >> (kCntWindows + kCntWindowBits * (t - 13))) & ((1u << kCntWindowBits) - 1);
        }
        partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kQualityRegionParts + t] = v;
    }
}

// One workgroup per frame: lane t adds the partials 2 (t % 8) and 2 (t % 8) + 1 of
// every 32nd tile, 16 bytes a load, consecutive lanes on consecutive words.
__global__ __launch_bounds__(256) void k_quality_fold_regions(const uint64_t* __restrict__ partials, int tiles,
                                                              QualityRegions* __restrict__ results)
{
    static_assert(kQualityRegionParts == 16, "eight lanes a tile, two partials a lane");
    __shared__ unsigned long long s_v[4][kQualityRegionParts];
    const int k = threadIdx.x & 7;
    const ulonglong2* p =
        reinterpret_cast<const ulonglong2*>(partials + (size_t)blockIdx.x * tiles * kQualityRegionParts);
    unsigned long long v0 = 0, v1 = 0;
#pragma unroll 4
    for (int i = threadIdx.x >> 3; i < tiles; i += 32) {
        const ulonglong2 w = p[(size_t)i * 8 + k];
        v0 += w.x;
        v1 += w.y;
    }
#pragma unroll
    for (int o = 32; o >= 8; o >>= 1) {
        v0 += __shfl_down(v0, o);
        v1 += __shfl_down(v1, o);
    }
    if ((threadIdx.x & 63) < 8) {
        s_v[threadIdx.x >> 6][2 * k] = v0;
        s_v[threadIdx.x >> 6][2 * k + 1] = v1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s[kQualityRegionParts];
        for (int j = 0; j < kQualityRegionParts; ++j) s[j] = s_v[0][j] + s_v[1][j] + s_v[2][j] + s_v[3][j];
        QualityRegions r;
        for (int j = 0; j < 8; ++j) r.sse[j >> 2][j & 3] = s[j];
        for (int j = 0; j < 2; ++j) r.pixels[j] = (uint32_t)s[8 + j];
        for (int j = 0; j < 3; ++j) {
            r.ssim_q32[j] = (int64_t)s[10 + j];
            r.windows[j] = (uint32_t)s[13 + j];
        }
        r.reserved = 0;
        results[blockIdx.x] = r;
    }
}

}  // namespace

hipError_t quality_launch_regions(const uint8_t* a, size_t a_pitch, size_t a_stride, const uint8_t* b, size_t b_pitch,
                                  size_t b_stride, const uint8_t* mask, size_t m_pitch, size_t m_stride, int block,
                                  int partial_static, int n, const QualityGeom& g, uint32_t* cls, uint64_t* partials,
                                  QualityRegions* results, hipStream_t st)
{
    const int aligned = a_pitch % 4 == 0 && b_pitch % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 3) == 0 &&
                        (n <= 1 || (a_stride % 4 == 0 && b_stride % 4 == 0));
    const int m_aligned = m_pitch % 4 == 0 && ((uintptr_t)mask & 3) == 0 && (n <= 1 || m_stride % 4 == 0);
    const int tiles = g.tiles_x * g.tiles_y, brows = (g.H + block - 1) / block;
    const uint32_t magic = quality_block_magic(block);
    hipLaunchKernelGGL(k_quality_class, dim3((unsigned)((g.W + kClassStrip - 1) / kClassStrip), (unsigned)brows, (unsigned)n),
                       dim3(256), 0, st, mask, m_pitch, m_stride, g.W, g.H, block, magic, partial_static, m_aligned, cls);
    hipLaunchKernelGGL(k_quality_tile_regions, dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, st, a, a_pitch, a_stride,
                       b, b_pitch, b_stride, cls, quality_class_words(g.W, g.H, block), block, magic, g, partials, aligned);
    hipLaunchKernelGGL(k_quality_fold_regions, dim3((unsigned)n), dim3(256), 0, st, partials, tiles, results);
    return hipGetLastError();
}

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
