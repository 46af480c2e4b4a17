// jpegd_kernels.hip — baseline-JPEG decoder for gfx950 (wave64): what the
// reference's cap.read() (frame_differencing.py:86-87; motion_compression_opt.py:
// 66, 142-143) does with a Motion-JPEG sample, on the GPU. DESIGN.md
// "Motion-JPEG decoder" is the normative text of the arithmetic.
//
//   k_jpegd_count  RSTn markers in each chunk of every frame
//   k_jpegd_index  their positions, in order; a wrong count damages the frame
//   k_jpegd_huff   one lane per restart segment: Huffman symbols -> int16 levels
//   k_jpegd_idct   dequantise, integer IDCT in LDS -> Y, Cb, Cr planes (chroma at its coded size)
//   k_jpegd_out    fancy chroma upsampling, YCbCr -> BGR (or the luma plane) -> the caller's rows
// k_jpegd_idct and k_jpegd_out are instantiated per layout (JpegdLayout): one
// component, 4:2:0, and a camera handle's 4:2:2 and 4:4:4.
//   k_jpegd_err    the batch's first damaged frame -> the handle's sticky word
//
// All integer-exact; every store is an ordinary vector store.
#include <algorithm>

#include "jpegd_kernels.h"

namespace dvc {

namespace {

constexpr int kHuffMaxLanes = 16;       // the most decoding lanes of a k_jpegd_huff workgroup (one wave)
constexpr long long kHuffWaves = 2048;   // workgroups to aim for: two waves on each of the 1024 SIMDs

// A stream's layout, the template parameter of k_jpegd_idct and k_jpegd_out.
enum JpegdLayout { kLayGray = 0, kLay420 = 1, kLay422 = 2, kLay444 = 3 };

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// Exclusive prefix of v over the 256 threads; *total = their sum. s_w: 4 words.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w, uint32_t* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v, lane);
    __syncthreads();
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t x = s_w[w];
        if (w < wave) base += x;
        tot += x;
    }
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ bool is_rst(const uint8_t* d, uint32_t i, uint32_t size)
{
    return d[i] == 0xffu && i + 1 < size && (d[i + 1] & 0xf8u) == 0xd0u;
}

// ---- k_jpegd_count, k_jpegd_index ---------------------------------------------------
// Entropy data holds 0xFF only in front of 0x00 or a marker, so "0xFF then
// 0xD0..0xD7" is exactly a restart marker. A frame's bytes are split into
// kJpegdChunks equal chunks, a workgroup each: k_jpegd_count counts a chunk's
// markers; k_jpegd_index sums the counts in front of its chunk, then walks the
// chunk 256 bytes at a time and a block scan gives every marker its index.
// Unless a frame holds exactly nseg - 1 markers it is damaged and nothing is
// written for it.
struct ChunkRange {
    const uint8_t* d;
    uint32_t size, lo, hi;
    bool fits;
};

__device__ __forceinline__ ChunkRange chunk_range(const uint8_t* data, size_t stride, const uint32_t* sizes, int n)
{
    ChunkRange r;
    const int f = blockIdx.y;
    r.size = sizes[f];
    r.fits = n <= 1 || (size_t)r.size <= stride;   // a frame may not run into the next one's bytes
    r.d = data + (size_t)f * stride;
    const uint32_t part = r.fits ? (r.size + kJpegdChunks - 1u) / kJpegdChunks : 0u;
    r.lo = min(blockIdx.x * part, r.size);
    r.hi = min(r.lo + part, r.size);
    return r;
}

__global__ __launch_bounds__(256) void k_jpegd_count(const uint8_t* __restrict__ data, size_t stride,
                                                     const uint32_t* __restrict__ sizes, int n,
                                                     uint32_t* __restrict__ chunkcnt)
{
    __shared__ uint32_t s_w[4];
    const ChunkRange r = chunk_range(data, stride, sizes, n);
    uint32_t cnt = 0;
    for (uint32_t i = r.lo + threadIdx.x; i < r.hi; i += 256) cnt += is_rst(r.d, i, r.size);
    uint32_t total;
    (void)block_excl_scan(cnt, s_w, &total);
    if (threadIdx.x == 0) chunkcnt[blockIdx.y * kJpegdChunks + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_jpegd_index(const uint8_t* __restrict__ data, size_t stride,
                                                     const uint32_t* __restrict__ sizes, int n, JpegdGeom g,
                                                     const uint32_t* __restrict__ chunkcnt,
                                                     uint32_t* __restrict__ markpos, int32_t* __restrict__ status)
{
    __shared__ uint32_t s_w[4];
    const int f = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
    const ChunkRange r = chunk_range(data, stride, sizes, n);
    uint32_t before = 0, total = 0, mine = 0;
    for (int j = 0; j < kJpegdChunks; ++j) {
        const uint32_t v = chunkcnt[f * kJpegdChunks + j];
        if (j < c) before += v;
        if (j == c) mine = v;
        total += v;
    }
    const bool ok = r.fits && r.size > 0 && total == (uint32_t)(g.nseg - 1);
    if (c == 0 && t == 0) status[f] = ok ? 0 : kJpegdDamaged;
    if (!ok || mine == 0) return;   // (uniform over the workgroup)
    uint32_t* mp = markpos + (size_t)f * g.nseg;
    uint32_t k = before;
    for (uint32_t base = r.lo; base < r.hi; base += 256) {
        const uint32_t i = base + t;
        const bool hit = i < r.hi && is_rst(r.d, i, r.size);
        uint32_t tot;
        const uint32_t ex = block_excl_scan(hit ? 1u : 0u, s_w, &tot);
        if (hit) mp[k + ex] = i;   // k + ex < before + mine <= total = nseg - 1
        k += tot;
    }
}

// ---- k_jpegd_huff -----------------------------------------------------------------
// One lane per (frame, restart segment); `lanes` of them in a one-wave workgroup,
// whose threads first copy the tables into LDS. Lanes of a wave decode different
// data, so they diverge at every branch: the fewer share a wave, the less each
// waits for the others, and the launch picks one lane a wave until there are
// waves enough to fill the machine. CAMERA: a 4:2:2 or 4:4:4 stream (jpegd_segment_t);
// the layouts of a default handle run the instantiation they always ran.
template <bool CAMERA>
__global__ __launch_bounds__(64) void k_jpegd_huff(const uint8_t* __restrict__ data, size_t stride,
                                                   const uint32_t* __restrict__ sizes, int n, JpegdGeom g,
                                                   const JpegdTables* __restrict__ tab, int lanes,
                                                   const uint32_t* __restrict__ markpos, int16_t* __restrict__ coef,
                                                   int32_t* __restrict__ status)
{
    __shared__ JpegdTables s_tab;
    static_assert(sizeof(JpegdTables) % 4 == 0, "copied as dwords");
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(tab);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s_tab);
        for (int i = threadIdx.x; i < (int)(sizeof(JpegdTables) / 4); i += 64) dst[i] = src[i];
    }
    __syncthreads();
    if ((int)threadIdx.x >= lanes) return;
    const long long id = (long long)blockIdx.x * lanes + threadIdx.x;
    if (id >= (long long)n * g.nseg) return;
    const int f = (int)(id / g.nseg), s = (int)(id - (long long)f * g.nseg);
    if (status[f] != 0) return;
    const uint32_t size = sizes[f];
    const uint32_t* mp = markpos + (size_t)f * g.nseg;
    const uint32_t start = s ? mp[s - 1] + 2u : 0u;
    const uint32_t end = s < g.nseg - 1 ? mp[s] : size;
    if (start > end || end > size) {   // (the index kernel's positions are ordered and inside the frame)
        atomicMin(&status[f], kJpegdDamaged);
        return;
    }
    const int m0 = s * g.ri, nmcu = min(g.ri, g.mcus - m0);
    int16_t* dst = coef + ((size_t)f * g.mcus + m0) * g.bpm * 64;
    const int rc = jpegd_segment_t<CAMERA>(data + (size_t)f * stride + start, end - start, nmcu, g.bpm, &s_tab, dst);
    if (rc != 0) atomicMin(&status[f], rc);
}

// ---- k_jpegd_idct -----------------------------------------------------------------
// 256 threads = 4 waves, one work unit each: an MCU's six blocks (4:2:0), four
// consecutive blocks (one component), two MCUs' eight blocks (4:2:2) or eight
// consecutive scan-order blocks (4:4:4: block b is plane b % 3 of MCU b / 3, so
// an MCU may straddle waves and workgroups). A lane takes column i8 of block
// blk, then its row i8; the pass between them goes through LDS.
template <int L>
__global__ __launch_bounds__(256) void k_jpegd_idct(JpegdGeom g, const JpegdTables* __restrict__ tab,
                                                    const int16_t* __restrict__ coef, uint8_t* __restrict__ planes,
                                                    const int32_t* __restrict__ status)
{
    constexpr bool GRAY = L == kLayGray;
    constexpr int NB = L == kLayGray ? 4 : (L == kLay420 ? 6 : 8);
    __shared__ int32_t s_ws[4][NB * 64];
    __shared__ uint16_t s_q[3 * 64];
    const int f = blockIdx.y;
    if (status[f] != 0) return;   // (uniform over the workgroup)
    if (threadIdx.x < 192) s_q[threadIdx.x] = (&tab->q[0][0])[threadIdx.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wave;
    const int blk = lane >> 3, i8 = lane & 7;
    const int nblocks = g.mcus * g.bpm;
    const int b = unit * NB + blk;   // the frame's block in scan order
    const bool live = blk < NB && b < nblocks;
    __syncthreads();
    // 4:2:2, 4:4:4: the block's MCU and its place in it
    const int mcu = L == kLay422 ? b >> 2 : (L == kLay444 ? b / 3 : 0);
    const int jb = L == kLay422 ? b & 3 : (L == kLay444 ? b - 3 * mcu : 0);
    const int comp = GRAY ? 0 : (L == kLay420 ? (blk < 4 ? 0 : blk - 3) : (L == kLay422 ? (jb < 2 ? 0 : jb - 1) : jb));
    if (live) {
        const int16_t* lv = coef + ((size_t)f * nblocks + b) * 64;
        const uint16_t* q = s_q + comp * 64;
        int32_t in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = (int32_t)lv[r * 8 + i8] * (int32_t)q[r * 8 + i8];
        jpegd_idct8(in, o, 1024, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_ws[wave][blk * 64 + r * 8 + i8] = o[r];
    }
    __syncthreads();
    if (!live) return;
    int32_t in[8], o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = s_ws[wave][blk * 64 + i8 * 8 + c];
    jpegd_idct8(in, o, 131072, 18);
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c >> 2] |= (uint32_t)jpegd_clamp8((int32_t)((uint32_t)o[c] + 128u)) << (8 * (c & 3));
    uint8_t* fp = planes + (size_t)f * ((size_t)g.yw * g.yh + 2 * (size_t)g.cw * g.ch);
    uint8_t* dst;
    if (GRAY) {
        const int my = b / g.mcus_x, mx = b - my * g.mcus_x;
        dst = fp + (size_t)(my * 8 + i8) * g.yw + mx * 8;
    } else if (L == kLay420) {
        const int my = unit / g.mcus_x, mx = unit - my * g.mcus_x;
        if (blk < 4)
            dst = fp + (size_t)(my * 16 + (blk >> 1) * 8 + i8) * g.yw + mx * 16 + (blk & 1) * 8;
        else
            dst = fp + (size_t)g.yw * g.yh + (size_t)(blk - 4) * g.cw * g.ch + (size_t)(my * 8 + i8) * g.cw + mx * 8;
    } else {
        // mcu < g.mcus since b < nblocks: the row is inside the plane's mcus_y * 8 rows
        const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
        if (comp == 0)
            dst = fp + (size_t)(my * 8 + i8) * g.yw + (L == kLay422 ? mx * 16 + jb * 8 : mx * 8);
        else
            dst = fp + (size_t)g.yw * g.yh + (size_t)(comp - 1) * g.cw * g.ch + (size_t)(my * 8 + i8) * g.cw + mx * 8;
    }
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);   // plane pitches and block columns are multiples of 8
    d32[0] = w[0];
    d32[1] = w[1];
}

// ---- k_jpegd_out ------------------------------------------------------------------
// A lane per 4 output pixels x 2 rows (4:2:0: one chroma row): the upsampling
// rules from the chroma planes with their true neighbours, the colour conversion,
// and three dword stores a row where the rows are 4-byte aligned. 4:2:2 upsamples
// along the row only; 4:4:4 takes the chroma samples as they are (a dword of each
// plane a row: 3 B/px read, 3 B/px written). A damaged frame's slot is left
// untouched.
__device__ __forceinline__ void jpegd_store_bgr4(uint8_t* row, uint32_t yv, const int* cb, const int* cr, bool dwords,
                                                 int nx)
{
    uint8_t px[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) jpegd_bgr((int)((yv >> (8 * i)) & 0xffu), cb[i], cr[i], px + 3 * i);
    if (dwords) {
        uint32_t* d32 = reinterpret_cast<uint32_t*>(row);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            d32[w] = (uint32_t)px[4 * w] | (uint32_t)px[4 * w + 1] << 8 | (uint32_t)px[4 * w + 2] << 16 |
                     (uint32_t)px[4 * w + 3] << 24;
    } else {
        for (int i = 0; i < 3 * nx; ++i) row[i] = px[i];
    }
}

template <int L>
__global__ __launch_bounds__(256) void k_jpegd_out(JpegdGeom g, const uint8_t* __restrict__ planes,
                                                   uint8_t* __restrict__ out, size_t pitch, size_t fstride, int aligned,
                                                   const int32_t* __restrict__ status)
{
    const int f = blockIdx.z;
    if (status[f] != 0) return;
    const int j = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
    const int x0 = 4 * j, y0 = 2 * r;
    if (x0 >= g.W || y0 >= g.H) return;
    const uint8_t* fp = planes + (size_t)f * ((size_t)g.yw * g.yh + 2 * (size_t)g.cw * g.ch);
    uint8_t* o = out + (size_t)f * fstride;
    const int rows = min(2, g.H - y0), nx = min(4, g.W - x0);
    if constexpr (L == kLay444) {
        const size_t psz = (size_t)g.yw * g.yh;   // the three planes are one size
        for (int dy = 0; dy < rows; ++dy) {
            // x0 is a multiple of 4 below W <= yw, yw a multiple of 8: the dword is inside the row
            const uint8_t* src = fp + (size_t)(y0 + dy) * g.yw + x0;
            const uint32_t yv = *reinterpret_cast<const uint32_t*>(src);
            const uint32_t bv = *reinterpret_cast<const uint32_t*>(src + psz);
            const uint32_t rv = *reinterpret_cast<const uint32_t*>(src + 2 * psz);
            int cb[4], cr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                cb[i] = (int)((bv >> (8 * i)) & 0xffu);
                cr[i] = (int)((rv >> (8 * i)) & 0xffu);
            }
            jpegd_store_bgr4(o + (size_t)(y0 + dy) * pitch + 3 * (size_t)x0, yv, cb, cr, aligned && nx == 4, nx);
        }
        return;
    }
    if constexpr (L == kLay422) {
        const int dw = (g.W + 1) >> 1;
        const uint8_t* cp[2] = {fp + (size_t)g.yw * g.yh, fp + (size_t)g.yw * g.yh + (size_t)g.cw * g.ch};
        // chroma columns 2j - 1 .. 2j + 2, clamped to the real width (2j < dw since x0 < W)
        const int col[4] = {max(2 * j - 1, 0), 2 * j, min(2 * j + 1, dw - 1), min(2 * j + 2, dw - 1)};
        for (int dy = 0; dy < rows; ++dy) {
            int up[2][4];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint8_t* crow = cp[c] + (size_t)(y0 + dy) * g.cw;   // chroma rows are luma rows
                int p[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) p[i] = (int)crow[col[i]];
                if (dw <= 2) {
                    up[c][0] = up[c][1] = p[1];
                    up[c][2] = up[c][3] = p[2];
                } else {
                    up[c][0] = (3 * p[1] + p[0] + 1) >> 2;
                    up[c][1] = (3 * p[1] + p[2] + 2) >> 2;
                    up[c][2] = (3 * p[2] + p[1] + 1) >> 2;
                    up[c][3] = (3 * p[2] + p[3] + 2) >> 2;
                }
            }
            const uint32_t yv = *reinterpret_cast<const uint32_t*>(fp + (size_t)(y0 + dy) * g.yw + x0);
            jpegd_store_bgr4(o + (size_t)(y0 + dy) * pitch + 3 * (size_t)x0, yv, up[0], up[1], aligned && nx == 4, nx);
        }
        return;
    }
    constexpr bool GRAY = L == kLayGray;
    if (GRAY) {
        for (int dy = 0; dy < rows; ++dy) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(fp + (size_t)(y0 + dy) * g.yw + x0);
            uint8_t* row = o + (size_t)(y0 + dy) * pitch + x0;
            if (aligned && nx == 4) {
                *reinterpret_cast<uint32_t*>(row) = v;
            } else {
                for (int i = 0; i < nx; ++i) row[i] = (uint8_t)(v >> (8 * i));
            }
        }
        return;
    }
    const int dw = (g.W + 1) >> 1, dh = (g.H + 1) >> 1;
    const uint8_t* cp[2] = {fp + (size_t)g.yw * g.yh, fp + (size_t)g.yw * g.yh + (size_t)g.cw * g.ch};
    int up[2][2][4];   // [plane][row of the pair][pixel]
    if (dw <= 2) {
        for (int c = 0; c < 2; ++c)
            for (int dy = 0; dy < 2; ++dy)
                for (int i = 0; i < 4; ++i) up[c][dy][i] = cp[c][(size_t)r * g.cw + min((x0 + i) >> 1, dw - 1)];
    } else {
        const int col[4] = {max(2 * j - 1, 0), 2 * j, min(2 * j + 1, dw - 1), min(2 * j + 2, dw - 1)};
        const int ra = max(r - 1, 0), rb = min(r + 1, dh - 1);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            int st[4], sb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mid = 3 * (int)cp[c][(size_t)r * g.cw + col[i]];
                st[i] = mid + (int)cp[c][(size_t)ra * g.cw + col[i]];
                sb[i] = mid + (int)cp[c][(size_t)rb * g.cw + col[i]];
            }
            up[c][0][0] = (3 * st[1] + st[0] + 8) >> 4;
            up[c][0][1] = (3 * st[1] + st[2] + 7) >> 4;
            up[c][0][2] = (3 * st[2] + st[1] + 8) >> 4;
            up[c][0][3] = (3 * st[2] + st[3] + 7) >> 4;
            up[c][1][0] = (3 * sb[1] + sb[0] + 8) >> 4;
            up[c][1][1] = (3 * sb[1] + sb[2] + 7) >> 4;
            up[c][1][2] = (3 * sb[2] + sb[1] + 8) >> 4;
            up[c][1][3] = (3 * sb[2] + sb[3] + 7) >> 4;
        }
    }
    for (int dy = 0; dy < rows; ++dy) {
        const uint32_t yv = *reinterpret_cast<const uint32_t*>(fp + (size_t)(y0 + dy) * g.yw + x0);
        uint8_t px[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) jpegd_bgr((int)((yv >> (8 * i)) & 0xffu), up[0][dy][i], up[1][dy][i], px + 3 * i);
        uint8_t* row = o + (size_t)(y0 + dy) * pitch + 3 * (size_t)x0;
        if (aligned && nx == 4) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(row);
#pragma unroll
            for (int w = 0; w < 3; ++w)
                d32[w] = (uint32_t)px[4 * w] | (uint32_t)px[4 * w + 1] << 8 | (uint32_t)px[4 * w + 2] << 16 |
                         (uint32_t)px[4 * w + 3] << 24;
        } else {
            for (int i = 0; i < 3 * nx; ++i) row[i] = px[i];
        }
    }
}

// The batch's first damaged frame, kept until dvc_jpegd_sync reads it.
__global__ void k_jpegd_err(const int32_t* __restrict__ status, int n, int32_t* __restrict__ first_err)
{
    if (*first_err != 0) return;
    for (int f = 0; f < n; ++f)
        if (status[f] != 0) {
            *first_err = status[f];
            return;
        }
}

}  // namespace

hipError_t jpegd_launch(const uint8_t* data, size_t stride, const uint32_t* sizes, int n, const JpegdGeom& g,
                        const JpegdTables* tab, const JpegdBufs& b, uint8_t* out, size_t pitch, size_t fstride,
                        int32_t* status, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const size_t ncoef = (size_t)n * g.mcus * g.bpm * 64;
    hipError_t e = hipMemsetAsync(b.coef, 0, ncoef * sizeof(int16_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_jpegd_count, dim3(kJpegdChunks, (unsigned)n), dim3(256), 0, st, data, stride, sizes, n,
                       b.chunkcnt);
    hipLaunchKernelGGL(k_jpegd_index, dim3(kJpegdChunks, (unsigned)n), dim3(256), 0, st, data, stride, sizes, n, g,
                       b.chunkcnt, b.markpos, status);
    const long long segs = (long long)n * g.nseg;
    const int lanes = (int)std::min<long long>(kHuffMaxLanes, std::max<long long>(1, segs / kHuffWaves));
    if (g.bpm == 1 || g.bpm == 6)
        hipLaunchKernelGGL(k_jpegd_huff<false>, dim3((unsigned)((segs + lanes - 1) / lanes)), dim3(64), 0, st, data, stride,
                           sizes, n, g, tab, lanes, b.markpos, b.coef, status);
    else
        hipLaunchKernelGGL(k_jpegd_huff<true>, dim3((unsigned)((segs + lanes - 1) / lanes)), dim3(64), 0, st, data, stride,
                           sizes, n, g, tab, lanes, b.markpos, b.coef, status);
    const int aligned = pitch % 4 == 0 && ((uintptr_t)out & 3) == 0 && (n <= 1 || fstride % 4 == 0);
    const dim3 ogrid((unsigned)(((g.W + 3) / 4 + 63) / 64), (unsigned)(((g.H + 1) / 2 + 3) / 4), (unsigned)n);
    if (g.gray) {
        const int units = (g.mcus + 3) / 4;
        hipLaunchKernelGGL(k_jpegd_idct<kLayGray>, dim3((unsigned)((units + 3) / 4), (unsigned)n), dim3(256), 0, st, g,
                           tab, b.coef, b.planes, status);
        hipLaunchKernelGGL(k_jpegd_out<kLayGray>, ogrid, dim3(64, 4), 0, st, g, b.planes, out, pitch, fstride, aligned,
                           status);
    } else if (g.hs == 2 && g.vs == 2) {
        hipLaunchKernelGGL(k_jpegd_idct<kLay420>, dim3((unsigned)((g.mcus + 3) / 4), (unsigned)n), dim3(256), 0, st, g,
                           tab, b.coef, b.planes, status);
        hipLaunchKernelGGL(k_jpegd_out<kLay420>, ogrid, dim3(64, 4), 0, st, g, b.planes, out, pitch, fstride, aligned,
                           status);
    } else if (g.hs == 2 && g.vs == 1) {   // two MCUs a wave
        const int units = (g.mcus + 1) / 2;
        hipLaunchKernelGGL(k_jpegd_idct<kLay422>, dim3((unsigned)((units + 3) / 4), (unsigned)n), dim3(256), 0, st, g,
                           tab, b.coef, b.planes, status);
        hipLaunchKernelGGL(k_jpegd_out<kLay422>, ogrid, dim3(64, 4), 0, st, g, b.planes, out, pitch, fstride, aligned,
                           status);
    } else if (g.hs == 1 && g.vs == 1) {   // eight scan-order blocks a wave
        const int units = (3 * g.mcus + 7) / 8;
        hipLaunchKernelGGL(k_jpegd_idct<kLay444>, dim3((unsigned)((units + 3) / 4), (unsigned)n), dim3(256), 0, st, g,
                           tab, b.coef, b.planes, status);
        hipLaunchKernelGGL(k_jpegd_out<kLay444>, ogrid, dim3(64, 4), 0, st, g, b.planes, out, pitch, fstride, aligned,
                           status);
    } else {
        return hipErrorInvalidValue;   // (the header parser accepts no other layout)
    }
    hipLaunchKernelGGL(k_jpegd_err, dim3(1), dim3(1), 0, st, status, n, b.first_err);
    return hipGetLastError();
}

}  // namespace dvc
