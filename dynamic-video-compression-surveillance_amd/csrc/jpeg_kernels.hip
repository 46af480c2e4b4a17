// jpeg_kernels.hip — baseline-JPEG encoder for gfx950 (wave64): the frames the
// reference hands to cv2.VideoWriter.write (frame_differencing.py:112,131;
// motion_compression_opt.py:99-100,185) become JFIF entropy data on the GPU.
// DESIGN.md "Motion-JPEG stream" is the normative text of the arithmetic.
//
//   k_jpeg_dct     BGR / gray -> YCbCr, 4:2:0, integer DCT, quantise, zigzag
//   k_jpeg_rate_bits, k_jpeg_rate_step, k_jpeg_quant  rate handles: coefficients kept
//                  unquantised, a search for the group's quality over their exact
//                  coded size, then the levels at that quality (jpeg_rate_core.h)
//   k_jpeg_bits    per-block code lengths, bit offsets along each restart segment
//   k_jpeg_pack    codes OR-ed into an LDS bit buffer, 0xFF stuffing -> scratch
//   k_jpeg_gather  segments + RST markers + EOI -> the frame's output slot
//   k_jpeg_stream_offsets, k_jpeg_stream_gather  the same segments as complete samples
//                  back to back (dvc_jpeg_encode_stream): offsets behind a device carry,
//                  then header, prefix, segments and markers straight to their places
//
// All are integer-exact; every store is an ordinary vector store.
#include "jpeg_kernels.h"

namespace dvc {

namespace {

// M[k][n] = round(8192 * a(k) * cos((2n+1) k pi / 16)), n < 4 (M[k][7-n] = +-M[k][n])
static __device__ const int kDctM[8][4] = {
    {2896, 2896, 2896, 2896},  {4017, 3406, 2276, 799},   {3784, 1567, -1567, -3784}, {3406, -799, -4017, -2276},
    {2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406}, {1567, -3784, 3784, -1567}, {799, -2276, 3406, -4017}};

// out[k] = (sum_n M[k][n] x[n] + rnd) >> sh: full integer sums, the even / odd
// symmetry of M used (exact).
__device__ __forceinline__ void dct8(const int x[8], int out[8], int rnd, int sh)
{
    int s[4], d[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        s[n] = x[n] + x[7 - n];
        d[n] = x[n] - x[7 - n];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int* v = (k & 1) ? d : s;
        int acc = rnd;
#pragma unroll
        for (int n = 0; n < 4; ++n) acc += kDctM[k][n] * v[n];
        out[k] = acc >> sh;
    }
}

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
    __syncthreads();   // the previous round's readers are done with s_w
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

// ---- k_jpeg_dct -------------------------------------------------------------------
// 256 threads = 4 waves, one work unit each: a 16x16 MCU (colour, 6 blocks) or
// four 8x8 blocks side by side (gray). A lane loads 4 pixels of one row (three
// aligned dwords of BGR, or one of gray), clamped to the frame edge.
// RAW (rate handles): the coefficients themselves, not their levels, go out.
template <bool GRAY, bool RAW>
__global__ __launch_bounds__(256) void k_jpeg_dct(const uint8_t* __restrict__ frames, size_t pitch, size_t fstride,
                                                  JpegGeom g, const JpegTables* __restrict__ tab,
                                                  int16_t* __restrict__ levels, int aligned)
{
    constexpr int NB = GRAY ? 4 : 6;
    constexpr int NPX = GRAY ? 256 : 768;
    __shared__ int16_t s_px[4][NPX];        // gray: 8 rows x 32; colour: Y, Cb, Cr planes of 16 x 16
    __shared__ int s_r[4][NB * 64];         // after the row pass
    __shared__ int16_t s_lv[4][NB * 64];    // levels, zigzag order
    __shared__ uint16_t s_q[128];
    __shared__ uint8_t s_zpos[64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (!RAW && threadIdx.x < 128) s_q[threadIdx.x] = (&tab->q[0][0])[threadIdx.x];
    if (threadIdx.x < 64) s_zpos[threadIdx.x] = tab->zpos[threadIdx.x];
    const int units = g.units_x * g.nseg;
    int unit = blockIdx.x * 4 + wave;
    const bool live = unit < units;
    if (!live) unit = units - 1;
    const int uy = unit / g.units_x, ux = unit - uy * g.units_x;
    const uint8_t* f = frames + (size_t)blockIdx.y * fstride;
    int16_t* px = s_px[wave];

    if (GRAY) {
        const int r = lane >> 3, run = lane & 7;
        const int x0 = ux * 32 + run * 4, y = min(uy * 8 + r, g.H - 1);
        const uint8_t* row = f + (size_t)y * pitch;
        uint32_t v;
        if (aligned && x0 + 4 <= g.W) {
            v = *reinterpret_cast<const uint32_t*>(row + x0);
        } else {
            v = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) v |= (uint32_t)row[min(x0 + i, g.W - 1)] << (8 * i);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) px[r * 32 + run * 4 + i] = (int16_t)((v >> (8 * i)) & 0xff);
    } else {
        const int r = lane >> 2, run = lane & 3;
        const int x0 = ux * 16 + run * 4, y = min(uy * 16 + r, g.H - 1);
        const uint8_t* row = f + (size_t)y * pitch;
        uint8_t c[12];
        if (aligned && x0 + 4 <= g.W) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(row + 3 * (size_t)x0);
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const uint32_t v = p[w];
#pragma unroll
                for (int i = 0; i < 4; ++i) c[4 * w + i] = (uint8_t)(v >> (8 * i));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint8_t* q = row + 3 * (size_t)min(x0 + i, g.W - 1);
                c[3 * i] = q[0];
                c[3 * i + 1] = q[1];
                c[3 * i + 2] = q[2];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int B = c[3 * i], G = c[3 * i + 1], R = c[3 * i + 2];
            const int o = r * 16 + run * 4 + i;
            px[o] = (int16_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
            px[256 + o] = (int16_t)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
            px[512 + o] = (int16_t)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
        }
    }
    __syncthreads();

    const int blk = lane >> 3, i8 = lane & 7;   // row pass: row i8 of block blk; column pass: its column i8
    if (blk < NB) {
        int x[8], o[8];
        if (GRAY) {
#pragma unroll
            for (int n = 0; n < 8; ++n) x[n] = px[i8 * 32 + blk * 8 + n] - 128;
        } else if (blk < 4) {
            const int base = ((blk >> 1) * 8 + i8) * 16 + (blk & 1) * 8;
#pragma unroll
            for (int n = 0; n < 8; ++n) x[n] = px[base + n] - 128;
        } else {
            const int16_t* p = px + 256 * (blk - 3) + 2 * i8 * 16;
#pragma unroll
            for (int n = 0; n < 8; ++n) x[n] = ((p[2 * n] + p[2 * n + 1] + p[16 + 2 * n] + p[17 + 2 * n] + 2) >> 2) - 128;
        }
        dct8(x, o, 512, 10);
#pragma unroll
        for (int k = 0; k < 8; ++k) s_r[wave][blk * 64 + i8 * 8 + k] = o[k];
    }
    __syncthreads();
    if (blk < NB) {
        int x[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) x[y] = s_r[wave][blk * 64 + y * 8 + i8];
        dct8(x, o, 32768, 16);
        const uint16_t* q = s_q + ((!GRAY && blk >= 4) ? 64 : 0);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int nat = v * 8 + i8;
            if (RAW) {   // |F| < 2^15: rate_coef_bound, run by tools/jpeg_rate_host_check.cc
                s_lv[wave][blk * 64 + s_zpos[nat]] = (int16_t)o[v];
                continue;
            }
            const int Q = q[nat], F = o[v];
            int l = (int)((uint32_t)(abs(F) + (Q >> 1)) / (uint32_t)Q);
            if (nat) l = min(l, 1023);
            s_lv[wave][blk * 64 + s_zpos[nat]] = (int16_t)(F < 0 ? -l : l);
        }
    }
    __syncthreads();
    if (!live) return;
    const size_t fblocks = (size_t)g.nseg * g.bps;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(s_lv[wave]);
    if (GRAY) {
        const int nv = min(4, g.mcus_x - ux * 4);
        uint32_t* dst = reinterpret_cast<uint32_t*>(levels + ((size_t)blockIdx.y * fblocks + (size_t)uy * g.bps + ux * 4) * 64);
        for (int i = lane; i < nv * 32; i += 64) dst[i] = src[i];
    } else {
        uint32_t* dst = reinterpret_cast<uint32_t*>(levels + ((size_t)blockIdx.y * fblocks + (size_t)uy * g.bps + ux * 6) * 64);
#pragma unroll
        for (int i = 0; i < 3; ++i) dst[lane + 64 * i] = src[lane + 64 * i];
    }
}

// ---- entropy coding: what one lane (one zigzag coefficient) emits ---------------------
// The symbol: the DC size on lane 0, (run & 15) << 4 | size with run >> 4 ZRLs
// in front on a lane with a non-zero level, EOB (0x00) on lane 63 behind
// trailing zeros, nothing (-1) elsewhere. Shared by the histogram and the coders.
struct LaneSym {
    int sym;    // -1: nothing
    int val;    // the value whose `size` magnitude bits follow the code
    int size;
    int nzrl;   // ZRL codes in front (runs of 16 zeros)
};

__device__ __forceinline__ LaneSym lane_symbol(int lv, int lane, int pred)
{
    LaneSym s{-1, lv, 0, 0};
    const unsigned long long nz = __ballot(lv != 0 && lane > 0) | 1ull;   // bit 0: the DC ends no run
    if (lane == 0) {
        s.val = max(-2047, min(2047, lv - pred));
        s.size = 32 - __clz(abs(s.val));
        s.sym = s.size;
    } else if (lv != 0) {
        const unsigned long long below = nz & ((1ull << lane) - 1ull);
        const int run = lane - (63 - __clzll((long long)below)) - 1;
        s.nzrl = run >> 4;
        s.size = 32 - __clz(abs(lv));
        s.sym = ((run & 15) << 4) | s.size;
    } else if (lane == 63) {   // trailing zeros: EOB
        s.sym = 0;
    }
    return s;
}

struct LaneCode {
    uint32_t code;   // Huffman code followed by the magnitude bits
    int n;           // their length (<= 27)
    int nzrl;        // ZRL codes in front (runs of 16 zeros)
};

__device__ __forceinline__ LaneCode lane_code(int lv, int lane, int pred, const uint32_t* s_dc, const uint32_t* s_ac)
{
    const LaneSym s = lane_symbol(lv, lane, pred);
    LaneCode c{0u, 0, s.nzrl};
    if (s.sym < 0) return c;
    const uint32_t e = lane == 0 ? s_dc[s.sym] : s_ac[s.sym];
    const uint32_t mag = (uint32_t)(s.val < 0 ? s.val - 1 : s.val) & ((1u << s.size) - 1u);
    c.code = ((e & 0xffffu) << s.size) | mag;
    c.n = (int)(e >> 16) + s.size;
    return c;
}

// The table class of block j of a segment: 0 luma (and gray), 1 Cb and Cr.
__device__ __forceinline__ int block_class(int j, int gray) { return !gray && j % 6 >= 4; }

// The DC predictor of block j of a segment: the previous block of its component.
__device__ __forceinline__ int dc_pred(const int16_t* seg_levels, int j, int gray)
{
    int p;
    if (gray) {
        p = j - 1;
    } else {
        const int b = j % 6;
        p = b == 0 ? j - 3 : (b < 4 ? j - 1 : j - 6);
    }
    return p >= 0 ? seg_levels[(size_t)p * 64] : 0;
}

// One workgroup per (segment, frame): a wave per block sizes its codes (a lane
// per coefficient, the run from a ballot), then the block scans the lengths.
// OPT: the group's tables (k_jpeg_huff_build), one pair per class, instead of
// the handle's fixed pair.
template <bool OPT>
__global__ __launch_bounds__(256) void k_jpeg_bits(JpegGeom g, const JpegTables* __restrict__ tab,
                                                   const JpegOptTables* __restrict__ opt,
                                                   const int16_t* __restrict__ levels, uint32_t* __restrict__ boff,
                                                   uint32_t* __restrict__ segbits)
{
    constexpr int NC = OPT ? 2 : 1;
    __shared__ uint32_t s_dc[NC][12], s_ac[NC][256], s_w[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (OPT) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            s_ac[k][t] = opt->ac[k][t];
            if (t < 12) s_dc[k][t] = opt->dc[k][t];
        }
    } else {
        s_ac[0][t] = tab->ac[t];
        if (t < 12) s_dc[0][t] = tab->dc[t];
    }
    __syncthreads();
    const size_t seg = (size_t)blockIdx.y * g.nseg + blockIdx.x;
    const int16_t* lv = levels + seg * g.bps * 64;
    uint32_t* bo = boff + seg * g.bps;
    const int zrl0 = (int)(s_ac[0][0xF0] >> 16);
    for (int j = wave; j < g.bps; j += 4) {
        const int v = lv[(size_t)j * 64 + lane];
        const int pred = lane == 0 ? dc_pred(lv, j, g.gray) : 0;
        const int k = OPT ? block_class(j, g.gray) : 0;
        const int zrl = OPT ? (int)(s_ac[k][0xF0] >> 16) : zrl0;
        const LaneCode c = lane_code(v, lane, pred, s_dc[k], s_ac[k]);
        const uint32_t inc = wave_incl_scan((uint32_t)(c.nzrl * zrl + c.n), lane);
        if (lane == 63) bo[j] = inc;
    }
    __syncthreads();
    uint32_t carry = 0;
    for (int c0 = 0; c0 < g.bps; c0 += 256) {
        const int j = c0 + t;
        const uint32_t v = j < g.bps ? bo[j] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan(v, s_w, &tot);
        if (j < g.bps) bo[j] = carry + ex;
        carry += tot;
    }
    if (t == 0) segbits[seg] = carry;
}

// ---- rate target: k_jpeg_rate_bits, k_jpeg_rate_step, k_jpeg_quant ------------------
// The block whose DC is block j's predictor (dc_pred's rule), -1 for none.
__device__ __forceinline__ int dc_pred_block(int j, int gray)
{
    if (gray) return j - 1;
    const int b = j % 6;
    return b == 0 ? j - 3 : (b < 4 ? j - 1 : j - 6);
}

// One round of the search, k_jpeg_bits' geometry: a workgroup per (segment,
// frame), a wave per block, a lane per coefficient. The two quantisers of the
// round's quality are built in LDS in zigzag order; a lane quantises its
// coefficient (lane 0 also the predecessor's DC) and sizes its code with the
// fixed tables; the segment's bits become bytes and go to the estimate with one
// atomic a workgroup. Integer sums: the order of the atomics does not matter.
__global__ __launch_bounds__(256) void k_jpeg_rate_bits(JpegGeom g, const JpegTables* __restrict__ tab,
                                                        const int16_t* __restrict__ coef,
                                                        JpegRateState* __restrict__ rs)
{
    __shared__ uint32_t s_dc[12], s_ac[256], s_w[4];
    __shared__ uint16_t s_q[2][64];
    if (!rs->search.active) return;   // (the same in every thread: k_jpeg_rate_step wrote it before this launch)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int quality = rs->search.q;
    s_ac[t] = tab->ac[t];
    if (t < 12) s_dc[t] = tab->dc[t];
    if (t < 128) s_q[t >> 6][tab->zpos[t & 63] & 63] = rate_quant(rs->base[t >> 6][t & 63], quality);
    __syncthreads();
    const size_t seg = (size_t)blockIdx.y * g.nseg + blockIdx.x;
    const int16_t* cf = coef + seg * g.bps * 64;
    const int zrl = (int)(s_ac[0xF0] >> 16);
    uint32_t bits = 0;   // of this wave's blocks (the same in all its lanes)
    for (int j = wave; j < g.bps; j += 4) {
        const uint16_t* q = s_q[block_class(j, g.gray)];
        const int lv = rate_level(cf[(size_t)j * 64 + lane], q[lane], lane > 0);
        int pred = 0;
        if (lane == 0) {
            const int p = dc_pred_block(j, g.gray);
            if (p >= 0) pred = rate_level(cf[(size_t)p * 64], q[0], false);
        }
        const LaneCode c = lane_code(lv, lane, pred, s_dc, s_ac);
        uint32_t n = (uint32_t)(c.nzrl * zrl + c.n);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
        bits += n;
    }
    if (lane == 0) s_w[wave] = bits;
    __syncthreads();
    if (t == 0) atomicAdd(&rs->est, (unsigned long long)rate_seg_bytes(s_w[0] + s_w[1] + s_w[2] + s_w[3]));
}

// Behind every round: thread 0 applies the search step to the round's estimate
// and clears it. Behind the last round the 128 threads also leave the chosen
// quality's quantiser in tab->q and its DQT pair in the group's prefix (the SOS
// behind them when `sos`: fixed tables; k_jpeg_huff_build appends DHT + SOS
// otherwise), and thread 0 the counters and the next group's search.
__global__ __launch_bounds__(128) void k_jpeg_rate_step(JpegRateState* __restrict__ rs, JpegTables* __restrict__ tab,
                                                        uint32_t m, int round, int last, int nc, int sos)
{
    __shared__ int s_quality;
    const int t = threadIdx.x;
    if (t == 0) {
        const uint64_t budget = (uint64_t)m * rs->target;
        RateSearch s = rs->search;
        rate_search_step(&s, round, rs->q_max, rate_estimate(m, rs->frame_fixed, rs->est), budget);
        rs->est = 0ull;
        s_quality = s.lo;
        if (last) {
            rate_stats_add(&rs->stats, s, m, budget);
            rate_search_begin(&s, rs->q_min);
        }
        rs->search = s;
    }
    if (!last) return;
    __syncthreads();
    const int id = t >> 6, i = t & 63;
    const uint16_t q = rate_quant(rs->base[id][i], s_quality);
    uint8_t* d = rs->prefix + id * kRateDqtBytes;
    tab->q[id][i] = q;
    d[5 + (tab->zpos[i] & 63)] = (uint8_t)q;
    if (i < 5) d[i] = rate_dqt_head(i, id);
    if (t == 0) {
        int len = kRateDqtPairBytes;
        if (sos) {   // the fixed tables' SOS: every component on tables 0
            len = huff_put_sos(rs->prefix, len, nc);
            for (int c = 0; c < 3; ++c)
                if (c < nc) rs->prefix[kRateDqtPairBytes + 6 + 2 * c] = 0x00;
        }
        rs->prefix_len = (uint32_t)len;
    }
}

// coef -> levels at tab's quantiser (what k_jpeg_dct stores at a fixed quality):
// a thread takes eight coefficients of one block, 16 bytes in and out.
__global__ __launch_bounds__(256) void k_jpeg_quant(const JpegTables* __restrict__ tab, const int16_t* __restrict__ coef,
                                                    int16_t* __restrict__ levels, size_t nvec, int gray)
{
    __shared__ uint16_t s_q[2][64];
    const int t = threadIdx.x;
    if (t < 128) s_q[t >> 6][tab->zpos[t & 63] & 63] = tab->q[t >> 6][t & 63];
    __syncthreads();
    const size_t v = (size_t)blockIdx.x * 256 + t;
    if (v >= nvec) return;
    const uint16_t* q = s_q[block_class((int)((v >> 3) % 6), gray)];   // (a segment's blocks are a multiple of 6 in colour)
    const int k0 = (int)(v & 7) * 8;
    union {
        uint4 u;
        int16_t h[8];
    } x;
    x.u = reinterpret_cast<const uint4*>(coef)[v];
#pragma unroll
    for (int i = 0; i < 8; ++i) x.h[i] = (int16_t)rate_level(x.h[i], q[k0 + i], k0 + i > 0);
    reinterpret_cast<uint4*>(levels)[v] = x.u;
}

// ---- k_jpeg_pack ------------------------------------------------------------------
constexpr int kPackDwords = (kJpegChunk * kJpegMaxBlockBits + 8 + 31) / 32 + 2;

// OR the low n (<= 32) bits of v into the MSB-first bit buffer at bit `pos`.
__device__ __forceinline__ void put_bits(uint32_t* buf, uint32_t pos, uint32_t v, int n)
{
    if (n <= 0) return;
    const uint32_t w = pos >> 5;
    if (w + 1 >= (uint32_t)kPackDwords) return;   // (cannot happen: the buffer holds a chunk's worst case)
    const unsigned long long x = ((unsigned long long)v << (64 - n)) >> (pos & 31);
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    if (hi) atomicOr(&buf[w], hi);
    if (lo) atomicOr(&buf[w + 1], lo);
}

// One workgroup per (segment, frame). Chunks of kJpegChunk blocks: the codes are
// OR-ed into LDS at their bit offsets (neighbouring lanes share dwords: LDS
// atomics), then the chunk's whole bytes are written out with every 0xFF
// followed by 0x00; the partial last byte is carried into the next chunk, and
// the segment's last byte is padded with 1-bits.
template <bool OPT>
__global__ __launch_bounds__(256) void k_jpeg_pack(JpegGeom g, const JpegTables* __restrict__ tab,
                                                   const JpegOptTables* __restrict__ opt,
                                                   const int16_t* __restrict__ levels,
                                                   const uint32_t* __restrict__ boff,
                                                   const uint32_t* __restrict__ segbits, uint8_t* __restrict__ scratch,
                                                   uint32_t* __restrict__ seglen)
{
    constexpr int NC = OPT ? 2 : 1;
    __shared__ uint32_t s_dc[NC][12], s_ac[NC][256], s_w[4];
    __shared__ uint32_t s_buf[kPackDwords];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (OPT) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            s_ac[k][t] = opt->ac[k][t];
            if (t < 12) s_dc[k][t] = opt->dc[k][t];
        }
    } else {
        s_ac[0][t] = tab->ac[t];
        if (t < 12) s_dc[0][t] = tab->dc[t];
    }
    const size_t seg = (size_t)blockIdx.y * g.nseg + blockIdx.x;
    const int16_t* lv = levels + seg * g.bps * 64;
    const uint32_t* bo = boff + seg * g.bps;
    uint8_t* dst = scratch + seg * g.segcap;
    const uint32_t total = segbits[seg];
    __syncthreads();
    const uint32_t zrl_code0 = s_ac[0][0xF0] & 0xffffu;
    const int zrl0 = (int)(s_ac[0][0xF0] >> 16);
    uint32_t carry = 0, outpos = 0;
    for (int c0 = 0; c0 < g.bps; c0 += kJpegChunk) {
        const int cnt = min(kJpegChunk, g.bps - c0);
        const bool last = c0 + cnt == g.bps;
        const uint32_t bit0 = bo[c0] & ~7u, bit1 = last ? total : bo[c0 + cnt];
        const uint32_t span = bit1 - bit0;
        const int nd = (int)min((uint32_t)kPackDwords, (span + 31) / 32 + 2);
        for (int i = t; i < nd; i += 256) s_buf[i] = i == 0 ? carry << 24 : 0u;
        __syncthreads();
        for (int j = wave; j < cnt; j += 4) {
            const int v = lv[(size_t)(c0 + j) * 64 + lane];
            const int pred = lane == 0 ? dc_pred(lv, c0 + j, g.gray) : 0;
            const int k = OPT ? block_class(c0 + j, g.gray) : 0;
            const uint32_t zrl_code = OPT ? s_ac[k][0xF0] & 0xffffu : zrl_code0;
            const int zrl = OPT ? (int)(s_ac[k][0xF0] >> 16) : zrl0;
            const LaneCode c = lane_code(v, lane, pred, s_dc[k], s_ac[k]);
            const uint32_t mine = (uint32_t)(c.nzrl * zrl + c.n);
            uint32_t pos = bo[c0 + j] - bit0 + wave_incl_scan(mine, lane) - mine;
            for (int z = 0; z < c.nzrl; ++z, pos += zrl) put_bits(s_buf, pos, zrl_code, zrl);
            put_bits(s_buf, pos, c.code, c.n);
        }
        if (last && t == 0) {
            const int npad = (int)((0u - span) & 7u);
            put_bits(s_buf, span, (1u << npad) - 1u, npad);
        }
        __syncthreads();
        const uint32_t nbytes = last ? (span + 7) >> 3 : span >> 3;
        carry = last ? 0u : (s_buf[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xffu;
        for (uint32_t base = 0; base < nbytes; base += 1024) {
            const uint32_t idx = (base >> 2) + t;
            const int nv = idx * 4 < nbytes ? (int)min(4u, nbytes - idx * 4) : 0;
            const uint32_t v = nv ? s_buf[idx] : 0u;
            uint32_t cntb = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nv) cntb += 1 + (((v >> (24 - 8 * i)) & 0xffu) == 0xffu);
            uint32_t tot;
            uint32_t p = outpos + block_excl_scan(cntb, s_w, &tot);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nv) {
                    const uint32_t b = (v >> (24 - 8 * i)) & 0xffu;
                    if (p < g.segcap) dst[p] = (uint8_t)b;
                    ++p;
                    if (b == 0xffu) {
                        if (p < g.segcap) dst[p] = 0;
                        ++p;
                    }
                }
            outpos += tot;
        }
        __syncthreads();   // s_buf is zeroed next
    }
    if (t == 0) seglen[seg] = outpos;
}

// ---- k_jpeg_hist ------------------------------------------------------------------
// One workgroup per (segment, frame), a wave per block, a lane per coefficient
// (k_jpeg_bits' shape): the symbols of the segment are counted per table class
// in LDS (a segment's counts fit 32 bits) and the non-zero counters added to the
// group's counts[4][256] (DC class 0, AC class 0, DC class 1, AC class 1).
// Integer sums: the result does not depend on the order of the atomics.
__global__ __launch_bounds__(256) void k_jpeg_hist(JpegGeom g, const int16_t* __restrict__ levels,
                                                   unsigned long long* __restrict__ counts)
{
    constexpr int NS = 12 + 256;
    __shared__ uint32_t s_h[2 * NS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < 2 * NS; i += 256) s_h[i] = 0u;
    __syncthreads();
    const size_t seg = (size_t)blockIdx.y * g.nseg + blockIdx.x;
    const int16_t* lv = levels + seg * g.bps * 64;
    for (int j = wave; j < g.bps; j += 4) {
        const int v = lv[(size_t)j * 64 + lane];
        const int pred = lane == 0 ? dc_pred(lv, j, g.gray) : 0;
        const LaneSym s = lane_symbol(v, lane, pred);
        uint32_t* h = s_h + block_class(j, g.gray) * NS;
        if (s.sym >= 0) atomicAdd(&h[lane == 0 ? min(s.sym, 11) : 12 + (s.sym & 255)], 1u);
        if (s.nzrl) atomicAdd(&h[12 + 0xF0], (uint32_t)s.nzrl);
    }
    __syncthreads();
    for (int i = t; i < 2 * NS; i += 256) {
        const uint32_t c = s_h[i];
        if (!c) continue;
        const int cls = i >= NS, r = i - cls * NS;
        atomicAdd(&counts[(size_t)(2 * cls + (r >= 12)) * 256 + (r >= 12 ? r - 12 : r)], (unsigned long long)c);
    }
}

// ---- k_jpeg_huff_build ------------------------------------------------------------
// counts[4][256] -> the group's tables and its DHT + SOS prefix; jpeg_huff_core.h
// is the serial statement. One workgroup, a wave per table. A lane owns the
// symbols lane + 64 k (k < 5; 256 is the reserved one): a merge of K.2 is one
// wave-wide reduction to the two least keys (frequency, then the larger index),
// and "every symbol of both groups one bit longer" one step on a per-symbol
// group id. At most 256 merges; no count can make a loop run on.
struct HuffKey {
    unsigned long long f;   // ~0: none
    int i;                  // -1: none
};

__device__ __forceinline__ bool huff_before(const HuffKey& a, const HuffKey& b)
{
    return a.f < b.f || (a.f == b.f && a.i > b.i);
}

// (a1, a2) <- the two least of {a1, a2, b1, b2}, given a1 <= a2 and b1 <= b2.
__device__ __forceinline__ void huff_least2(HuffKey& a1, HuffKey& a2, const HuffKey& b1, const HuffKey& b2)
{
    if (huff_before(b1, a1)) {
        a2 = huff_before(a1, b2) ? a1 : b2;
        a1 = b1;
    } else if (huff_before(b1, a2)) {
        a2 = b1;
    }
}

__device__ __forceinline__ HuffKey huff_shfl_xor(const HuffKey& k, int d)
{
    return HuffKey{__shfl_xor(k.f, d, 64), __shfl_xor(k.i, d, 64)};
}

// The DHT + SOS bytes go to pdst + base and base + their length to *plen_dst: the
// tables' own prefix (base 0), or a rate handle's behind its DQT pair.
__global__ __launch_bounds__(256) void k_jpeg_huff_build(const unsigned long long* __restrict__ counts, int nc,
                                                         JpegOptTables* __restrict__ out, uint8_t* __restrict__ pdst,
                                                         uint32_t* __restrict__ plen_dst, uint32_t base)
{
    __shared__ uint16_t s_size[kHuffTables][kHuffSyms + 1];
    __shared__ uint32_t s_cnt[kHuffTables][kHuffMaxDepth + 2];
    __shared__ uint16_t s_bits[kHuffTables][kHuffMaxDepth + 2];
    __shared__ uint8_t s_vals[kHuffTables][256];
    __shared__ uint32_t s_code[kHuffTables][256];
    __shared__ int s_nvals[kHuffTables];
    __shared__ uint8_t s_prefix[(kHuffPrefixCap + 3) & ~3];
    __shared__ int s_plen;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const unsigned long long* c = counts + 256 * w;
    const HuffKey none{~0ull, -1};
    unsigned long long freq[5];
    int size[5], group[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int s = lane + 64 * k;
        freq[k] = s < 256 ? c[s] : (s == 256 ? 1ull : 0ull);
        size[k] = 0;
        group[k] = s;
        if (k < 4) s_code[w][s] = 0u;
    }
    for (int l = lane; l < kHuffMaxDepth + 2; l += 64) s_cnt[w][l] = 0u;
    for (int merge = 0; merge < 256; ++merge) {
        HuffKey m1 = none, m2 = none;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (freq[k]) huff_least2(m1, m2, HuffKey{freq[k], lane + 64 * k}, none);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const HuffKey o1 = huff_shfl_xor(m1, d), o2 = huff_shfl_xor(m2, d);
            huff_least2(m1, m2, o1, o2);
        }
        if (m2.i < 0) break;   // one group left (the same in every lane)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int s = lane + 64 * k;
            if (s == m1.i) freq[k] = m1.f + m2.f;
            if (s == m2.i) freq[k] = 0;
            if (group[k] == m1.i || group[k] == m2.i) {
                ++size[k];
                group[k] = m1.i;
            }
        }
    }
    int deepest = 0, nvals = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int s = lane + 64 * k;
        if (s < kHuffSyms) s_size[w][s] = (uint16_t)size[k];
        deepest = max(deepest, size[k]);
        if (k < 4) nvals += __popcll(__ballot(size[k] > 0));
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) deepest = max(deepest, __shfl_xor(deepest, d, 64));
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (size[k] > 0) atomicAdd(&s_cnt[w][min(size[k], kHuffMaxDepth)], 1u);
    __syncthreads();
    for (int l = lane; l < kHuffMaxDepth + 2; l += 64) s_bits[w][l] = (uint16_t)s_cnt[w][l];
    // HUFFVAL: a symbol's place is the number of coded symbols in front of it
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (size[k] <= 0) continue;
        const int s = lane + 64 * k;
        int rank = 0;
        for (int o = 0; o < 256; ++o) {
            const int so = s_size[w][o];
            rank += so > 0 && (so < size[k] || (so == size[k] && o < s));
        }
        s_vals[w][rank] = (uint8_t)s;
    }
    __syncthreads();
    if (lane == 0) {
        const bool any = huff_limit_bits(s_bits[w], deepest);
        s_nvals[w] = any ? nvals : 0;
        huff_codes(s_bits[w], s_vals[w], s_nvals[w], s_code[w]);
    }
    __syncthreads();
    if (t == 0) {
        int at = 4;
        for (int k = 0; k < kHuffTables; ++k)
            if (s_nvals[k]) at = huff_put_table(s_prefix, at, (k & 1) << 4 | k >> 1, s_bits[k], s_vals[k], s_nvals[k]);
        huff_put_dht_head(s_prefix, at - 4);
        s_plen = huff_put_sos(s_prefix, at, nc);
    }
    __syncthreads();
    for (int k = 0; k < 2; ++k) {
        out->ac[k][t] = s_code[2 * k + 1][t];
        if (t < 12) out->dc[k][t] = s_code[2 * k][t];
    }
    const int plen = s_plen;
    for (int i = t; i < plen; i += 256) pdst[base + i] = s_prefix[i];
    if (t == 0) *plen_dst = base + (uint32_t)plen;
}

// ---- k_jpeg_gather ----------------------------------------------------------------
// One workgroup per (segment, frame): the segment's place is the sum of the
// lengths before it plus their 2-byte RST markers; the last segment is followed
// by EOI. A frame that does not fit its slot is not written at all. prefix (its
// bytes may be NULL): the group's table segments go in front of every frame's
// first segment and count in its size.
__global__ __launch_bounds__(256) void k_jpeg_gather(JpegGeom g, const uint8_t* __restrict__ scratch,
                                                     const uint32_t* __restrict__ seglen,
                                                     JpegPrefix prefix, uint8_t* __restrict__ out,
                                                     size_t out_stride, uint32_t* __restrict__ sizes,
                                                     uint32_t* __restrict__ overflow)
{
    __shared__ uint32_t s_w[4];
    const int t = threadIdx.x, s = blockIdx.x;
    const uint32_t* sl = seglen + (size_t)blockIdx.y * g.nseg;
    const uint32_t plen = prefix.bytes ? min(*prefix.len, prefix.cap) : 0u;
    uint32_t before = 0, all = 0;
    for (int i = t; i < g.nseg; i += 256) {
        const uint32_t n = sl[i] + 2u;   // its RST marker, or EOI after the last
        all += n;
        if (i < s) before += n;
    }
    uint32_t need, pre;
    (void)block_excl_scan(all, s_w, &need);
    (void)block_excl_scan(before, s_w, &pre);
    need += plen;
    pre += plen;
    const bool fits = (size_t)need <= out_stride;
    if (s == 0 && t == 0) {
        sizes[blockIdx.y] = need;
        if (!fits) *overflow = 1u;
    }
    if (!fits) return;
    const uint32_t len = sl[s];
    const uint8_t* src = scratch + ((size_t)blockIdx.y * g.nseg + s) * g.segcap;
    uint8_t* dst = out + (size_t)blockIdx.y * out_stride + pre;
    for (uint32_t i = t; i < len; i += 256) dst[i] = src[i];
    if (s == 0) {
        uint8_t* head = out + (size_t)blockIdx.y * out_stride;
        for (uint32_t i = t; i < plen; i += 256) head[i] = prefix.bytes[i];
    }
    if (t == 0) {
        dst[len] = 0xff;
        dst[len + 1] = s == g.nseg - 1 ? (uint8_t)0xd9 : (uint8_t)(0xd0 + (s & 7));
    }
}

// ---- stream output (dvc_jpeg_encode_stream) ---------------------------------------
// Complete samples back to back; the arithmetic is jpeg_stream_core.h. A frame's
// segments sum to less than 2^31 (dvc_jpeg_create refuses larger frames), so the
// sums inside a frame run in 32 bits and only the offsets in 64.

// One workgroup per launch group of m <= DVC_MAX_BATCH frames: a wave sums a
// frame's segments, then one thread runs the exclusive prefix behind the carry
// of the groups before (*carry; 0 when `first`) and leaves this group's end there.
__global__ __launch_bounds__(256) void k_jpeg_stream_offsets(JpegGeom g, const uint32_t* __restrict__ seglen,
                                                             JpegPrefix prefix,
                                                             uint32_t header_len, int m, int first, uint64_t cap,
                                                             uint64_t* __restrict__ carry,
                                                             uint64_t* __restrict__ offsets,
                                                             uint32_t* __restrict__ overflow)
{
    __shared__ uint64_t s_need[kJpegStreamMaxGroup];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t plen = prefix.bytes ? min(*prefix.len, prefix.cap) : 0u;
    for (int f = wave; f < m; f += 4) {
        uint32_t sum = (uint32_t)stream_seg_sum(seglen + (size_t)f * g.nseg, g.nseg, lane, 64);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (lane == 0) s_need[f] = stream_frame_need(header_len, plen, sum);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ov = 0;
        *carry = stream_group_offsets(s_need, m, first ? 0ull : *carry, cap, offsets, &ov);
        if (ov) *overflow = 1u;
    }
}

// One workgroup per (segment, frame), as k_jpeg_gather, but every byte goes to
// its final place: out + offsets[f] (less *rebase, when the caller's buffer
// begins at this group) + header + prefix + the segments before. Segment 0's
// workgroup also writes the header and the prefix. A sample that does not lie
// inside `cap` is not written.
__global__ __launch_bounds__(256) void k_jpeg_stream_gather(JpegGeom g, const uint8_t* __restrict__ scratch,
                                                            const uint32_t* __restrict__ seglen, JpegPrefix prefix,
                                                            const uint8_t* __restrict__ header, uint32_t header_len,
                                                            const uint64_t* __restrict__ offsets,
                                                            const uint64_t* __restrict__ rebase, uint64_t cap,
                                                            uint8_t* __restrict__ out)
{
    __shared__ uint32_t s_w[4];
    const int t = threadIdx.x, s = blockIdx.x, f = blockIdx.y;
    if (!stream_fits(offsets[f + 1], cap)) return;
    const uint32_t* sl = seglen + (size_t)f * g.nseg;
    const uint32_t plen = prefix.bytes ? min(*prefix.len, prefix.cap) : 0u;
    uint32_t before;
    (void)block_excl_scan((uint32_t)stream_seg_sum(sl, s, t, 256), s_w, &before);
    uint8_t* sample = out + (offsets[f] - (rebase ? *rebase : 0ull));
    uint8_t* dst = sample + stream_seg_start(header_len, plen, before);
    const uint32_t len = sl[s];
    const uint8_t* src = scratch + ((size_t)f * g.nseg + s) * g.segcap;
    for (uint32_t i = t; i < len; i += 256) dst[i] = src[i];
    if (s == 0) {
        for (uint32_t i = t; i < header_len; i += 256) sample[i] = header[i];
        for (uint32_t i = t; i < plen; i += 256) sample[header_len + i] = prefix.bytes[i];
    }
    if (t == 0) {
        dst[len] = 0xff;
        dst[len + 1] = s == g.nseg - 1 ? (uint8_t)0xd9 : (uint8_t)(0xd0 + (s & 7));
    }
}

}  // namespace

hipError_t jpeg_launch_dct(const uint8_t* frames, size_t pitch, size_t fstride, int n, const JpegGeom& g,
                           const JpegTables* tab, const JpegBufs& b, hipStream_t st)
{
    const int aligned = pitch % 4 == 0 && ((uintptr_t)frames & 3) == 0 && (n <= 1 || fstride % 4 == 0);
    const dim3 grid((unsigned)((g.units_x * g.nseg + 3) / 4), (unsigned)n);
    if (b.rate) {
        if (g.gray)
            hipLaunchKernelGGL((k_jpeg_dct<true, true>), grid, dim3(256), 0, st, frames, pitch, fstride, g, tab, b.coef,
                               aligned);
        else
            hipLaunchKernelGGL((k_jpeg_dct<false, true>), grid, dim3(256), 0, st, frames, pitch, fstride, g, tab, b.coef,
                               aligned);
    } else if (g.gray) {
        hipLaunchKernelGGL((k_jpeg_dct<true, false>), grid, dim3(256), 0, st, frames, pitch, fstride, g, tab, b.levels,
                           aligned);
    } else {
        hipLaunchKernelGGL((k_jpeg_dct<false, false>), grid, dim3(256), 0, st, frames, pitch, fstride, g, tab, b.levels,
                           aligned);
    }
    return hipGetLastError();
}

hipError_t jpeg_launch_hist(int n, const JpegGeom& g, const JpegBufs& b, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(b.counts, 0, kHuffTables * 256 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_jpeg_hist, dim3((unsigned)g.nseg, (unsigned)n), dim3(256), 0, st, g, b.levels, b.counts);
    return hipGetLastError();
}

hipError_t jpeg_launch_huff_build(const JpegGeom& g, const JpegBufs& b, hipStream_t st, bool group)
{
    if (group && b.rate)
        hipLaunchKernelGGL(k_jpeg_huff_build, dim3(1), dim3(256), 0, st, b.counts, g.gray ? 1 : 3, b.opt, b.rate->prefix,
                           &b.rate->prefix_len, (uint32_t)kRateDqtPairBytes);
    else
        hipLaunchKernelGGL(k_jpeg_huff_build, dim3(1), dim3(256), 0, st, b.counts, g.gray ? 1 : 3, b.opt, b.opt->prefix,
                           &b.opt->prefix_len, 0u);
    return hipGetLastError();
}

hipError_t jpeg_launch_rate_bits(int n, const JpegGeom& g, const JpegTables* tab, const JpegBufs& b, hipStream_t st)
{
    hipLaunchKernelGGL(k_jpeg_rate_bits, dim3((unsigned)g.nseg, (unsigned)n), dim3(256), 0, st, g, tab, b.coef, b.rate);
    return hipGetLastError();
}

hipError_t jpeg_launch_rate_step(int n, int round, int rounds, const JpegGeom& g, JpegTables* tab, const JpegBufs& b,
                                 hipStream_t st)
{
    hipLaunchKernelGGL(k_jpeg_rate_step, dim3(1), dim3(128), 0, st, b.rate, tab, (uint32_t)n, round,
                       (int)(round == rounds - 1), g.gray ? 1 : 3, (int)(b.opt == nullptr));
    return hipGetLastError();
}

hipError_t jpeg_launch_quant(int n, const JpegGeom& g, const JpegTables* tab, const JpegBufs& b, hipStream_t st)
{
    const size_t nvec = (size_t)n * g.nseg * g.bps * 8;
    hipLaunchKernelGGL(k_jpeg_quant, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, st, tab, b.coef, b.levels, nvec,
                       g.gray);
    return hipGetLastError();
}

hipError_t jpeg_launch_bits(int n, const JpegGeom& g, const JpegTables* tab, const JpegBufs& b, hipStream_t st)
{
    const dim3 grid((unsigned)g.nseg, (unsigned)n);
    if (b.opt)
        hipLaunchKernelGGL(k_jpeg_bits<true>, grid, dim3(256), 0, st, g, tab, b.opt, b.levels, b.boff, b.segbits);
    else
        hipLaunchKernelGGL(k_jpeg_bits<false>, grid, dim3(256), 0, st, g, tab, b.opt, b.levels, b.boff, b.segbits);
    return hipGetLastError();
}

hipError_t jpeg_launch_pack(int n, const JpegGeom& g, const JpegTables* tab, const JpegBufs& b, hipStream_t st)
{
    const dim3 grid((unsigned)g.nseg, (unsigned)n);
    if (b.opt)
        hipLaunchKernelGGL(k_jpeg_pack<true>, grid, dim3(256), 0, st, g, tab, b.opt, b.levels, b.boff, b.segbits,
                           b.scratch, b.seglen);
    else
        hipLaunchKernelGGL(k_jpeg_pack<false>, grid, dim3(256), 0, st, g, tab, b.opt, b.levels, b.boff, b.segbits,
                           b.scratch, b.seglen);
    return hipGetLastError();
}

hipError_t jpeg_launch_gather(int n, const JpegGeom& g, const JpegBufs& b, uint8_t* out, size_t out_stride,
                              uint32_t* sizes, hipStream_t st)
{
    hipLaunchKernelGGL(k_jpeg_gather, dim3((unsigned)g.nseg, (unsigned)n), dim3(256), 0, st, g, b.scratch, b.seglen,
                       b.prefix, out, out_stride, sizes, b.overflow);
    return hipGetLastError();
}

hipError_t jpeg_launch_stream(int n, int first, const JpegGeom& g, const JpegBufs& b, const uint8_t* header,
                              uint32_t header_len, uint64_t* carry, uint64_t* offsets, const uint64_t* rebase,
                              uint8_t* out, uint64_t cap, hipStream_t st)
{
    if (n < 1 || n > kJpegStreamMaxGroup) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_jpeg_stream_offsets, dim3(1), dim3(256), 0, st, g, b.seglen, b.prefix, header_len, n, first, cap,
                       carry, offsets, b.overflow);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_jpeg_stream_gather, dim3((unsigned)g.nseg, (unsigned)n), dim3(256), 0, st, g, b.scratch,
                       b.seglen, b.prefix, header, header_len, offsets, rebase, cap, out);
    return hipGetLastError();
}

}  // namespace dvc
