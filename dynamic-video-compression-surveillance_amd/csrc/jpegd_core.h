// jpegd_core.h — the baseline-JPEG decoder's two serial routines, as plain C++
// that compiles for the device (jpegd_kernels.hip) and for the host
// (jpegd_api.hip's header parser shares the tables; tools/jpegd_host_check.cc
// runs the same text under the host sanitizers): the entropy decoder of one
// restart segment and the 8-point inverse DCT. DESIGN.md "Motion-JPEG decoder"
// is the normative text. Ordinary loads and stores only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DVC_HD __host__ __device__ __forceinline__
#else
#define DVC_HD inline
#endif

namespace dvc {

constexpr int kJpegdLookBits = 9;
constexpr int kJpegdDamaged = -1;   // DVC_E_INVALID: a frame's entropy data is damaged

// One Huffman table as the decoder walks it.
struct JpegdHuff {
    uint16_t look[1 << kJpegdLookBits];   // by the next 9 bits: code length << 8 | symbol; 0: a longer code, or none
    int32_t maxcode[17];                  // [l]: the largest code of length l, -1 when there is none
    int32_t valoff[17];                   // [l]: index into vals of length l's first code, minus that code
    uint8_t vals[256];
};

struct JpegdTables {
    JpegdHuff dc[2], ac[2];
    uint16_t q[3][64];    // quantiser of each component, natural order
    uint8_t nat[64];      // natural (row-major) index of zigzag position k
    uint8_t dc_sel[3], ac_sel[3];   // each component's tables
    uint8_t pad_[2];
};

// One stream's geometry. A single component's MCU is one 8x8 block. A colour
// MCU is 8 hs x 8 vs pixels, (hs, vs) the luma sampling factors: 2x2 (4:2:0),
// and for a camera handle 2x1 (4:2:2) and 1x1 (4:4:4); its hs * vs + 2 blocks
// are the luma blocks in raster order inside the MCU (Y00 Y01 Y10 Y11), then
// Cb, Cr. A restart segment is `ri` MCUs in raster order (the last may be
// shorter). The real chroma size is ceil(W / hs) x ceil(H / vs).
struct JpegdGeom {
    int W, H;
    int gray;
    int mcus_x, mcus_y, mcus;
    int ri;       // MCUs per segment (the whole frame when the stream has no DRI)
    int nseg;
    int bpm;      // blocks per MCU: hs * vs + 2, or 1
    int yw, yh;   // the MCU-padded luma plane
    int cw, ch;   // the MCU-padded chroma planes, 8 mcus_x x 8 mcus_y (0 when gray)
    int hs, vs;   // luma sampling factors (1, 1 when gray)
};

// Canonical tables from a DHT's BITS (16 counts) and HUFFVAL. False when the
// counts overflow a length's code space or name more than 256 symbols.
inline bool jpegd_build_huff(const uint8_t* bits, const uint8_t* vals, int nvals, JpegdHuff* h)
{
    for (int i = 0; i < (1 << kJpegdLookBits); ++i) h->look[i] = 0;
    for (int i = 0; i < 256; ++i) h->vals[i] = i < nvals ? vals[i] : 0;
    h->maxcode[0] = -1;
    h->valoff[0] = 0;
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (k + n > 256 || k + n > nvals || code + n > (1 << l)) return false;
        h->valoff[l] = k - code;
        for (int i = 0; i < n; ++i, ++k, ++code) {
            if (l <= kJpegdLookBits) {
                const int sh = kJpegdLookBits - l;
                for (int f = 0; f < (1 << sh); ++f) h->look[(code << sh) | f] = (uint16_t)(l << 8 | vals[k]);
            }
        }
        h->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    return true;
}

// MSB-first bit reader over one segment's bytes: 0xFF 0x00 unstuffs to 0xFF, any
// other byte after 0xFF is a marker and ends the data. Bits past the end read as
// zero and are never counted as available.
struct JpegdBits {
    const uint8_t* p;
    uint32_t len, pos;
    uint64_t buf;   // the next bits, from bit 63 down
    int cnt;        // how many of them are real
};

// The four bytes p[0..3], first byte highest. The caller has checked that p[0..7]
// are inside the data. On the device they come from the two aligned dwords that
// hold them: the first may start up to three bytes in front of p, inside the
// same aligned dword as p[0] (so inside the same page of the same allocation).
DVC_HD uint32_t jpegd_load_be32(const uint8_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uintptr_t a = (uintptr_t)p;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    const uint64_t two = (uint64_t)w[1] << 32 | w[0];
    return __builtin_bswap32((uint32_t)(two >> (8 * (a & 3))));
#else
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
#endif
}

// At most 32 real bits on entry (jpegd_symbol's refill point). Four bytes at once
// when none of them is 0xFF and eight are left; byte by byte otherwise.
DVC_HD void jpegd_fill(JpegdBits& b)
{
    if (b.cnt <= 32 && b.pos + 8 <= b.len) {
        const uint32_t w = jpegd_load_be32(b.p + b.pos);
        if (((~w - 0x01010101u) & w & 0x80808080u) == 0) {   // no byte of w is 0xFF
            b.buf |= (uint64_t)w << (32 - b.cnt);
            b.cnt += 32;
            b.pos += 4;
            return;
        }
    }
    while (b.cnt <= 56 && b.pos < b.len) {
        const uint32_t v = b.p[b.pos];
        if (v == 0xffu) {
            if (b.pos + 1 < b.len && b.p[b.pos + 1] == 0) {
                b.pos += 2;
            } else {
                b.pos = b.len;
                break;
            }
        } else {
            b.pos += 1;
        }
        b.buf |= (uint64_t)v << (56 - b.cnt);
        b.cnt += 8;
    }
}

// The next Huffman symbol, or -1: no such code, or the data ran out.
DVC_HD int jpegd_symbol(JpegdBits& b, const JpegdHuff* h)
{
    if (b.cnt < 32) jpegd_fill(b);
    const uint32_t e = h->look[(uint32_t)(b.buf >> (64 - kJpegdLookBits))];
    int l, sym;
    if (e) {
        l = (int)(e >> 8);
        sym = (int)(e & 0xffu);
    } else {
        sym = -1;
        for (l = kJpegdLookBits + 1; l <= 16; ++l) {
            const int32_t code = (int32_t)(b.buf >> (64 - l));
            if (code <= h->maxcode[l]) {
                sym = h->vals[(code + h->valoff[l]) & 255];
                break;
            }
        }
        if (sym < 0) return -1;
    }
    if (l > b.cnt) return -1;
    b.buf <<= l;
    b.cnt -= l;
    return sym;
}

// s (1..15) magnitude bits, extended: v < 2^(s-1) ? v - 2^s + 1 : v. False when the data ran out.
DVC_HD bool jpegd_receive(JpegdBits& b, int s, int* out)
{
    if (s > b.cnt) return false;
    const int v = (int)(b.buf >> (64 - s));
    b.buf <<= s;
    b.cnt -= s;
    *out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    return true;
}

// One restart segment: `nmcu` MCUs of entropy data in p[0, len) -> int16 levels,
// natural order, 64 per block, blocks in scan order at `coef` (zero on entry).
// `bpm` is the layout (JpegdGeom::bpm): 1 for a single component, otherwise the
// MCU's bpm - 2 luma blocks come first, then Cb and Cr. Every read is inside
// p[0, len) and every store inside coef[0, nmcu * bpm * 64). Returns 0, or
// kJpegdDamaged at the first invalid code, run past coefficient 63 or read past
// the data. CAMERA false is the text for the two layouts of a default handle
// (bpm 1 and 6), which keeps its code; true takes any bpm.
template <bool CAMERA>
DVC_HD int jpegd_segment_t(const uint8_t* p, uint32_t len, int nmcu, int layout, const JpegdTables* t, int16_t* coef)
{
    JpegdBits b{p, len, 0u, 0ull, 0};
    int pred[3] = {0, 0, 0};
    const int bpm = CAMERA ? layout : (layout == 1 ? 1 : 6);
    const int nluma = bpm == 1 ? 1 : bpm - 2;
    for (int m = 0; m < nmcu; ++m) {
        for (int j = 0; j < bpm; ++j) {
            const int c = CAMERA ? (j < nluma ? 0 : j - nluma + 1) : (j < 4 ? 0 : j - 3);
            const JpegdHuff* dc = &t->dc[t->dc_sel[c] & 1];
            const JpegdHuff* ac = &t->ac[t->ac_sel[c] & 1];
            int16_t* blk = coef + ((size_t)m * bpm + j) * 64;
            int s = jpegd_symbol(b, dc);
            if (s < 0 || s > 15) return kJpegdDamaged;
            if (s) {
                int d;
                if (!jpegd_receive(b, s, &d)) return kJpegdDamaged;
                pred[c] = (int)((uint32_t)pred[c] + (uint32_t)d);
            }
            blk[0] = (int16_t)pred[c];
            int k = 1;
            while (k < 64) {
                const int rs = jpegd_symbol(b, ac);
                if (rs < 0) return kJpegdDamaged;
                const int r = rs >> 4;
                s = rs & 15;
                if (s == 0) {
                    if (r != 15) break;   // EOB
                    k += 16;              // ZRL
                    if (k > 64) return kJpegdDamaged;
                    continue;
                }
                k += r;
                if (k > 63) return kJpegdDamaged;
                int v;
                if (!jpegd_receive(b, s, &v)) return kJpegdDamaged;
                blk[t->nat[k] & 63] = (int16_t)v;
                ++k;
            }
        }
    }
    return 0;
}

DVC_HD int jpegd_segment(const uint8_t* p, uint32_t len, int nmcu, int bpm, const JpegdTables* t, int16_t* coef)
{
    if (bpm == 1 || bpm == 6) return jpegd_segment_t<false>(p, len, nmcu, bpm, t, coef);
    return jpegd_segment_t<true>(p, len, nmcu, bpm, t, coef);
}

// libjpeg's slow-integer 8-point inverse DCT pass (jidctint): out[i] = (x + rnd)
// >> sh with an arithmetic shift; the sums wrap in 32 bits.
DVC_HD void jpegd_idct8(const int32_t in[8], int32_t out[8], int32_t rnd, int sh)
{
    typedef uint32_t u;
    const u i0 = (u)in[0], i1 = (u)in[1], i2 = (u)in[2], i3 = (u)in[3], i4 = (u)in[4], i5 = (u)in[5], i6 = (u)in[6],
            i7 = (u)in[7];
    u z1 = (i2 + i6) * 4433u;
    const u t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
    const u t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u z5 = (z3 + z4) * 9633u;
    a0 *= 2446u;
    a1 *= 16819u;
    a2 *= 25172u;
    a3 *= 12299u;
    z1 *= (u)-7373;
    z2 *= (u)-20995;
    z3 = z3 * (u)-16069 + z5;
    z4 = z4 * (u)-3196 + z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    const u r = (u)rnd;
    const u o[8] = {t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3};
    for (int i = 0; i < 8; ++i) {
        const u x = o[i] + r;
        // arithmetic shift of the two's-complement value, without a signed overflow
        out[i] = (int32_t)((x >> sh) | ((x & 0x80000000u) ? ~(0xffffffffu >> sh) : 0u));
    }
}

DVC_HD uint8_t jpegd_clamp8(int32_t x) { return (uint8_t)(x < 0 ? 0 : (x > 255 ? 255 : x)); }

// One block: dequantise, columns, rows, + 128, clamp -> 8 rows of 8 bytes.
DVC_HD void jpegd_idct_block(const int16_t* lv, const uint16_t* q, uint8_t* out, size_t pitch)
{
    int32_t ws[64];
    for (int c = 0; c < 8; ++c) {
        int32_t in[8], o[8];
        for (int r = 0; r < 8; ++r) in[r] = (int32_t)lv[r * 8 + c] * (int32_t)q[r * 8 + c];
        jpegd_idct8(in, o, 1024, 11);
        for (int r = 0; r < 8; ++r) ws[r * 8 + c] = o[r];
    }
    for (int r = 0; r < 8; ++r) {
        int32_t o[8];
        jpegd_idct8(ws + r * 8, o, 131072, 18);
        for (int c = 0; c < 8; ++c) out[r * pitch + c] = jpegd_clamp8((int32_t)((uint32_t)o[c] + 128u));
    }
}

// ---- chroma upsampling and colour, per output pixel ---------------------
// s_top / s_bot of chroma row r at column x of plane p (pitch cw): 3 * p[r][x] + the
// row above / below, clamped to the real chroma size dh.
DVC_HD int jpegd_vsum(const uint8_t* p, size_t cw, int dh, int r, int x, int bottom)
{
    const int rn = bottom ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
    return 3 * (int)p[(size_t)r * cw + x] + (int)p[(size_t)rn * cw + x];
}

// The upsampled chroma sample at output pixel (x, y).
DVC_HD int jpegd_chroma_at(const uint8_t* p, size_t cw, int dw, int dh, int x, int y)
{
    const int cx = x >> 1, r = y >> 1;
    if (dw <= 2) return p[(size_t)r * cw + cx];
    const int bottom = y & 1;
    const int s = jpegd_vsum(p, cw, dh, r, cx, bottom);
    if (x & 1) return (3 * s + jpegd_vsum(p, cw, dh, r, cx + 1 < dw ? cx + 1 : dw - 1, bottom) + 7) >> 4;
    return (3 * s + jpegd_vsum(p, cw, dh, r, cx > 0 ? cx - 1 : 0, bottom) + 8) >> 4;
}

// 4:2:2 (camera handles): the upsampled chroma sample at output pixel (x, y). No
// vertical step; along the row 3/4 of the nearer sample and 1/4 of the farther.
DVC_HD int jpegd_chroma_at_h2v1(const uint8_t* p, size_t cw, int dw, int x, int y)
{
    const int cx = x >> 1;
    const uint8_t* row = p + (size_t)y * cw;
    if (dw <= 2) return row[cx];
    if (x & 1) return (3 * (int)row[cx] + (int)row[cx + 1 < dw ? cx + 1 : dw - 1] + 2) >> 2;
    return (3 * (int)row[cx] + (int)row[cx > 0 ? cx - 1 : 0] + 1) >> 2;
}

// Y, Cb, Cr (0..255) -> bgr[3].
DVC_HD void jpegd_bgr(int Y, int Cb, int Cr, uint8_t* bgr)
{
    const int cb = Cb - 128, cr = Cr - 128;
    bgr[2] = jpegd_clamp8(Y + ((91881 * cr + 32768) >> 16));
    bgr[0] = jpegd_clamp8(Y + ((116130 * cb + 32768) >> 16));
    bgr[1] = jpegd_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
}

}  // namespace dvc
