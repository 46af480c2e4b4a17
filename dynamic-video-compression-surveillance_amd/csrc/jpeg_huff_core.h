// jpeg_huff_core.h — the optimised Huffman tables of the Motion-JPEG encoder
// (DESIGN.md "Motion-JPEG stream", "Optimised Huffman tables"), as plain C++
// that compiles for the device (k_jpeg_huff_build in jpeg_kernels.hip) and for
// the host (tools/jpeg_huff_host_check.cc runs the same text under the host
// sanitizers): symbol counts -> code sizes (ISO/IEC 10918-1 K.2 with the
// project's tie-breaks) -> BITS limited to 16 -> HUFFVAL -> canonical codes ->
// the DHT segment and the SOS header behind it. The kernel runs the merge and
// the ranking a lane per symbol and takes the rest from here. Every loop has a
// static trip bound, whatever the counts hold.
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

constexpr int kHuffSyms = 257;         // 256 symbols and the reserved one (256)
constexpr int kHuffMaxDepth = 256;     // 257 leaves: no code is longer
constexpr int kHuffTables = 4;         // DC class 0, AC class 0, DC class 1, AC class 1
// Bytes of the longest DHT + SOS a group can get: four tables of 256 symbols.
constexpr int kHuffPrefixCap = 4 + kHuffTables * (17 + 256) + 14;

// K.2 (figure K.1): merge the two least frequent groups until one is left.
// freq[s] = counts[s], freq[256] = 1. c1 is the least non-zero frequency, the
// largest index among equals; c2 the same without c1; freq[c1] += freq[c2],
// freq[c2] = 0; every symbol of both groups gets one bit longer and belongs to
// c1's group from then on. size[s] = 0 for a symbol that never occurs.
DVC_HD void huff_code_sizes(const uint64_t* counts, uint16_t* size)
{
    uint64_t freq[kHuffSyms];
    uint16_t group[kHuffSyms];
    for (int s = 0; s < kHuffSyms; ++s) {
        freq[s] = s < 256 ? counts[s] : 1u;
        size[s] = 0;
        group[s] = (uint16_t)s;
    }
    for (int merge = 0; merge < 256; ++merge) {
        int c1 = -1, c2 = -1;
        for (int i = 0; i < kHuffSyms; ++i)
            if (freq[i] && (c1 < 0 || freq[i] <= freq[c1])) c1 = i;
        for (int i = 0; i < kHuffSyms; ++i)
            if (freq[i] && i != c1 && (c2 < 0 || freq[i] <= freq[c2])) c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        for (int s = 0; s < kHuffSyms; ++s)
            if (group[s] == c1 || group[s] == c2) {
                ++size[s];
                group[s] = (uint16_t)c1;
            }
    }
}

// bits[l] = how many of the 257 symbols have size l (l in 1..256; bits[0] unused).
// Returns the deepest occupied length.
DVC_HD int huff_count_sizes(const uint16_t* size, uint16_t* bits)
{
    int deepest = 0;
    for (int l = 0; l <= kHuffMaxDepth; ++l) bits[l] = 0;
    for (int s = 0; s < kHuffSyms; ++s)
        if (size[s] >= 1 && size[s] <= kHuffMaxDepth) {
            ++bits[size[s]];
            if (size[s] > deepest) deepest = size[s];
        }
    return deepest;
}

// K.2 (figure K.3) from the deepest occupied length down to 17: a pair of the
// longest codes gives up its common prefix to one of them, the other goes below
// the deepest shorter code, which moves down one bit with it. Then the reserved
// symbol leaves the longest occupied length. False when nothing is coded.
DVC_HD bool huff_limit_bits(uint16_t* bits, int deepest)
{
    for (int i = deepest < kHuffMaxDepth ? deepest : kHuffMaxDepth; i > 16; --i)
        for (int n = 0; n < kHuffSyms && bits[i] > 0; ++n) {
            int j = i - 2;
            for (int k = 0; k < kHuffMaxDepth && j > 0 && bits[j] == 0; ++k) --j;
            if (j <= 0 || bits[i] < 2) {   // (no Huffman tree gives this; counts that are none end here)
                bits[i] = 0;
                break;
            }
            bits[i] = (uint16_t)(bits[i] - 2);
            ++bits[i - 1];
            bits[j + 1] = (uint16_t)(bits[j + 1] + 2);
            --bits[j];
        }
    int i = 16;
    for (int k = 0; k < 16 && i > 0 && bits[i] == 0; ++k) --i;
    if (i <= 0) return false;
    --bits[i];
    return true;
}

// HUFFVAL: the symbols 0..255 that have a code, by size before the adjustment,
// then by value. Returns how many.
DVC_HD int huff_vals(const uint16_t* size, uint8_t* vals)
{
    uint16_t start[kHuffMaxDepth + 2];
    for (int l = 0; l <= kHuffMaxDepth + 1; ++l) start[l] = 0;
    for (int s = 0; s < 256; ++s)
        if (size[s] >= 1 && size[s] <= kHuffMaxDepth) ++start[size[s] + 1];
    for (int l = 1; l <= kHuffMaxDepth + 1; ++l) start[l] = (uint16_t)(start[l] + start[l - 1]);
    const int n = start[kHuffMaxDepth + 1];
    for (int s = 0; s < 256; ++s)
        if (size[s] >= 1 && size[s] <= kHuffMaxDepth) vals[start[size[s]]++] = (uint8_t)s;
    return n;
}

// Canonical codes as a decoder derives them from BITS (bits[1..16]) and
// HUFFVAL: table[symbol] = length << 16 | code; the others stay as they are.
DVC_HD void huff_codes(const uint16_t* bits, const uint8_t* vals, int nvals, uint32_t* table)
{
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < 256 && i < bits[len] && k < nvals; ++i, ++k, ++code) table[vals[k]] = (uint32_t)len << 16 | code;
        code <<= 1;
    }
}

// One table inside a DHT segment: Tc << 4 | Th, BITS, HUFFVAL. Returns the end.
DVC_HD int huff_put_table(uint8_t* dst, int at, int id, const uint16_t* bits, const uint8_t* vals, int nvals)
{
    dst[at++] = (uint8_t)id;
    for (int len = 1; len <= 16; ++len) dst[at++] = (uint8_t)bits[len];
    for (int k = 0; k < 256 && k < nvals; ++k) dst[at++] = vals[k];
    return at;
}

// The DHT marker and length in front of `body` bytes of tables at dst + 4.
DVC_HD void huff_put_dht_head(uint8_t* dst, int body)
{
    dst[0] = 0xff;
    dst[1] = 0xc4;
    dst[2] = (uint8_t)((body + 2) >> 8);
    dst[3] = (uint8_t)(body + 2);
}

// SOS of nc components: table class 0 (DC 0, AC 0) for the first, class 1 for
// the others; spectral selection 0..63, no approximation. Returns the end.
DVC_HD int huff_put_sos(uint8_t* dst, int at, int nc)
{
    dst[at++] = 0xff;
    dst[at++] = 0xda;
    dst[at++] = 0;
    dst[at++] = (uint8_t)(6 + 2 * nc);
    dst[at++] = (uint8_t)nc;
    for (int c = 0; c < nc; ++c) {
        dst[at++] = (uint8_t)(c + 1);
        dst[at++] = c ? 0x11 : 0x00;
    }
    dst[at++] = 0;
    dst[at++] = 63;
    dst[at++] = 0;
    return at;
}

// What one table comes to: BITS in bits[1..16], HUFFVAL, the codes.
struct HuffTable {
    uint16_t bits[kHuffMaxDepth + 1];
    uint8_t vals[256];
    int nvals;             // 0: no symbol occurs, the table is omitted
    uint32_t code[256];    // length << 16 | code; 0 for a symbol without one
};

// The serial statement of the whole path for one table.
DVC_HD void huff_build(const uint64_t* counts, HuffTable* t)
{
    uint16_t size[kHuffSyms];
    huff_code_sizes(counts, size);
    const int deepest = huff_count_sizes(size, t->bits);
    for (int s = 0; s < 256; ++s) t->code[s] = 0;
    t->nvals = huff_limit_bits(t->bits, deepest) ? huff_vals(size, t->vals) : 0;
    huff_codes(t->bits, t->vals, t->nvals, t->code);
}

// counts[4][256] (DC class 0, AC class 0, DC class 1, AC class 1) -> the DHT
// segment (tables 00, 10, 01, 11; one without counts is left out) and the SOS
// header of nc components behind it, at most kHuffPrefixCap bytes. *dht_len
// receives the DHT segment's length; returns the whole length.
DVC_HD int huff_prefix(const uint64_t* counts, int nc, uint8_t* dst, int* dht_len)
{
    int at = 4;
    for (int k = 0; k < kHuffTables; ++k) {
        HuffTable t;
        huff_build(counts + 256 * k, &t);
        if (t.nvals) at = huff_put_table(dst, at, (k & 1) << 4 | k >> 1, t.bits, t.vals, t.nvals);
    }
    huff_put_dht_head(dst, at - 4);
    *dht_len = at;
    return huff_put_sos(dst, at, nc);
}

}  // namespace dvc
