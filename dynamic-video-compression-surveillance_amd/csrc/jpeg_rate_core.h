// jpeg_rate_core.h — the arithmetic of the Motion-JPEG encoder's rate target
// (DESIGN.md "Motion-JPEG stream", "Rate target"), as plain C++ that compiles
// for the device (k_jpeg_rate_bits, k_jpeg_rate_step and k_jpeg_quant in
// jpeg_kernels.hip), for the library's host side (jpeg_api.hip) and for the host
// alone (tools/jpeg_rate_host_check.cc runs the same text under the host
// sanitizers): the quantiser of a quality, a level from a coefficient, the
// bytes a segment adds to the estimate, the search for the group's quality and
// the DQT segments in front of its frames. Every loop has a static trip count.
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

constexpr int kRateMaxRounds = 8;     // 1 + ceil(log2(100))
constexpr int kRateDqtBytes = 69;     // marker, length, id, 64 entries
constexpr int kRateDqtPairBytes = 2 * kRateDqtBytes;

// Entry of natural index i of the quantiser of `quality` (1..100): the IJG
// scaling of the base entry, kept inside 1..255 (8-bit DQT entries).
DVC_HD uint16_t rate_quant(int base, int quality)
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base * s + 50) / 100;
    return (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
}

// The level of coefficient F under the entry Q: round half away from zero; an
// AC level (zigzag position > 0) is kept inside +-1023, the DC is not (its
// difference is clamped where it is coded). What k_jpeg_dct does at one quality.
DVC_HD int rate_level(int F, int Q, bool ac)
{
    const uint32_t a = (uint32_t)(F < 0 ? -F : F);
    uint32_t l = (a + ((uint32_t)Q >> 1)) / (uint32_t)Q;
    if (ac && l > 1023u) l = 1023u;
    return F < 0 ? -(int)l : (int)l;
}

// The largest |F| the two integer DCT passes give on samples in -128..127, from
// the absolute row sums of the matrix M (M[k][n], n < 4; M[k][7-n] = +-M[k][n]):
// a row pass (+512) >> 10 and a column pass (+32768) >> 16. A coefficient
// stored as int16 needs this below 32768.
DVC_HD int64_t rate_coef_bound(const int M[8][4])
{
    int64_t worst = 0;
    for (int k = 0; k < 8; ++k) {
        int64_t sum = 0;
        for (int n = 0; n < 4; ++n) sum += 2 * (int64_t)(M[k][n] < 0 ? -M[k][n] : M[k][n]);
        if (sum > worst) worst = sum;
    }
    const int64_t r = (128 * worst + 512) >> 10;        // |x| <= 128; the negative side rounds no further out
    return ((r * worst + 32768) >> 16) + 1;
}

// Rounds of a search over q_min..q_max: the one at q_min, then a bisection.
DVC_HD int rate_rounds(int q_min, int q_max)
{
    const int n = q_max - q_min + 1;
    int r = 0;
    for (int k = 0; k < kRateMaxRounds - 1; ++k)
        if ((1 << r) < n) ++r;
    return 1 + r;
}

// What a segment of `bits` bits adds to the estimate: its whole bytes before
// stuffing and its 2-byte RST or EOI marker.
DVC_HD uint64_t rate_seg_bytes(uint32_t bits) { return (((uint64_t)bits + 7u) >> 3) + 2u; }

// E(q) of a group of m frames: what is constant per frame (the fixed-table
// header with its DQT, DHT and SOS segments) and the segments' sum.
DVC_HD uint64_t rate_estimate(uint32_t m, uint32_t frame_fixed, uint64_t seg_sum)
{
    return (uint64_t)m * frame_fixed + seg_sum;
}

// The search of one group. `q` is the quality the coming round evaluates while
// `active`; afterwards lo is the chosen quality and est_lo its estimate.
struct RateSearch {
    uint64_t est_lo;
    int32_t lo, hi, q, active, miss;
};

DVC_HD void rate_search_begin(RateSearch* s, int q_min)
{
    s->est_lo = 0;
    s->lo = s->hi = s->q = q_min;
    s->active = 1;
    s->miss = 0;
}

// Apply round `round`'s estimate `est` = E(s->q) against the budget. Round 0 is
// E(q_min): over the budget the group is a miss and the search ends at q_min.
// A later round moves lo up to q when E(q) fits and hi below q when not.
DVC_HD void rate_search_step(RateSearch* s, int round, int q_max, uint64_t est, uint64_t budget)
{
    if (!s->active) return;
    if (round == 0) {
        s->est_lo = est;
        if (est > budget) {
            s->miss = 1;
            s->active = 0;
            return;
        }
        s->hi = q_max;
    } else if (est <= budget) {
        s->lo = s->q;
        s->est_lo = est;
    } else {
        s->hi = s->q - 1;
    }
    if (s->lo < s->hi) {
        s->q = (s->lo + s->hi + 1) >> 1;
    } else {
        s->q = s->lo;
        s->active = 0;
    }
}

// The cumulative counters of a rate handle (dvc_jpeg_rate_stats, same layout).
struct RateStats {
    uint64_t groups, frames, missed_groups, est_bytes, budget_bytes, quality_frames, q_lowest, q_highest, q_last;
};

DVC_HD void rate_stats_add(RateStats* st, const RateSearch& s, uint32_t m, uint64_t budget)
{
    const uint64_t q = (uint64_t)s.lo;
    if (!st->groups || q < st->q_lowest) st->q_lowest = q;
    if (!st->groups || q > st->q_highest) st->q_highest = q;
    st->q_last = q;
    st->groups += 1;
    st->frames += m;
    st->missed_groups += (uint64_t)s.miss;
    st->est_bytes += s.est_lo;
    st->budget_bytes += budget;
    st->quality_frames += q * m;
}

// Byte i (< kRateDqtBytes) of the DQT segment of table `id` whose entry at
// zigzag position k is qz(k): marker, length 67, Pq/Tq, the entries.
DVC_HD uint8_t rate_dqt_head(int i, int id)
{
    return i == 0 ? 0xff : (i == 1 ? 0xdb : (i == 2 ? 0 : (i == 3 ? 67 : (uint8_t)id)));
}

// The two DQT segments of `quality` at dst[0 .. kRateDqtPairBytes): base[t] in
// natural order, zpos[i] the zigzag position of natural index i.
DVC_HD void rate_put_dqt_pair(uint8_t* dst, const uint8_t* base0, const uint8_t* base1, const uint8_t* zpos, int quality)
{
    for (int t = 0; t < 2; ++t) {
        uint8_t* d = dst + t * kRateDqtBytes;
        const uint8_t* base = t ? base1 : base0;
        for (int i = 0; i < 5; ++i) d[i] = rate_dqt_head(i, t);
        for (int i = 0; i < 64; ++i) d[5 + (zpos[i] & 63)] = (uint8_t)rate_quant(base[i], quality);
    }
}

}  // namespace dvc
