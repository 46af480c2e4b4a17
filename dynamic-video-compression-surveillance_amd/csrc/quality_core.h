// quality_core.h — the quality meter's arithmetic (DESIGN.md "Quality metrics"),
// as plain C++ that compiles for the device (quality_kernels.hip) and for the
// host (tools/quality_host_check.cc runs the same text under the host
// sanitizers): the luma, one pixel pair's contribution to its 4x4 cell, and the
// value of one 8x8 SSIM window from the sums of its four cells; and for the
// split into kept and static regions (tools/quality_regions_host_check.cc) the
// block rule, the classes a cell holds and a window's class. Every result is
// an integer, so any summation order gives the same frame record.
#pragma once
#include <math.h>
#include <stdint.h>

#include "color_core.h"

namespace dvc {

constexpr int kQualitySsimC1 = 416;      // (int)(.01^2 * 255^2 * 64 + .5)
constexpr int kQualitySsimC2 = 235963;   // (int)(.03^2 * 255^2 * 64 * 63 + .5)

// Luma sums of one 4x4 cell of a frame pair: s1 = sum a, s2 = sum b,
// ss = sum (a^2 + b^2), s12 = sum a b. A window is four cells: s1, s2 <= 16320,
// ss <= 8323200, s12 <= 4161600.
struct QualityCell {
    int s1, s2, ss, s12;
};

DVC_HD uint32_t quality_luma(uint32_t b, uint32_t g, uint32_t r) { return gray_px(b, g, r); }   // color_core.h

// One pixel of the reference (a) and of the test frame (b): its squared errors
// go to sse[0..2] (B, G, R) and sse[3] (luma), its luma to the cell's sums. A
// 32-bit sse[] holds 66051 pixels (65025 each at the most).
DVC_HD void quality_px(uint32_t ab, uint32_t ag, uint32_t ar, uint32_t bb, uint32_t bg, uint32_t br, uint32_t (&sse)[4],
                       QualityCell& c)
{
    const int db = (int)ab - (int)bb, dg = (int)ag - (int)bg, dr = (int)ar - (int)br;
    const int ya = (int)quality_luma(ab, ag, ar), yb = (int)quality_luma(bb, bg, br);
    sse[0] += (uint32_t)(db * db);
    sse[1] += (uint32_t)(dg * dg);
    sse[2] += (uint32_t)(dr * dr);
    sse[3] += (uint32_t)((ya - yb) * (ya - yb));
    c.s1 += ya;
    c.s2 += yb;
    c.ss += ya * ya + yb * yb;
    c.s12 += ya * yb;
}

DVC_HD QualityCell quality_add(const QualityCell& p, const QualityCell& q)
{
    return {p.s1 + q.s1, p.s2 + q.s2, p.ss + q.ss, p.s12 + q.s12};
}

// One 8x8 window from its 64-pixel sums: the integer SSIM of x264 / ffmpeg's
// ssim filter, A B / (C D) in IEEE f64 (two multiplies, one correctly rounded
// divide, no contraction: the library and the host check are built with
// -ffp-contract=off), times 2^32, rounded half to even. A, B, C, D stay below
// 2^31 in magnitude; C, D > 0 (vars >= 0 by Cauchy-Schwarz).
DVC_HD int64_t quality_window_q32(const QualityCell& w)
{
    const int s1 = w.s1, s2 = w.s2;
    const int vars = 64 * w.ss - s1 * s1 - s2 * s2, cov = 64 * w.s12 - s1 * s2;
    const int A = 2 * s1 * s2 + kQualitySsimC1, B = 2 * cov + kQualitySsimC2;
    const int C = s1 * s1 + s2 * s2 + kQualitySsimC1, D = vars + kQualitySsimC2;
    const double v = ((double)A * (double)B) / ((double)C * (double)D);
    return (int64_t)llrint(v * 4294967296.0);
}

// ---- kept and static regions (DESIGN.md "Quality metrics", "Regions") ----------
// A pixel has the class of its mask block: 0 kept, 1 static. A set of pixels (a
// cell, a window) is summarised by which classes it holds.
constexpr uint32_t kQualityHasKept = 1, kQualityHasStatic = 2;

// The block rule. any: some mask byte of the block inside the frame is not 0;
// partial: the block crosses the right or bottom edge. fd:117-120 clips the
// block and tests it (partial_static = 1); of:156-161 skips it, so it is kept
// (partial_static = 0).
DVC_HD uint32_t quality_block_static(uint32_t any, bool partial, int partial_static)
{
    return (partial && !partial_static) ? 0u : (any == 0 ? 1u : 0u);
}

// x / B without a divide, for the per-lane block indices: exact for x < 2^17 and
// B in 1..128 (x (magic B - 2^32) <= x B < 2^32). B = 1 has no 32-bit magic.
DVC_HD uint32_t quality_block_magic(int B)
{
    return B == 1 ? 0u : (uint32_t)((1ull << 32) / (uint32_t)B + 1);
}

DVC_HD uint32_t quality_block_of(uint32_t x, uint32_t magic)
{
    return magic ? (uint32_t)(((uint64_t)x * magic) >> 32) : x;
}

// Squared errors of one pixel pair alone, for the pixels of a cell that holds
// both classes.
DVC_HD void quality_px_sse(uint32_t ab, uint32_t ag, uint32_t ar, uint32_t bb, uint32_t bg, uint32_t br,
                           uint32_t (&sse)[4])
{
    const int db = (int)ab - (int)bb, dg = (int)ag - (int)bg, dr = (int)ar - (int)br;
    const int dy = (int)quality_luma(ab, ag, ar) - (int)quality_luma(bb, bg, br);
    sse[0] += (uint32_t)(db * db);
    sse[1] += (uint32_t)(dg * dg);
    sse[2] += (uint32_t)(dr * dr);
    sse[3] += (uint32_t)(dy * dy);
}

// The pixels of cell (x0, y0) that lie inside the frame, bit 4 r + i for (x0 + i, y0 + r).
DVC_HD uint32_t quality_cell_inside(int x0, int y0, int W, int H)
{
    const int nx = W - x0 < 4 ? W - x0 : 4, ny = H - y0 < 4 ? H - y0 : 4;
    const uint32_t row = (1u << nx) - 1;
    return (row | row << 4 | row << 8 | row << 12) & ((1u << 4 * ny) - 1);
}

// Which classes a cell holds: m has a bit per static pixel, inside per pixel in the frame.
DVC_HD uint32_t quality_cell_has(uint32_t m, uint32_t inside)
{
    return ((inside & ~m) ? kQualityHasKept : 0u) | ((inside & m) ? kQualityHasStatic : 0u);
}

// A window holds what its four cells hold (quality_cell_has values, or-ed):
// 0 kept, 1 static, 2 mixed — the index into ssim_q32[] and windows[].
DVC_HD int quality_window_class(uint32_t has)
{
    return has == kQualityHasKept ? 0 : has == kQualityHasStatic ? 1 : 2;
}

}  // namespace dvc
