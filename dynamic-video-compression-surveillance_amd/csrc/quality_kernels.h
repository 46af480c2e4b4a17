// quality_kernels.h — quality-meter kernels (DESIGN.md "Quality metrics").
// Internal launch interface; the C-ABI is in include/dvc.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quality_core.h"

namespace dvc {

// A workgroup's tile: kQualityTileCX x kQualityTileCY cells of 4x4 pixels
// (128 x 32 pixels), one lane per cell, plus the column of cells to its right
// and the row below for the windows that start in the tile.
constexpr int kQualityTileCX = 32, kQualityTileCY = 8;
constexpr int kQualityTileW = 4 * kQualityTileCX, kQualityTileH = 4 * kQualityTileCY;
// a workgroup's squared-error partials are 32-bit: its tile's pixels, 65025 each at the most
static_assert(65025ull * kQualityTileW * kQualityTileH < (1ull << 32), "a tile's SSE partial must fit 32 bits");

struct QualityGeom {
    int W, H;
    int cells_x, cells_y;   // cells that hold a pixel: ceil(W / 4), ceil(H / 4)
    int full_x, full_y;     // cells wholly inside the frame: W / 4, H / 4 (the cells windows are made of)
    int tiles_x, tiles_y;
};

inline QualityGeom quality_geom(int W, int H)
{
    QualityGeom g{};
    g.W = W;
    g.H = H;
    g.cells_x = (W + 3) / 4;
    g.cells_y = (H + 3) / 4;
    g.full_x = W / 4;
    g.full_y = H / 4;
    g.tiles_x = (g.cells_x + kQualityTileCX - 1) / kQualityTileCX;
    g.tiles_y = (g.cells_y + kQualityTileCY - 1) / kQualityTileCY;
    return g;
}

// What dvc_quality_frame is (include/dvc.h), restated for the kernels.
struct QualityFrame {
    uint64_t sse[4];
    int64_t ssim_q32;
    uint32_t windows, pixels;
};

// n frame pairs (frame t at a + t * a_stride and b + t * b_stride, rows of
// a_pitch / b_pitch bytes) -> results[0..n). partials: n * tiles_x * tiles_y * 5
// words of workspace. All pointers are device pointers.
hipError_t quality_launch(const uint8_t* a, size_t a_pitch, size_t a_stride, const uint8_t* b, size_t b_pitch,
                          size_t b_stride, int n, const QualityGeom& g, uint64_t* partials, QualityFrame* results,
                          hipStream_t st);

// ---- kept and static regions ----------------------------------------------------
// What dvc_quality_regions is (include/dvc.h).
struct QualityRegions {
    uint64_t sse[2][4];
    int64_t ssim_q32[3];
    uint32_t windows[3];
    uint32_t pixels[2];
    uint32_t reserved;
};

// The class bits of a frame: one bit per pixel column and block row (every pixel
// row of a block row has the same bits), ceil(H / block) rows of ceil(W / 32)
// words; bit x % 32 of word x / 32 is set where the column's block is static.
constexpr int kQualityRegionParts = 16;   // words per tile and frame (k_quality_tile_regions)
constexpr int kQualityMaxBlock = 128;
inline size_t quality_class_words(int W, int H, int block)
{
    return (size_t)((H + block - 1) / block) * (size_t)((W + 31) / 32);
}

// quality_launch with a mask frame per pair (frame t at mask + t * m_stride, rows
// of m_pitch >= W bytes) -> results[0..n). cls: n * quality_class_words words,
// partials: n * tiles_x * tiles_y * kQualityRegionParts words of workspace.
hipError_t quality_launch_regions(const uint8_t* a, size_t a_pitch, size_t a_stride, const uint8_t* b, size_t b_pitch,
                                  size_t b_stride, const uint8_t* mask, size_t m_pitch, size_t m_stride, int block,
                                  int partial_static, int n, const QualityGeom& g, uint32_t* cls, uint64_t* partials,
                                  QualityRegions* results, hipStream_t st);

}  // namespace dvc
