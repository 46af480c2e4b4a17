// jpeg_kernels.h — baseline-JPEG encoder kernels (DESIGN.md "Motion-JPEG
// stream"). Internal launch interface; the C-ABI is in include/dvc.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_huff_core.h"
#include "jpeg_rate_core.h"
#include "jpeg_stream_core.h"

namespace dvc {

// The most bits one block can take: a DC code (16 + 11 magnitude bits) and 63
// AC codes (16 + 10 each). Runs >= 16 cost less than the coefficients they skip.
constexpr int kJpegMaxBlockBits = 27 + 63 * 26;
// Blocks whose codes k_jpeg_pack assembles in LDS at a time.
constexpr int kJpegChunk = 64;
// The frames of one launch group of the stream output (= DVC_MAX_BATCH).
constexpr int kJpegStreamMaxGroup = 512;

// Per-handle tables in device memory.
struct JpegTables {
    uint16_t q[2][64];   // quantiser, natural order: luma, chroma
    uint32_t dc[12];     // code length << 16 | code, by DC size
    uint32_t ac[256];    // the same by (run << 4 | size); 0x00 EOB, 0xF0 ZRL
    uint8_t zpos[64];    // zigzag position of natural index i
};

// A table group's tables (DVC_FLAG_JPEG_OPT_HUFFMAN), built on the device from
// the group's symbol counts: one DC and one AC table per class (0: luma and
// gray, 1: Cb and Cr), and the DHT + SOS bytes in front of each of its frames.
struct JpegOptTables {
    uint32_t dc[2][12];    // code length << 16 | code by DC size; 0: no code
    uint32_t ac[2][256];
    uint32_t prefix_len;
    uint8_t prefix[(kHuffPrefixCap + 3) & ~3];
};

// The bytes in front of every frame of a group (NULL bytes: none): the DHT + SOS
// of optimised tables, or a rate handle's DQT, DQT, [DHT,] SOS. `len` is
// written on the device by the kernels that build the bytes.
struct JpegPrefix {
    const uint8_t* bytes;
    const uint32_t* len;
    uint32_t cap;
};

// A rate handle's device state (DESIGN.md "Rate target"): what create sets, the
// running search of the current group, the estimate the round's workgroups add
// to, the counters, and the group's prefix.
constexpr int kRatePrefixCap = kRateDqtPairBytes + kHuffPrefixCap;
struct JpegRateState {
    unsigned long long est;     // sum of rate_seg_bytes over the round's segments
    unsigned long long target;  // bytes a frame
    RateSearch search;
    RateStats stats;
    int32_t q_min, q_max;
    uint32_t frame_fixed;       // a fixed-table sample's bytes in front of its entropy data
    uint32_t prefix_len;
    uint8_t base[2][64];        // quantiser base tables, natural order
    uint8_t prefix[(kRatePrefixCap + 3) & ~3];
};

// One frame's geometry. A restart segment is one MCU row: `bps` blocks in scan
// order (colour: Y00 Y01 Y10 Y11 Cb Cr per 16x16 MCU; gray: one 8x8 block per MCU).
struct JpegGeom {
    int W, H;
    int gray;       // 1: DVC_FMT_GRAY
    int mcus_x;     // MCUs per segment
    int nseg;       // segments (MCU rows) per frame
    int bps;        // blocks per segment
    int units_x;    // k_jpeg_dct work units per MCU row (colour: one MCU; gray: four blocks)
    uint32_t segcap;   // bytes of one segment's scratch slot (its worst case, stuffing included)
};

// Work buffers for max_batch frames (frame f's part at index f * per-frame count).
struct JpegBufs {
    int16_t* levels;     // nseg * bps * 64 quantised levels, zigzag order, DC undifferenced
    uint32_t* boff;      // nseg * bps: a block's bit offset inside its segment
    uint32_t* segbits;   // nseg: a segment's bits
    uint32_t* seglen;    // nseg: its bytes after stuffing
    uint8_t* scratch;    // nseg * segcap
    uint32_t* overflow;  // one word: set when a frame did not fit its output slot
    // optimised tables only (NULL otherwise):
    unsigned long long* counts;   // [4][256]: DC class 0, AC class 0, DC class 1, AC class 1
    JpegOptTables* opt;
    JpegPrefix prefix;   // what k_jpeg_gather and the stream kernels put in front of a frame
    // rate handles only (NULL otherwise):
    int16_t* coef;       // nseg * bps * 64 unquantised coefficients, zigzag order
    JpegRateState* rate;
};

// n frames (rows of `pitch` bytes, frames `fstride` apart; BGR or one channel)
// -> levels; on a rate handle (b.rate set) -> coef.
hipError_t jpeg_launch_dct(const uint8_t* frames, size_t pitch, size_t fstride, int n, const JpegGeom& g,
                           const JpegTables* tab, const JpegBufs& b, hipStream_t st);
// Optimised tables: levels of the n frames of a group -> counts (zeroed first).
hipError_t jpeg_launch_hist(int n, const JpegGeom& g, const JpegBufs& b, hipStream_t st);
// counts -> opt (tables), and the DHT + SOS bytes: behind the DQT pair of
// b.rate's prefix when `group` and b.rate is set, into opt's own prefix otherwise.
hipError_t jpeg_launch_huff_build(const JpegGeom& g, const JpegBufs& b, hipStream_t st, bool group = true);
// Rate handles. One round of the search over the n frames of a group: coef at
// the state's quality -> the state's estimate (nothing once the search ended).
hipError_t jpeg_launch_rate_bits(int n, const JpegGeom& g, const JpegTables* tab, const JpegBufs& b, hipStream_t st);
// The search step behind round `round`; the last of `rounds` also leaves the
// chosen quantiser in tab, the DQT pair (and the SOS, without b.opt) in the
// prefix, the counters, and the search ready for the next group.
hipError_t jpeg_launch_rate_step(int n, int round, int rounds, const JpegGeom& g, JpegTables* tab, const JpegBufs& b,
                                 hipStream_t st);
// coef -> levels with tab's quantiser.
hipError_t jpeg_launch_quant(int n, const JpegGeom& g, const JpegTables* tab, const JpegBufs& b, hipStream_t st);
// The three below read b.opt's tables when it is set and `tab`'s fixed ones otherwise.
// levels -> boff, segbits.
hipError_t jpeg_launch_bits(int n, const JpegGeom& g, const JpegTables* tab, const JpegBufs& b, hipStream_t st);
// levels, boff, segbits -> scratch, seglen.
hipError_t jpeg_launch_pack(int n, const JpegGeom& g, const JpegTables* tab, const JpegBufs& b, hipStream_t st);
// scratch, seglen -> out + f * out_stride ([prefix,] segments, RST markers, EOI), sizes[f].
hipError_t jpeg_launch_gather(int n, const JpegGeom& g, const JpegBufs& b, uint8_t* out, size_t out_stride,
                              uint32_t* sizes, hipStream_t st);
// The stream output of one launch group of n <= kJpegStreamMaxGroup frames:
// seglen -> offsets[0..n] behind *carry (0 when `first`; left at the group's
// end), then header, [prefix,] segments, RST markers and EOI of every sample
// that ends inside `cap`, at out + offsets[t] - (rebase ? *rebase : 0).
// header, carry, offsets and rebase are device pointers.
hipError_t jpeg_launch_stream(int n, int first, const JpegGeom& g, const JpegBufs& b, const uint8_t* header,
                              uint32_t header_len, uint64_t* carry, uint64_t* offsets, const uint64_t* rebase,
                              uint8_t* out, uint64_t cap, hipStream_t st);

}  // namespace dvc
