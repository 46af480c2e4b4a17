// host_frames_check — the frame contract of csrc/host_frames.h on the CPU.
//
// Stand-alone, so that it runs under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o host_frames_check tools/host_frames_check.cc
//   host_frames_check
// Every source frame is a heap block of exactly frame_span() bytes (byte i =
// 7 i + 3 mod 256) and every destination a heap block of exactly the packed
// size (filled with 0xee), so a read or a write one byte past either is a
// sanitizer error. One line per result goes to stdout: "span <case> <bytes>",
// "pack <case> <hex of the destination>", "pitch_ok <fmt> <w> <pitch> <0|1>".
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../dynamic-video-compression-surveillance_amd/csrc/host_frames.h"

using dvc_host::FrameFmt;

namespace {

void print_hex(const char* what, int id, const uint8_t* p, size_t n)
{
    std::printf("%s %d ", what, id);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}

void pack_case(int id, const FrameFmt& f, size_t pitch, size_t dst_bgr_pitch, size_t dst_bytes)
{
    const size_t span = dvc_host::frame_span(f, pitch);
    uint8_t* src = static_cast<uint8_t*>(std::malloc(span));
    uint8_t* dst = static_cast<uint8_t*>(std::malloc(dst_bytes));
    for (size_t i = 0; i < span; ++i) src[i] = (uint8_t)(7 * i + 3);
    for (size_t i = 0; i < dst_bytes; ++i) dst[i] = 0xee;
    dvc_host::pack_host_frame(f, src, pitch, dst, dst_bgr_pitch);
    std::printf("span %d %zu\n", id, span);
    print_hex("pack", id, dst, dst_bytes);
    std::free(src);
    std::free(dst);
}

void pitch_case(int fmt, int w, size_t pitch)
{
    std::printf("pitch_ok %d %d %zu %d\n", fmt, w, pitch, (int)dvc_host::pitch_ok(FrameFmt{fmt, w, 4, 4}, pitch));
}

}  // namespace

int main()
{
    pack_case(1, FrameFmt{DVC_FMT_BGR, 10, 6, 0}, 37, 36, 36 * 5 + 30);
    pack_case(2, FrameFmt{DVC_FMT_I420, 6, 4, 6}, 10, 0, 36);
    pack_case(3, FrameFmt{DVC_FMT_NV12, 6, 4, 4}, 9, 0, 36);
    {   // case 4: a bit plane of W = 70, H = 3 in rows of WW = 2 words
        const size_t W = 70, H = 3, WW = 2;
        uint64_t* bits = static_cast<uint64_t*>(std::calloc(H * WW, sizeof(uint64_t)));
        uint8_t* dst = static_cast<uint8_t*>(std::malloc(W * H));
        for (size_t y = 0; y < H; ++y)
            for (size_t x : {0, 63, 64, 69}) bits[y * WW + x / 64] |= 1ull << (x % 64);
        dvc_host::expand_bit_plane(bits, W, H, WW, dst);
        print_hex("pack", 4, dst, W * H);
        std::free(bits);
        std::free(dst);
    }
    pitch_case(DVC_FMT_BGR, 10, 29);
    pitch_case(DVC_FMT_BGR, 10, 30);
    pitch_case(DVC_FMT_I420, 6, 7);
    pitch_case(DVC_FMT_I420, 6, 8);
    pitch_case(DVC_FMT_NV12, 6, 7);
    return 0;
}
