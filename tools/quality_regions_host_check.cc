// quality_regions_host_check — the quality meter's kept / static split on the CPU.
//
// Compiles csrc/quality_core.h (the block rule, the classes a cell holds, a
// window's class and the per-pixel arithmetic: the text the GPU kernels
// compile) for the host, stand-alone, so that it runs under the host sanitizers:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o quality_regions_host_check tools/quality_regions_host_check.cc
//   quality_regions_host_check IN_DIR
// For every IN_DIR/<name>.dim (text: "W H block partial_static") the frames
// IN_DIR/<name>.ref and IN_DIR/<name>.test (packed BGR, 3*W*H bytes each) are
// compared under the mask IN_DIR/<name>.mask (W*H bytes), and one line
//   <name> sse[0][0..3] sse[1][0..3] ssim_q32[0..2] windows[0..2] pixels[0..1]
// goes to stdout: the sixteen integers of dvc_quality_regions. Frames and mask
// are held in heap blocks of exactly their size, so a read outside one is a
// sanitizer error. The walk is the kernels': blocks, 4x4 cells, 2x2 cells a window.
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../dynamic-video-compression-surveillance_amd/csrc/quality_core.h"

namespace {

uint8_t* read_exact(const std::string& path, size_t n)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return nullptr;
    uint8_t* p = new uint8_t[n];
    const bool ok = std::fread(p, 1, n, f) == n && std::fgetc(f) == EOF;
    std::fclose(f);
    if (!ok) {
        delete[] p;
        return nullptr;
    }
    return p;
}

struct Record {
    uint64_t sse[2][4] = {};
    int64_t q32[3] = {};
    unsigned windows[3] = {}, pixels[2] = {};
};

// One bit per block: static or not.
std::vector<uint8_t> classify(const uint8_t* mask, int W, int H, int B, int partial_static)
{
    const int bw = (W + B - 1) / B, bh = (H + B - 1) / B;
    std::vector<uint8_t> st((size_t)bw * bh);
    for (int by = 0; by < bh; ++by)
        for (int bx = 0; bx < bw; ++bx) {
            uint32_t any = 0;
            for (int y = by * B; y < std::min(by * B + B, H); ++y)
                for (int x = bx * B; x < std::min(bx * B + B, W); ++x) any |= mask[(size_t)y * W + x];
            st[(size_t)by * bw + bx] =
                (uint8_t)dvc::quality_block_static(any, bx * B + B > W || by * B + B > H, partial_static);
        }
    return st;
}

Record compare(const uint8_t* a, const uint8_t* b, const uint8_t* mask, int W, int H, int B, int partial_static)
{
    const int cw = (W + 3) / 4, ch = (H + 3) / 4, fw = W / 4, fh = H / 4, bw = (W + B - 1) / B;
    const std::vector<uint8_t> st = classify(mask, W, H, B, partial_static);
    const uint32_t magic = dvc::quality_block_magic(B);
    std::vector<dvc::QualityCell> cells((size_t)fw * fh);
    std::vector<uint32_t> has((size_t)fw * fh);
    Record r;
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const uint32_t inside = dvc::quality_cell_inside(4 * cx, 4 * cy, W, H);
            uint32_t m = 0;
            for (int k = 0; k < 16; ++k)
                if ((inside >> k) & 1)   // (the kernels' divide-free block index)
                    m |= (uint32_t)st[(size_t)dvc::quality_block_of(4 * cy + k / 4, magic) * bw +
                                      dvc::quality_block_of(4 * cx + k % 4, magic)] << k;
            const uint32_t holds = dvc::quality_cell_has(m, inside);
            uint32_t e[4] = {0, 0, 0, 0}, es[4] = {0, 0, 0, 0};
            dvc::QualityCell c{0, 0, 0, 0};
            for (int k = 0; k < 16; ++k) {
                if (!((inside >> k) & 1)) continue;
                const size_t o = ((size_t)(4 * cy + k / 4) * W + 4 * cx + k % 4) * 3;
                dvc::quality_px(a[o], a[o + 1], a[o + 2], b[o], b[o + 1], b[o + 2], e, c);
                if ((m >> k) & 1) dvc::quality_px_sse(a[o], a[o + 1], a[o + 2], b[o], b[o + 1], b[o + 2], es);
            }
            for (int k = 0; k < 4; ++k) {
                r.sse[0][k] += e[k] - es[k];
                r.sse[1][k] += es[k];
            }
            for (int k = 0; k < 16; ++k) r.pixels[(m >> k) & 1] += (inside >> k) & 1;
            if (cx < fw && cy < fh) {
                cells[(size_t)cy * fw + cx] = c;
                has[(size_t)cy * fw + cx] = holds;
            }
        }
    for (int j = 0; j + 1 < fh; ++j)
        for (int i = 0; i + 1 < fw; ++i) {
            const size_t o = (size_t)j * fw + i;
            const dvc::QualityCell* c = &cells[o];
            const int k = dvc::quality_window_class(has[o] | has[o + 1] | has[o + fw] | has[o + fw + 1]);
            r.q32[k] += dvc::quality_window_q32(dvc::quality_add(dvc::quality_add(c[0], c[1]), dvc::quality_add(c[fw], c[fw + 1])));
            r.windows[k] += 1;
        }
    return r;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s IN_DIR\n", argv[0]);
        return 2;
    }
    const std::string in = argv[1];
    std::vector<std::string> names;
    DIR* d = opendir(in.c_str());
    if (!d) {
        std::perror(in.c_str());
        return 2;
    }
    while (dirent* e = readdir(d)) {
        const std::string n = e->d_name;
        if (n.size() > 4 && n.compare(n.size() - 4, 4, ".dim") == 0) names.push_back(n.substr(0, n.size() - 4));
    }
    closedir(d);
    std::sort(names.begin(), names.end());
    for (const std::string& n : names) {
        int W = 0, H = 0, B = 0, ps = -1;
        FILE* f = std::fopen((in + "/" + n + ".dim").c_str(), "r");
        const bool ok = f && std::fscanf(f, "%d %d %d %d", &W, &H, &B, &ps) == 4 && W >= 8 && H >= 8 && W <= 65535 &&
                        H <= 65535 && B >= 1 && B <= 128 && (ps == 0 || ps == 1);
        if (f) std::fclose(f);
        if (!ok) {
            std::fprintf(stderr, "%s: bad size, block or partial_static\n", n.c_str());
            return 2;
        }
        const size_t px = (size_t)W * H;
        uint8_t *a = read_exact(in + "/" + n + ".ref", 3 * px), *b = read_exact(in + "/" + n + ".test", 3 * px);
        uint8_t* m = read_exact(in + "/" + n + ".mask", px);
        if (!a || !b || !m) {
            std::fprintf(stderr, "%s: frames or mask missing or of another size\n", n.c_str());
            delete[] a;
            delete[] b;
            delete[] m;
            return 2;
        }
        const Record r = compare(a, b, m, W, H, B, ps);
        std::printf("%s", n.c_str());
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < 4; ++k) std::printf(" %llu", (unsigned long long)r.sse[c][k]);
        for (int k = 0; k < 3; ++k) std::printf(" %lld", (long long)r.q32[k]);
        std::printf(" %u %u %u %u %u\n", r.windows[0], r.windows[1], r.windows[2], r.pixels[0], r.pixels[1]);
        delete[] a;
        delete[] b;
        delete[] m;
    }
    return 0;
}
