// quality_host_check — the quality meter's arithmetic on the CPU.
//
// Compiles csrc/quality_core.h (the luma, a pixel pair's contribution and the
// 8x8 window value: the text the GPU kernels compile) for the host, stand-alone,
// so that it runs under the host sanitizers:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o quality_host_check tools/quality_host_check.cc
//   quality_host_check IN_DIR
// For every IN_DIR/<name>.dim (text: "W H") the frames IN_DIR/<name>.ref and
// IN_DIR/<name>.test (packed BGR, 3*W*H bytes each) are compared, and one line
//   <name> sse_b sse_g sse_r sse_y ssim_q32 windows pixels
// goes to stdout: the seven integers of dvc_quality_frame. The frames are held
// in heap blocks of exactly their size, so a read outside either one is a
// sanitizer error. The walk is the kernel's: 4x4 cells, then 2x2 cells a window.
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

void compare(const uint8_t* a, const uint8_t* b, int W, int H, uint64_t (&sse)[4], int64_t* q32)
{
    const int cw = (W + 3) / 4, ch = (H + 3) / 4, fw = W / 4, fh = H / 4;
    std::vector<dvc::QualityCell> cells((size_t)fw * fh);
    for (int k = 0; k < 4; ++k) sse[k] = 0;
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            uint32_t e[4] = {0, 0, 0, 0};
            dvc::QualityCell c{0, 0, 0, 0};
            for (int y = 4 * cy; y < std::min(4 * cy + 4, H); ++y)
                for (int x = 4 * cx; x < std::min(4 * cx + 4, W); ++x) {
                    const uint8_t *p = a + ((size_t)y * W + x) * 3, *q = b + ((size_t)y * W + x) * 3;
                    dvc::quality_px(p[0], p[1], p[2], q[0], q[1], q[2], e, c);
                }
            for (int k = 0; k < 4; ++k) sse[k] += e[k];
            if (cx < fw && cy < fh) cells[(size_t)cy * fw + cx] = c;
        }
    *q32 = 0;
    for (int j = 0; j + 1 < fh; ++j)
        for (int i = 0; i + 1 < fw; ++i) {
            const dvc::QualityCell* c = &cells[(size_t)j * fw + i];
            *q32 += dvc::quality_window_q32(dvc::quality_add(dvc::quality_add(c[0], c[1]), dvc::quality_add(c[fw], c[fw + 1])));
        }
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
        int W = 0, H = 0;
        FILE* f = std::fopen((in + "/" + n + ".dim").c_str(), "r");
        const bool ok = f && std::fscanf(f, "%d %d", &W, &H) == 2 && W >= 8 && H >= 8 && W <= 65535 && H <= 65535;
        if (f) std::fclose(f);
        if (!ok) {
            std::fprintf(stderr, "%s: bad size\n", n.c_str());
            return 2;
        }
        const size_t bytes = (size_t)W * H * 3;
        uint8_t *a = read_exact(in + "/" + n + ".ref", bytes), *b = read_exact(in + "/" + n + ".test", bytes);
        if (!a || !b) {
            std::fprintf(stderr, "%s: frames missing or not 3*W*H bytes\n", n.c_str());
            delete[] a;
            delete[] b;
            return 2;
        }
        uint64_t sse[4];
        int64_t q32;
        compare(a, b, W, H, sse, &q32);
        std::printf("%s %llu %llu %llu %llu %lld %u %u\n", n.c_str(), (unsigned long long)sse[0],
                    (unsigned long long)sse[1], (unsigned long long)sse[2], (unsigned long long)sse[3], (long long)q32,
                    (unsigned)(W / 4 - 1) * (unsigned)(H / 4 - 1), (unsigned)W * (unsigned)H);
        delete[] a;
        delete[] b;
    }
    return 0;
}
