// acc_fast_host_check — k_acc's short form against its clamped form, on the CPU.
//
// Compiles csrc/fd_kernels.h for the host, stand-alone, and executes the
// argument stated at acc_fast_ok: wherever the predicate holds for a triple
// (alpha, beta, gamma), the short form
//     rint(fmaf(acc, alpha, bit ? fmaf(255, beta, gamma) : +0))      (no clamp)
// is a byte value and equals the general form
//     min(max(rint(fmaf(acc, alpha, fmaf(bit ? 255 : 0, beta, gamma))), 0), 255)
// on all 512 inputs (acc 0..255, dilated bit 0 / 1), and acc_zero_fixed holds.
//   c++ -std=c++17 -O1 -g -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I<ROCm>/include \
//       [-fsanitize=address,undefined -fno-sanitize-recover=all] \
//       -o acc_fast_host_check tools/acc_fast_host_check.cc
//   acc_fast_host_check ROWS
// ROWS is text, one named triple a line, the floats as their 32 bits in hex
// (NaN, -0 and denormals arrive as they are):
//   <name> <alpha bits> <beta bits> <gamma bits>
// The sweep is those rows, then
//   * (r, 1 - r, 0) for r = i / 65536, i = 0..65536, and for the 16 floats on
//     either side of 0, 0.5 and 1 (1 - r in double, as the host derives it);
//   * every triple over a set of special values: +-0, denormals, FLT_MIN,
//     ordinary weights, FLT_MAX, +-inf, NaN;
//   * raw grids: alpha in [0, 1.25], beta in [-0.25, 1.25] (so that
//     d1 = fmaf(255, beta, gamma) lies on both sides of 0 and of 255) with
//     gamma = +0 and -0, and gamma in [-64, 320] with a few betas.
// One JSON object goes to stdout: the predicate and acc_zero_fixed of every
// named row, the number of triples swept, how many the predicate accepted, and
// the number of failures (the first ones are described on stderr). The exit
// status is 1 if there was a failure.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../dynamic-video-compression-surveillance_amd/csrc/fd_kernels.h"

static float from_bits(uint32_t b)
{
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

static uint32_t to_bits(float f)
{
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

static uint64_t g_swept, g_fast, g_fail;

static void fail(float al, float be, float ga, const char* what, int acc, int bit, float s, int g)
{
    if (g_fail++ < 16)
        std::fprintf(stderr, "alpha %a beta %a gamma %a (%08x %08x %08x): %s at acc %d bit %d: short %a general %d\n",
                     (double)al, (double)be, (double)ga, to_bits(al), to_bits(be), to_bits(ga), what, acc, bit,
                     (double)s, g);
}

static void check(float al, float be, float ga)
{
    ++g_swept;
    if (!dvc::acc_fast_ok(al, be, ga)) return;
    ++g_fast;
    if (!dvc::acc_zero_fixed(al, be, ga)) fail(al, be, ga, "acc_fast_ok without acc_zero_fixed", 0, 0, 0.f, 0);
    const float dil0 = std::fmaf(0.f, be, ga), dil1 = std::fmaf(255.f, be, ga);
    for (int bit = 0; bit < 2; ++bit)
        for (int acc = 0; acc < 256; ++acc) {
            const float s = std::rint(std::fmaf((float)acc, al, bit ? dil1 : 0.0f));
            const float c = std::fmin(std::fmax(std::rint(std::fmaf((float)acc, al, bit ? dil1 : dil0)), 0.f), 255.f);
            const int g = (int)c;   // c is in [0, 255]: fmax(NaN, 0) = 0
            if (!(s >= 0.f && s <= 255.f)) fail(al, be, ga, "short form is no byte value", acc, bit, s, g);
            else if ((int)s != g) fail(al, be, ga, "short form != general form", acc, bit, s, g);
        }
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s ROWS\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::printf("{\"rows\": {");
    char name[128];
    uint32_t ab, bb, gb;
    bool first = true;
    while (std::fscanf(f, "%127s %" SCNx32 " %" SCNx32 " %" SCNx32, name, &ab, &bb, &gb) == 4) {
        const float al = from_bits(ab), be = from_bits(bb), ga = from_bits(gb);
        std::printf("%s\"%s\": {\"fast\": %d, \"acc0_fixed\": %d}", first ? "" : ", ", name,
                    (int)dvc::acc_fast_ok(al, be, ga), (int)dvc::acc_zero_fixed(al, be, ga));
        first = false;
        check(al, be, ga);
    }
    std::fclose(f);

    // (r, 1 - r, 0): the grid and the neighbours of 0, 0.5 and 1
    auto ref = [](float r) { check(r, (float)(1.0 - (double)r), 0.0f); };
    for (int i = 0; i <= 65536; ++i) ref((float)(i / 65536.0));
    for (float c : {0.0f, 0.5f, 1.0f}) {
        float lo = c, hi = c;
        for (int k = 0; k < 16; ++k) {
            lo = std::nextafter(lo, -2.0f);
            hi = std::nextafter(hi, 2.0f);
            ref(lo);
            ref(hi);
        }
    }
    // special values in every position
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float dmin = std::numeric_limits<float>::denorm_min(), fmin_ = std::numeric_limits<float>::min();
    const float fmax_ = std::numeric_limits<float>::max();
    const std::vector<float> sp = {0.0f, -0.0f, dmin, -dmin, fmin_ - dmin, -(fmin_ - dmin), fmin_, -fmin_,
                                   0.25f, 0.5f, 0.75f, 1.0f, -0.5f, -1.0f, 1.0f / 255.0f, 255.0f, -255.0f,
                                   fmax_, -fmax_, inf, -inf, nan, -nan};
    for (float al : sp)
        for (float be : sp)
            for (float ga : sp) check(al, be, ga);
    // raw grids: d1 = fmaf(255, beta, gamma) on both sides of 0 and of 255
    for (int ia = 0; ia <= 40; ++ia)
        for (int ib = -64; ib <= 320; ++ib)
            for (float ga : {0.0f, -0.0f}) check((float)(ia / 32.0), (float)(ib / 256.0), ga);
    for (float al : {0.0f, 0.5f, 1.0f})
        for (float be : {-0.25f, 0.0f, 0.5f, 1.0f})
            for (int ig = -256; ig <= 1280; ++ig) check(al, be, (float)(ig / 4.0));
    // alpha + beta just above 1 at d1 near 255: the last term of the predicate
    for (int ia = 0; ia <= 64; ++ia)
        for (int k = -8; k <= 8; ++k) {
            float be = (float)(1.0 - ia / 64.0);
            for (int j = 0; j < (k < 0 ? -k : k); ++j) be = std::nextafter(be, k < 0 ? -2.0f : 2.0f);
            check((float)(ia / 64.0), be, 0.0f);
        }
    std::printf("}, \"swept\": %" PRIu64 ", \"fast\": %" PRIu64 ", \"failures\": %" PRIu64 "}\n", g_swept, g_fast, g_fail);
    return g_fail ? 1 : 0;
}
