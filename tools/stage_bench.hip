// stage_bench.hip — profiling harness (not part of the product): runs the FD
// kernels of fd_kernels.hip stage by stage, each stage alone on the device
// (synchronised between stages), over one batch of n synthetic frames, so a
// rocprofv3 kernel trace shows every kernel's isolated duration.
//   stage_bench W H n reps frames.raw [fused]   (frames.raw: n+1 packed BGR frames;
//   fused = 1: the fused front's speculative outputs + k_fix4, as the handle runs
//   block_size 4 with BGR frames)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dynamic-video-compression-surveillance_amd/csrc/fd_kernels.h"

#define CK(x)                                                                            \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            std::fprintf(stderr, "%s: %s (%d)\n", #x, hipGetErrorString(e_), __LINE__);  \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s W H n reps frames.raw\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), n = std::atoi(argv[3]), reps = std::atoi(argv[4]);
    const bool fused = argc > 6 && std::atoi(argv[6]) != 0;
    const size_t F = (size_t)3 * W * H, N = (size_t)W * H;
    std::vector<uint8_t> host(F * (n + 1));
    FILE* fp = std::fopen(argv[5], "rb");
    if (!fp || std::fread(host.data(), 1, host.size(), fp) != host.size()) {
        std::fprintf(stderr, "cannot read %s\n", argv[5]);
        return 2;
    }
    std::fclose(fp);
    dvc::RowGeom g{W, H, (W + 63) / 64, W / 2 + 1};
    uint8_t *frames, *gray0, *gray1, *gtmp, *acc, *ov, *cp;
    uint32_t* tmp32;
    unsigned long long* stats;
    CK(hipMalloc(&frames, host.size()));
    CK(hipMemcpy(frames, host.data(), host.size(), hipMemcpyHostToDevice));
    CK(hipMalloc(&gray0, N));
    CK(hipMalloc(&gray1, N));
    CK(hipMalloc(&gtmp, N));
    CK(hipMalloc(&tmp32, 4 * N));
    CK(hipMalloc(&acc, N + 4 * (size_t)W));
    CK(hipMalloc(&ov, F * n));
    CK(hipMalloc(&cp, F * n));
    CK(hipMalloc(&stats, 8 * 4 * 64));
    CK(hipMemset(acc, 0, N));
    dvc::CclBufs c{};
    size_t sz[dvc::CclBufs::NARR];
    dvc::CclBufs::sizes(g, n, sz);
    void** ptrs[dvc::CclBufs::NARR];
    c.ptrs(ptrs);
    for (int i = 0; i < dvc::CclBufs::NARR; ++i) CK(hipMalloc(ptrs[i], sz[i]));
    CK(hipMemset(c.gpar, 0, sz[dvc::CclBufs::I_GPAR]));
    c.stats = stats;
    CK(hipMalloc(&c.kocc, (size_t)H * n));   // sparse kept rows, as the handle runs it
    const int B = 4, NBX = (W + B - 1) / B, NBY = (H + B - 1) / B, SW = (NBX + 63) / 64, gs = (W + 3) & ~3;
    uint64_t *dblk, *rblk, *sbits;
    CK(hipMalloc(&dblk, 2 * (size_t)NBX * NBY * n));
    CK(hipMalloc(&rblk, 2 * (size_t)NBX * NBY * n));
    CK(hipMalloc(&sbits, 8 * (size_t)NBY * SW * n));
    dvc::GaussTaps kp{};
    kp.n = 25;
    // taps for (25, 30.0) as the handle computes them (dvc_gaussian_taps_q8)
    const uint16_t t25[25] = {10, 10, 10, 10, 10, 10, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 10, 10, 10, 10, 10, 10};
    for (int i = 0; i < 25; ++i) kp.t[i] = t25[i];
    CK(dvc::launch_prime(frames, 3 * W, gtmp, tmp32, gray0, W, H, gs, kp, nullptr));
    dvc::BackArgs a{};
    a.g = g;
    a.bgr = frames + F;
    a.pitch = 3 * W;
    a.fstride = F;
    a.acc = acc;
    a.ap = NBX * B;
    a.B = B;
    a.NBX = NBX;
    a.NBY = NBY;
    a.overlay = ov;
    a.compressed = cp;
    a.opitch = 3 * W;
    a.ostride = F;
    a.kbits = c.kbits;
    a.kocc = c.kocc;
    CK(hipMalloc(&a.docc, (size_t)NBY * n));
    a.dblk = dblk;
    a.rblk = rblk;
    a.sbits = sbits;
    a.SW = SW;
    a.sstride = (size_t)NBY * SW;
    a.n = n;
    a.ksize = 7;
    a.anchor = 3;
    a.alpha = 0.5f;
    a.beta = 0.5f;
    a.gamma = 0.f;
    a.quant = 100.f;
    a.qinv = 1.0 / 100.0;
    a.acc0_fixed = 1;
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 4; ++j)
            a.M.m[k * 4 + j] = a.M.mt[j * 4 + k] = (float)((k == 0 ? std::sqrt(0.25) : std::sqrt(0.5)) * std::cos(M_PI * (2 * j + 1) * k / 8.0));
    a.stats = stats;
    unsigned long long* err;
    CK(hipMalloc(&err, 8));
    CK(hipMemset(err, 0xff, 8));
    a.err = err;
    double tf = 0, tc = 0, tb = 0;
    for (int r = 0; r < reps; ++r) {
        CK(hipDeviceSynchronize());
        auto t0 = std::chrono::steady_clock::now();
        // rep 0 starts from the 25x25-blurred prime gray (a near-full first mask);
        // later reps continue from the previous rep's last gray like a feed would
        dvc::FrontOut fo{ov, cp, 3 * W, F, 100.f, 1.0 / 100.0, a.M};
        CK(dvc::launch_front(frames + F, 3 * W, F, dvc::SrcFmt{0, 0, 0, 0}, n, (r & 1) ? gray1 : gray0, (r & 1) ? gray0 : gray1, gs, c.mbits, g,
                             0, nullptr, fused ? &fo : nullptr));
        CK(hipDeviceSynchronize());
        auto t1 = std::chrono::steady_clock::now();
        CK(dvc::launch_ccl(c, g, n, 1000, nullptr));
        CK(hipDeviceSynchronize());
        auto t2 = std::chrono::steady_clock::now();
        CK(dvc::launch_accumulate(a, nullptr));
        CK(hipDeviceSynchronize());
        CK(dvc::launch_out(a, nullptr, fused));
        CK(hipDeviceSynchronize());
        auto t3 = std::chrono::steady_clock::now();
        if (r > 0) {
            tf += std::chrono::duration<double>(t1 - t0).count();
            tc += std::chrono::duration<double>(t2 - t1).count();
            tb += std::chrono::duration<double>(t3 - t2).count();
        }
    }
    const double k = 1e6 / ((reps - 1) * (double)n);
    std::printf("per frame (us, host wall incl. launch): front %.2f  ccl %.2f  back %.2f  total %.2f\n", tf * k,
                tc * k, tb * k, (tf + tc + tb) * k);
    return 0;
}
