// host_common.hip — the host plumbing of host_common.h. No kernels.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "dct_const.h"
#include "host_common.h"

namespace dvc_host {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char* last_error() { return g_err.c_str(); }

int create_failed(hipError_t e, const char* what)
{
    return fail(e == hipErrorOutOfMemory ? DVC_E_NOMEM : DVC_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

// getGaussianKernelBitExact in double (OpenCV 4.11): the small binomial tables
// for sigma <= 0 and n <= 7, else exp(-x^2 / 2 sigma^2) normalised with the
// centre tap 1/sum. The float kernels of getGaussianKernel(CV_32F) are these
// values cast to float.
void gauss_f64(int n, double sigma, double* k)
{
    if (sigma <= 0 && n <= 7) {
        static const double t1[] = {1.0};
        static const double t3[] = {0.25, 0.5, 0.25};
        static const double t5[] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
        static const double t7[] = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125};
        const double* t = n == 1 ? t1 : n == 3 ? t3 : n == 5 ? t5 : t7;
        for (int i = 0; i < n; ++i) k[i] = t[i];
        return;
    }
    double sx = sigma > 0 ? sigma : std::fma((double)n, 0.15, 0.35);
    double scale2X = -0.125 / (sx * sx);
    int n2 = (n - 1) / 2;
    double vals[64], sum = 0.0;
    for (int i = 0, x = 1 - n; i < n2; ++i, x += 2) {
        vals[i] = std::exp((double)(x * x) * scale2X);
        sum += vals[i];
    }
    sum = sum * 2.0 + 1.0;
    double mul1 = 1.0 / sum;
    for (int i = 0; i < n2; ++i) k[i] = k[n - 1 - i] = vals[i] * mul1;
    k[n2] = mul1;
}

int gauss_taps(int n, double sigma, uint16_t* taps)
{
    if (n < 1 || n > 63 || (n & 1) == 0) return -1;
    double k[64];
    gauss_f64(n, sigma, k);
    int n2 = n / 2;
    double err = 0.0;
    long long s = 0;
    for (int i = 0; i < n2; ++i) {
        double adj = k[i] * 256.0 + err;
        double v0 = std::nearbyint(adj);
        err = adj - v0;
        taps[i] = taps[n - 1 - i] = (uint16_t)v0;
        s += (long long)v0;
    }
    taps[n2] = (uint16_t)(256 - 2 * s);
    return 0;
}

void dct_basis(int n, float* m)
{
    const double PI = 3.14159265358979323846;
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < n; ++j) {
            const double c = k == 0 ? std::sqrt(1.0 / n) : std::sqrt(2.0 / n);
            m[k * n + j] = (float)(c * std::cos(PI * (2 * j + 1) * k / (2.0 * n)));
        }
}

void dct_matrix(int B, dvc::DctMat& M)
{
    // the fast block sizes take the compiled tables (dct_const.h), so the host
    // basis and the kernels' constant basis cannot differ on a host whose libm
    // cos rounds differently
    if (B == 4 || B == 8) {
        const float* t = B == 4 ? dvc::kDct4Host : dvc::kDct8Host;
        std::memcpy(M.m, t, sizeof(float) * B * B);
        std::memcpy(M.mt, t + B * B, sizeof(float) * B * B);
        return;
    }
    dct_basis(B, M.m);
    for (int k = 0; k < B; ++k)
        for (int n = 0; n < B; ++n) M.mt[n * B + k] = M.m[k * B + n];
}

hipError_t DevMem::event(hipEvent_t* ev)
{
    const hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e == hipSuccess) events.push_back(*ev);
    return e;
}

void DevMem::release(void* p)
{
    for (size_t i = 0; i < dev.size(); ++i)
        if (p && dev[i] == p) {
            (void)hipFree(p);
            dev.erase(dev.begin() + (long)i);
            return;
        }
}

void DevMem::free_all()
{
    for (void* p : dev) (void)hipFree(p);
    for (void* p : pinned) (void)hipHostFree(p);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    dev.clear();
    pinned.clear();
    events.clear();
}

hipError_t HandleStream::open(void* hip_stream, bool join_null)
{
    if (hip_stream || join_null) {
        s = (hipStream_t)hip_stream;
        return hipSuccess;
    }
    const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    own = e == hipSuccess;
    return e;
}

void HandleStream::close()
{
    if (own && s) (void)hipStreamDestroy(s);
    s = nullptr;
    own = false;
}

hipError_t stage_rows_h2d(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t pitch, size_t stride, size_t roww,
                          size_t H, int n, hipStream_t stream)
{
    const bool packed = pitch == roww && roww == dpitch;
    if (packed && (n == 1 || stride == roww * H))
        return hipMemcpyAsync(dst, src, (size_t)n * roww * H, hipMemcpyHostToDevice, stream);
    hipError_t e = hipSuccess;
    for (int t = 0; t < n && e == hipSuccess; ++t) {
        const uint8_t* s = src + (size_t)t * stride;
        uint8_t* d = dst + (size_t)t * dpitch * H;
        e = packed ? hipMemcpyAsync(d, s, roww * H, hipMemcpyHostToDevice, stream)
                   : hipMemcpy2DAsync(d, dpitch, s, pitch, roww, H, hipMemcpyHostToDevice, stream);
    }
    return e;
}

hipError_t fork_streams(hipStream_t user, hipEvent_t ev, std::initializer_list<hipStream_t> streams)
{
    hipError_t e = hipEventRecord(ev, user);
    for (hipStream_t st : streams)
        if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
    return e;
}

hipError_t sync_streams(std::initializer_list<hipStream_t> streams)
{
    hipError_t e = hipSuccess;
    for (hipStream_t st : streams)
        if (e == hipSuccess && st) e = hipStreamSynchronize(st);
    return e;
}

double ktime_sum(const std::vector<hipEvent_t>& ev, size_t used, hipError_t* err)
{
    double t = 0.0;
    *err = hipSuccess;
    for (size_t i = 0; i + 1 < used && *err == hipSuccess; i += 2) {
        float ms = 0.f;
        *err = hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
        t += ms;
    }
    return t;
}

hipError_t fold_stats(const unsigned long long* dev, unsigned long long s[4])
{
    unsigned long long slots[64 * 4];
    const hipError_t e = hipMemcpy(slots, dev, sizeof(slots), hipMemcpyDeviceToHost);
    for (int i = 0; i < 4; ++i) s[i] = 0;
    for (int i = 0; i < 64 * 4 && e == hipSuccess; ++i) s[i % 4] += slots[i];
    return e;
}

hipError_t read_bit_plane(const uint64_t* src, size_t W, size_t H, size_t WW, uint8_t* dst)
{
    std::vector<uint64_t> bits(H * WW);
    const hipError_t e = hipMemcpy(bits.data(), src, 8 * H * WW, hipMemcpyDeviceToHost);
    if (e == hipSuccess) expand_bit_plane(bits.data(), W, H, WW, dst);
    return e;
}

}  // namespace dvc_host

// ---- include/dvc_stream.h: a stream several handles join, for callers without a HIP binding ----
#include "../../include/dvc_stream.h"

extern "C" {

int dvc_stream_create(int device, void** stream)
{
    if (!stream) return dvc_host::fail(DVC_E_INVALID, "NULL argument");
    *stream = nullptr;
    HIP_OK(hipSetDevice(device));
    hipStream_t s = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return DVC_OK;
}

int dvc_stream_destroy(int device, void* stream)
{
    if (!stream) return DVC_OK;
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    HIP_OK(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return DVC_OK;
}

}  // extern "C"
