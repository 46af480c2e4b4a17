// host_common.h — the host plumbing every C-ABI source shares (fd_api.hip,
// of_api.hip, jpeg_api.hip, jpegd_api.hip, quality_api.hip, yuv_kernels.hip,
// diag.hip): the error text, the filter and DCT tables, what a handle owns
// (device memory, pinned memory, events, its stream) and the copies and
// read-backs more than one handle makes. Defined in host_common.hip; the frame
// contract is host_frames.h. Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <vector>

#include "fd_kernels.h"
#include "host_frames.h"

namespace dvc_host {

// Set the calling thread's dvc_last_error() text; returns `code`.
int fail(int code, const char* fmt, ...);
const char* last_error();
// A create call's failed HIP call `what`: DVC_E_NOMEM or DVC_E_HIP, with the
// runtime's text. The caller deletes its handle.
int create_failed(hipError_t e, const char* what);

// getGaussianKernelBitExact values in double (n odd <= 63).
void gauss_f64(int n, double sigma, double* k);
// ... and getGaussianKernelFixedPoint_ED (8 fraction bits): the taps OpenCV's
// 8U GaussianBlur uses (fd:77, fd:93). -1: n even or outside 1..63.
int gauss_taps(int n, double sigma, uint16_t* taps);
// n x n orthonormal DCT-II basis m[k][j], float32 of the double cos form.
void dct_basis(int n, float* m);
// BxB basis and its transpose: the compiled tables of dct_const.h for the fast
// block sizes (4, 8), dct_basis otherwise.
void dct_matrix(int B, dvc::DctMat& M);

// What a handle allocated: freed together, when the handle goes (or by
// free_all). Handles hold one by value and are never copied.
struct DevMem {
    std::vector<void*> dev, pinned;
    std::vector<hipEvent_t> events;

    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { free_all(); }

    // device memory (at least 16 bytes), or page-locked host memory
    template <class T>
    hipError_t alloc(T** p, size_t bytes, bool host = false)
    {
        void* q = nullptr;
        const hipError_t e = host ? hipHostMalloc(&q, bytes) : hipMalloc(&q, bytes ? bytes : 16);
        if (e == hipSuccess) {
            (host ? pinned : dev).push_back(q);
            *p = static_cast<T*>(q);
        }
        return e;
    }
    template <class T>
    hipError_t alloc_pinned(T** p, size_t bytes) { return alloc(p, bytes, true); }
    hipError_t event(hipEvent_t* ev);   // an ordering event (no timing)
    void release(void* p);              // one device buffer, ahead of the rest (NULL: nothing)
    void free_all();
};

// The stream a single-stream handle works on: the caller's — create's
// hip_stream, or with join_null also a NULL one, the legacy default stream
// (DVC_FLAG_JOIN_STREAM) — or a non-blocking stream of its own.
struct HandleStream {
    hipStream_t s = nullptr;
    bool own = false;

    HandleStream() = default;
    HandleStream(const HandleStream&) = delete;
    HandleStream& operator=(const HandleStream&) = delete;
    ~HandleStream() { close(); }

    hipError_t open(void* hip_stream, bool join_null);
    void close();
};

// n host frames (rows of roww bytes, `pitch` apart, frames `stride` apart) up
// into device rows of dpitch bytes: a packed batch in one copy, packed frames
// in one copy each (a 2-D copy of pageable memory goes row by row), anything
// else as 2-D copies.
hipError_t stage_rows_h2d(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t pitch, size_t stride, size_t roww,
                          size_t H, int n, hipStream_t stream);

// The caller's stream -> a handle's internal streams: work the caller queued
// before a call (the copy that produced the frames, reads of the previous
// outputs) happens before the call's kernels.
hipError_t fork_streams(hipStream_t user, hipEvent_t ev, std::initializer_list<hipStream_t> streams);
hipError_t sync_streams(std::initializer_list<hipStream_t> streams);

// Sum of the KTIMING event pairs ev[0..used), in ms.
double ktime_sum(const std::vector<hipEvent_t>& ev, size_t used, hipError_t* err);
// The 64 x 4 statistics slots the kernels spread their atomics over, folded.
hipError_t fold_stats(const unsigned long long* dev, unsigned long long s[4]);
// A device bit plane (host_frames.h expand_bit_plane) into W x H bytes of 0 / 255.
hipError_t read_bit_plane(const uint64_t* src, size_t W, size_t H, size_t WW, uint8_t* dst);

}  // namespace dvc_host

#define HIP_OK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return dvc_host::fail(DVC_E_HIP, "%s failed: %s (%s:%d)", #expr,                  \
                                  hipGetErrorString(e_), __FILE__, __LINE__);                 \
    } while (0)
