// quality_api.hip — C-ABI of the quality meter (include/dvc.h, dvc_quality_*):
// what a size figure of performance_analysis.py lacks, the distortion of a
// compressed output against its source. The arithmetic is DESIGN.md "Quality
// metrics" (quality_core.h); the kernels are in quality_kernels.hip.
#include "../../include/dvc.h"
#include "../../include/dvc_quality_regions.h"
#include "host_common.h"
#include "quality_kernels.h"

using dvc_host::fail;

static_assert(sizeof(dvc_quality_frame) == sizeof(dvc::QualityFrame) && sizeof(dvc_quality_frame) == 48,
              "quality_kernels.h restates dvc_quality_frame");
static_assert(sizeof(dvc_quality_regions) == sizeof(dvc::QualityRegions) && sizeof(dvc_quality_regions) == 112,
              "quality_kernels.h restates dvc_quality_regions");

struct dvc_quality {
    dvc::QualityGeom g{};
    int device = -1, max_batch = 1;
    uint32_t flags = 0;
    dvc_host::HandleStream stream;   // the caller's (may be NULL = legacy default) or our own
    dvc_host::DevMem mem;
    uint64_t* d_part = nullptr;     // five words per tile and frame
    // host-pointer mode: both staged batches (rows of ip bytes) and the records
    uint8_t *d_a = nullptr, *d_b = nullptr;
    dvc::QualityFrame* d_res = nullptr;
    size_t ip = 0;
    // dvc_quality_compare_regions, allocated by its first call: the class bits (sized for
    // block 1, the most rows), sixteen words per tile and frame, and in host-pointer
    // mode the staged masks (rows of mp bytes) and the records
    uint32_t* d_cls = nullptr;
    uint64_t* d_part_r = nullptr;
    uint8_t* d_m = nullptr;
    dvc::QualityRegions* d_res_r = nullptr;
    size_t mp = 0;

    hipError_t regions_memory()
    {
        if (d_cls) return hipSuccess;
        const size_t mb = max_batch, tiles = (size_t)g.tiles_x * g.tiles_y;
        mp = ((size_t)g.W + 3) & ~(size_t)3;
        hipError_t e = mem.alloc(&d_part_r, mb * tiles * dvc::kQualityRegionParts * sizeof(uint64_t));
        if (e == hipSuccess && !(flags & DVC_FLAG_DEVICE_PTRS)) {
            e = mem.alloc(&d_m, mb * mp * g.H);
            if (e == hipSuccess) e = mem.alloc(&d_res_r, mb * sizeof(dvc::QualityRegions));
        }
        if (e == hipSuccess) e = mem.alloc(&d_cls, mb * dvc::quality_class_words(g.W, g.H, 1) * sizeof(uint32_t));
        return e;
    }
};

extern "C" {

int dvc_quality_create(int width, int height, int max_batch, int device, void* hip_stream, uint32_t flags,
                       dvc_quality** out)
{
    if (!out) return fail(DVC_E_INVALID, "NULL argument");
    *out = nullptr;
    if (width < 8 || height < 8)
        return fail(DVC_E_UNSUPPORTED, "frame %dx%d has no 8x8 window", width, height);
    if (width > 65535 || height > 65535) return fail(DVC_E_INVALID, "frame %dx%d invalid", width, height);
    if (max_batch < 1 || max_batch > DVC_MAX_BATCH) return fail(DVC_E_INVALID, "max_batch %d outside 1..%d", max_batch,
                                                                DVC_MAX_BATCH);
    if (flags & ~(DVC_FLAG_DEVICE_PTRS | DVC_FLAG_JOIN_STREAM)) return fail(DVC_E_INVALID, "unknown flags 0x%x", flags);
    dvc_quality* h = new dvc_quality();
    h->g = dvc::quality_geom(width, height);
    h->device = device;
    h->max_batch = max_batch;
    h->flags = flags;
    h->ip = (3 * (size_t)width + 3) & ~(size_t)3;
    const size_t mb = max_batch, tiles = (size_t)h->g.tiles_x * h->g.tiles_y;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = h->stream.open(hip_stream, flags & DVC_FLAG_JOIN_STREAM);
    if (e == hipSuccess) e = h->mem.alloc(&h->d_part, mb * tiles * 5 * sizeof(uint64_t));
    if (e == hipSuccess && !(flags & DVC_FLAG_DEVICE_PTRS)) {
        e = h->mem.alloc(&h->d_a, mb * h->ip * height);
        if (e == hipSuccess) e = h->mem.alloc(&h->d_b, mb * h->ip * height);
        if (e == hipSuccess) e = h->mem.alloc(&h->d_res, mb * sizeof(dvc::QualityFrame));
    }
    if (e != hipSuccess) {
        delete h;
        return dvc_host::create_failed(e, "quality create");
    }
    *out = h;
    return DVC_OK;
}

int dvc_quality_compare(dvc_quality* h, const uint8_t* ref, size_t ref_pitch, size_t ref_stride, const uint8_t* test,
                        size_t test_pitch, size_t test_stride, int n, dvc_quality_frame* results)
{
    if (!h || !ref || !test || !results) return fail(DVC_E_INVALID, "NULL argument");
    if (n < 1 || n > h->max_batch) return fail(DVC_E_INVALID, "frame count %d outside 1..%d", n, h->max_batch);
    const size_t roww = 3 * (size_t)h->g.W, H = h->g.H;
    if (ref_pitch < roww || test_pitch < roww) return fail(DVC_E_INVALID, "pitch invalid");
    if (n > 1 && (ref_stride < ref_pitch * (H - 1) + roww || test_stride < test_pitch * (H - 1) + roww))
        return fail(DVC_E_INVALID, "frame stride invalid");
    HIP_OK(hipSetDevice(h->device));
    auto* res = reinterpret_cast<dvc::QualityFrame*>(results);
    if (h->flags & DVC_FLAG_DEVICE_PTRS) {
        if ((uintptr_t)results & 7) return fail(DVC_E_INVALID, "results must be 8-byte aligned");
        HIP_OK(dvc::quality_launch(ref, ref_pitch, ref_stride, test, test_pitch, test_stride, n, h->g, h->d_part, res,
                                   h->stream.s));
        return DVC_OK;
    }
    HIP_OK(dvc_host::stage_rows_h2d(h->d_a, h->ip, ref, ref_pitch, ref_stride, roww, H, n, h->stream.s));
    HIP_OK(dvc_host::stage_rows_h2d(h->d_b, h->ip, test, test_pitch, test_stride, roww, H, n, h->stream.s));
    HIP_OK(dvc::quality_launch(h->d_a, h->ip, h->ip * H, h->d_b, h->ip, h->ip * H, n, h->g, h->d_part, h->d_res,
                               h->stream.s));
    HIP_OK(hipMemcpyAsync(res, h->d_res, n * sizeof(dvc::QualityFrame), hipMemcpyDeviceToHost, h->stream.s));
    HIP_OK(hipStreamSynchronize(h->stream.s));
    return DVC_OK;
}

int dvc_quality_compare_regions(dvc_quality* h, const uint8_t* ref, size_t ref_pitch, size_t ref_stride,
                                const uint8_t* test, size_t test_pitch, size_t test_stride, const uint8_t* mask,
                                size_t mask_pitch, size_t mask_stride, int block, int partial_static, int n,
                                dvc_quality_regions* results)
{
    if (!h || !ref || !test || !mask || !results) return fail(DVC_E_INVALID, "NULL argument");
    if (n < 1 || n > h->max_batch) return fail(DVC_E_INVALID, "frame count %d outside 1..%d", n, h->max_batch);
    if (block < 1 || block > dvc::kQualityMaxBlock)
        return fail(DVC_E_INVALID, "block %d outside 1..%d", block, dvc::kQualityMaxBlock);
    if (partial_static != 0 && partial_static != 1)
        return fail(DVC_E_INVALID, "partial_static %d is neither 0 nor 1", partial_static);
    const size_t W = h->g.W, roww = 3 * W, H = h->g.H;
    if (ref_pitch < roww || test_pitch < roww || mask_pitch < W) return fail(DVC_E_INVALID, "pitch invalid");
    if (n > 1 && (ref_stride < ref_pitch * (H - 1) + roww || test_stride < test_pitch * (H - 1) + roww ||
                  mask_stride < mask_pitch * (H - 1) + W))
        return fail(DVC_E_INVALID, "frame stride invalid");
    const bool dev = h->flags & DVC_FLAG_DEVICE_PTRS;
    if (dev && ((uintptr_t)results & 7)) return fail(DVC_E_INVALID, "results must be 8-byte aligned");
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(h->regions_memory());
    auto* res = reinterpret_cast<dvc::QualityRegions*>(results);
    if (dev) {
        HIP_OK(dvc::quality_launch_regions(ref, ref_pitch, ref_stride, test, test_pitch, test_stride, mask, mask_pitch,
                                           mask_stride, block, partial_static, n, h->g, h->d_cls, h->d_part_r, res,
                                           h->stream.s));
        return DVC_OK;
    }
    HIP_OK(dvc_host::stage_rows_h2d(h->d_a, h->ip, ref, ref_pitch, ref_stride, roww, H, n, h->stream.s));
    HIP_OK(dvc_host::stage_rows_h2d(h->d_b, h->ip, test, test_pitch, test_stride, roww, H, n, h->stream.s));
    HIP_OK(dvc_host::stage_rows_h2d(h->d_m, h->mp, mask, mask_pitch, mask_stride, W, H, n, h->stream.s));
    HIP_OK(dvc::quality_launch_regions(h->d_a, h->ip, h->ip * H, h->d_b, h->ip, h->ip * H, h->d_m, h->mp, h->mp * H,
                                       block, partial_static, n, h->g, h->d_cls, h->d_part_r, h->d_res_r, h->stream.s));
    HIP_OK(hipMemcpyAsync(res, h->d_res_r, n * sizeof(dvc::QualityRegions), hipMemcpyDeviceToHost, h->stream.s));
    HIP_OK(hipStreamSynchronize(h->stream.s));
    return DVC_OK;
}

int dvc_quality_sync(dvc_quality* h)
{
    if (!h) return fail(DVC_E_INVALID, "NULL handle");
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(h->stream.s));
    return DVC_OK;
}

void dvc_quality_destroy(dvc_quality* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream.s);
    delete h;
}

}  // extern "C"
