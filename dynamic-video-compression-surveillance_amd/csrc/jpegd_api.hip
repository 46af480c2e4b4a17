// jpegd_api.hip — C-ABI of the Motion-JPEG decoder (include/dvc.h, dvc_jpegd_*):
// what the reference's cap.read() (frame_differencing.py:86-87;
// motion_compression_opt.py:66, 142-143) does with one sample of a Motion-JPEG
// file. The arithmetic is DESIGN.md "Motion-JPEG decoder"; the kernels are in
// jpegd_kernels.hip, the header parser in jpegd_header.h.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dvc.h"
#include "host_common.h"
#include "jpegd_header.h"
#include "jpegd_kernels.h"

using dvc_host::fail;

static_assert(dvc::kJpegdInvalid == DVC_E_INVALID && dvc::kJpegdUnsupported == DVC_E_UNSUPPORTED &&
                  dvc::kJpegdDamaged == DVC_E_INVALID,
              "jpegd_header.h / jpegd_core.h restate the status codes");

struct dvc_jpegd {
    int max_w = 0, max_h = 0, max_batch = 1, device = -1;
    uint32_t flags = 0;
    bool have_header = false, tab_dirty = false;
    dvc::JpegdHeader hdr{};
    dvc_host::HandleStream stream;   // the caller's (may be NULL = legacy default) or our own
    dvc_host::DevMem mem;
    dvc::JpegdTables* d_tab = nullptr;
    dvc::JpegdBufs b{};
    // host-pointer mode: staged samples (slots of in_slot bytes), sizes, packed output frames, statuses
    uint8_t *d_in = nullptr, *d_out = nullptr;
    uint32_t* d_sizes = nullptr;
    int32_t* d_status = nullptr;
    size_t in_slot = 0;
};

static size_t up(size_t v, size_t m) { return (v + m - 1) / m * m; }

extern "C" {

int dvc_jpegd_create(int max_width, int max_height, int max_batch, int device, void* hip_stream, uint32_t flags,
                     dvc_jpegd** out)
{
    if (!out) return fail(DVC_E_INVALID, "NULL argument");
    if (max_width < 1 || max_height < 1 || max_width > 65535 || max_height > 65535)
        return fail(DVC_E_INVALID, "largest frame %dx%d invalid", max_width, max_height);
    if (max_batch < 0 || max_batch > DVC_MAX_BATCH) return fail(DVC_E_INVALID, "max_batch %d outside 1..%d", max_batch,
                                                                DVC_MAX_BATCH);
    const size_t yw = up(max_width, 16), yh = up(max_height, 16);
    // 4:2:0, the larger of the two layouts; a camera handle's largest is 4:4:4's three full planes
    const size_t ncoef = (flags & DVC_FLAG_JPEGD_CAMERA) ? yw * yh * 3 : yw * yh * 3 / 2;
    const size_t nmark = up(max_width, 8) / 8 * (up(max_height, 8) / 8);         // one MCU per segment, one component
    if (ncoef * 2 > 0x7fffffffull) return fail(DVC_E_UNSUPPORTED, "largest frame %dx%d too large", max_width, max_height);
    dvc_jpegd* h = new dvc_jpegd();
    h->max_w = max_width;
    h->max_h = max_height;
    h->max_batch = max_batch ? max_batch : 1;
    h->device = device;
    h->flags = flags;
    *out = h;
    if (device < 0) return DVC_OK;   // host-only handle: dvc_jpegd_set_header alone
    *out = nullptr;
    const size_t mb = h->max_batch;
    hipError_t e = hipSetDevice(device);
    dvc_host::DevMem& mem = h->mem;
    if (e == hipSuccess) e = h->stream.open(hip_stream, flags & DVC_FLAG_JOIN_STREAM);
    if (e == hipSuccess) e = mem.alloc(&h->d_tab, sizeof(dvc::JpegdTables));
    if (e == hipSuccess) e = mem.alloc(&h->b.coef, mb * ncoef * sizeof(int16_t));
    if (e == hipSuccess) e = mem.alloc(&h->b.chunkcnt, mb * dvc::kJpegdChunks * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(&h->b.markpos, mb * nmark * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(&h->b.planes, mb * ncoef);
    if (e == hipSuccess) e = mem.alloc(&h->b.first_err, sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->b.first_err, 0, sizeof(int32_t));
    if (e == hipSuccess && !(flags & DVC_FLAG_DEVICE_PTRS)) {
        e = mem.alloc(&h->d_out, mb * 3 * (size_t)max_width * max_height);
        if (e == hipSuccess) e = mem.alloc(&h->d_sizes, mb * sizeof(uint32_t));
        if (e == hipSuccess) e = mem.alloc(&h->d_status, mb * sizeof(int32_t));
    }
    if (e != hipSuccess) {
        delete h;
        return dvc_host::create_failed(e, "jpegd create");
    }
    *out = h;
    return DVC_OK;
}

int dvc_jpegd_set_header(dvc_jpegd* h, const uint8_t* hdr, size_t n, size_t* header_len, int* width, int* height,
                         int* fmt)
{
    if (!h || !hdr) return fail(DVC_E_INVALID, "NULL argument");
    dvc::JpegdHeader parsed;
    const char* why = "";
    const int rc = dvc::jpegd_parse_header(hdr, n, &parsed, &why, (h->flags & DVC_FLAG_JPEGD_CAMERA) != 0);
    if (rc != dvc::kJpegdOk) return fail(rc, "JPEG header: %s", why);
    if (parsed.g.W > h->max_w || parsed.g.H > h->max_h)
        return fail(DVC_E_INVALID, "frame %dx%d exceeds the handle's %dx%d", parsed.g.W, parsed.g.H, h->max_w, h->max_h);
    h->hdr = parsed;
    h->have_header = true;
    h->tab_dirty = true;
    if (header_len) *header_len = parsed.length;
    if (width) *width = parsed.g.W;
    if (height) *height = parsed.g.H;
    if (fmt) *fmt = parsed.g.gray ? DVC_FMT_GRAY : DVC_FMT_BGR;
    return DVC_OK;
}

int dvc_jpegd_decode(dvc_jpegd* h, const uint8_t* data, size_t data_stride, const uint32_t* sizes, int n, uint8_t* out,
                     size_t pitch, size_t frame_stride, int32_t* status)
{
    if (!h || !data || !sizes || !out || !status) return fail(DVC_E_INVALID, "NULL argument");
    if (h->device < 0) return fail(DVC_E_STATE, "a host-only handle cannot decode");
    if (!h->have_header) return fail(DVC_E_STATE, "dvc_jpegd_decode before dvc_jpegd_set_header");
    if (n < 0) return fail(DVC_E_INVALID, "negative frame count");
    const dvc::JpegdGeom& g = h->hdr.g;
    const size_t roww = (size_t)(g.gray ? 1 : 3) * g.W, H = g.H;
    if (pitch < roww) return fail(DVC_E_INVALID, "pitch invalid");
    if (n > 1 && frame_stride < pitch * (H - 1) + roww) return fail(DVC_E_INVALID, "frame stride invalid");
    HIP_OK(hipSetDevice(h->device));
    hipStream_t st = h->stream.s;
    if (h->tab_dirty) {   // (pageable source: the runtime has taken its copy when the call returns)
        HIP_OK(hipMemcpyAsync(h->d_tab, &h->hdr.t, sizeof(dvc::JpegdTables), hipMemcpyHostToDevice, st));
        h->tab_dirty = false;
    }
    const bool devp = h->flags & DVC_FLAG_DEVICE_PTRS;
    int first = 0;
    std::vector<int32_t> hst((size_t)h->max_batch);
    for (int f0 = 0; f0 < n; f0 += h->max_batch) {
        const int m = std::min(h->max_batch, n - f0);
        const uint8_t* in = data + (size_t)f0 * data_stride;
        uint8_t* o = out + (size_t)f0 * frame_stride;
        if (devp) {
            HIP_OK(dvc::jpegd_launch(in, data_stride, sizes + f0, m, g, h->d_tab, h->b, o, pitch, frame_stride,
                                     status + f0, st));
            continue;
        }
        uint32_t big = 0;
        for (int t = 0; t < m; ++t) {
            if (n > 1 && sizes[f0 + t] > data_stride) return fail(DVC_E_INVALID, "a frame's size exceeds data_stride");
            big = std::max(big, sizes[f0 + t]);
        }
        const size_t slot = up(std::max<size_t>(big, 4), 256);
        if (slot > h->in_slot) {   // the staging area grows to the largest sample seen
            HIP_OK(hipStreamSynchronize(st));
            h->mem.release(h->d_in);
            h->d_in = nullptr;
            h->in_slot = 0;
            const hipError_t e = h->mem.alloc(&h->d_in, slot * h->max_batch);
            if (e != hipSuccess) return fail(DVC_E_NOMEM, "jpegd staging: %s", hipGetErrorString(e));
            h->in_slot = slot;
        }
        for (int t = 0; t < m; ++t)
            if (sizes[f0 + t])
                HIP_OK(hipMemcpyAsync(h->d_in + t * h->in_slot, in + (size_t)t * data_stride, sizes[f0 + t],
                                      hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(h->d_sizes, sizes + f0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        const size_t fbytes = roww * H;
        HIP_OK(dvc::jpegd_launch(h->d_in, h->in_slot, h->d_sizes, m, g, h->d_tab, h->b, h->d_out, roww, fbytes,
                                 h->d_status, st));
        HIP_OK(hipMemcpyAsync(hst.data(), h->d_status, m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (int t = 0; t < m; ++t) {
            status[f0 + t] = hst[t];
            if (hst[t] != 0) {
                if (!first) first = hst[t];
                continue;   // a damaged frame's slot is left as it was
            }
            uint8_t* dst = o + (size_t)t * frame_stride;
            if (pitch == roww)
                HIP_OK(hipMemcpyAsync(dst, h->d_out + t * fbytes, fbytes, hipMemcpyDeviceToHost, st));
            else
                HIP_OK(hipMemcpy2DAsync(dst, pitch, h->d_out + t * fbytes, roww, roww, H, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipStreamSynchronize(st));
    }
    if (!devp) {   // reported here, not again by dvc_jpegd_sync
        HIP_OK(hipMemsetAsync(h->b.first_err, 0, sizeof(int32_t), st));
        if (first) return fail(first, "a frame's entropy data is damaged (status[] names the frames)");
    }
    return DVC_OK;
}

int dvc_jpegd_sync(dvc_jpegd* h)
{
    if (!h) return fail(DVC_E_INVALID, "NULL handle");
    if (h->device < 0) return DVC_OK;
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(h->stream.s));
    if (h->flags & DVC_FLAG_DEVICE_PTRS) {   // a damaged frame of an asynchronous call is reported here, once
        int32_t err = 0;
        HIP_OK(hipMemcpy(&err, h->b.first_err, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (err) {
            HIP_OK(hipMemset(h->b.first_err, 0, sizeof(int32_t)));
            return fail(err, "a frame's entropy data was damaged (status[] names the frames)");
        }
    }
    return DVC_OK;
}

void dvc_jpegd_destroy(dvc_jpegd* h)
{
    if (!h) return;
    if (h->device >= 0) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream.s);
    }
    delete h;
}

}  // extern "C"
