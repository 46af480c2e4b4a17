// jpeg_api.hip — C-ABI of the Motion-JPEG encoder (include/dvc.h, dvc_jpeg_*):
// what the reference's cv2.VideoWriter does with every written frame
// (frame_differencing.py:63-65,112,131; motion_compression_opt.py:50-52,99-100,
// 135-136,185), as baseline JPEG instead of MPEG-4 Part 2. The stream format is
// DESIGN.md "Motion-JPEG stream"; the kernels are in jpeg_kernels.hip.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dvc.h"
#include "../../include/dvc_jpeg_opt.h"
#include "../../include/dvc_jpeg_rate.h"
#include "../../include/dvc_jpeg_stream.h"
#include "host_common.h"
#include "jpeg_kernels.h"
#include "jpeg_tables.h"

using dvc_host::fail;

namespace {

// Worst-case bytes of one restart segment of `bps` blocks: every byte stuffed.
uint64_t seg_cap(uint64_t bps) { return 2 * ((bps * dvc::kJpegMaxBlockBits + 7) / 8); }

bool geometry(int width, int height, int fmt, dvc::JpegGeom* g)
{
    if (width < 1 || height < 1 || width > 65520 || height > 65520) return false;
    if (fmt != DVC_FMT_BGR && fmt != DVC_FMT_GRAY) return false;
    const int gray = fmt == DVC_FMT_GRAY, m = gray ? 8 : 16;
    g->W = width;
    g->H = height;
    g->gray = gray;
    g->mcus_x = (width + m - 1) / m;
    g->nseg = (height + m - 1) / m;
    g->bps = g->mcus_x * (gray ? 1 : 6);
    g->units_x = gray ? (g->mcus_x + 3) / 4 : g->mcus_x;
    g->segcap = (uint32_t)seg_cap((uint64_t)g->bps);
    return true;
}

// Worst-case entropy bytes of a frame: its segments, their RST markers, EOI.
uint64_t frame_bound(const dvc::JpegGeom& g) { return (uint64_t)g.nseg * ((uint64_t)g.segcap + 2); }

void quant_table(const uint8_t* base, int quality, uint16_t* q)
{
    for (int i = 0; i < 64; ++i) q[i] = dvc::rate_quant(base[i], quality);
}

// Canonical codes from a DHT's BITS / HUFFVAL, as a decoder derives them.
void canonical(const uint8_t* bits, const uint8_t* vals, uint32_t* table)
{
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code) table[vals[k]] = (uint32_t)len << 16 | code;
        code <<= 1;
    }
}

void fill_tables(int quality, dvc::JpegTables* t)
{
    using namespace dvc_jpeg_tab;
    std::memset(t, 0, sizeof(*t));
    quant_table(kBaseLuma, quality, t->q[0]);
    quant_table(kBaseChroma, quality, t->q[1]);
    canonical(kDcBits, kDcVals, t->dc);
    canonical(kAcBits, kAcVals, t->ac);
    for (int k = 0; k < 64; ++k) t->zpos[kZigzag[k]] = (uint8_t)k;
}

void put16(std::vector<uint8_t>& v, unsigned x)
{
    v.push_back((uint8_t)(x >> 8));
    v.push_back((uint8_t)x);
}

// SOI, APP0 JFIF, 2 x DQT, SOF0, 2 x DHT, DRI, SOS header; with optimised
// tables the DHT and SOS segments are not here but in front of every frame, and
// on a rate handle the DQT and SOS segments.
std::vector<uint8_t> make_header(const dvc::JpegGeom& g, const dvc::JpegTables& t, bool opt, bool rate = false)
{
    using namespace dvc_jpeg_tab;
    std::vector<uint8_t> v = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int id = 0; id < 2 && !rate; ++id) {
        v.insert(v.end(), {0xff, 0xdb, 0, 67, (uint8_t)id});
        for (int k = 0; k < 64; ++k) v.push_back((uint8_t)t.q[id][kZigzag[k]]);
    }
    const int nc = g.gray ? 1 : 3;
    v.insert(v.end(), {0xff, 0xc0});
    put16(v, 8 + 3 * nc);
    v.push_back(8);
    put16(v, g.H);
    put16(v, g.W);
    v.push_back((uint8_t)nc);
    for (int c = 0; c < nc; ++c) v.insert(v.end(), {(uint8_t)(c + 1), (uint8_t)(c == 0 && !g.gray ? 0x22 : 0x11), (uint8_t)(c ? 1 : 0)});
    const struct {
        uint8_t id;
        const uint8_t *bits, *vals;
        int n;
    } dht[2] = {{0x00, kDcBits, kDcVals, 12}, {0x10, kAcBits, kAcVals, 162}};
    for (const auto& d : dht) {
        if (opt) break;
        v.insert(v.end(), {0xff, 0xc4});
        put16(v, 2 + 1 + 16 + d.n);
        v.push_back(d.id);
        v.insert(v.end(), d.bits, d.bits + 16);
        v.insert(v.end(), d.vals, d.vals + d.n);
    }
    v.insert(v.end(), {0xff, 0xdd, 0, 4});
    put16(v, g.mcus_x);
    if (opt || rate) return v;
    v.insert(v.end(), {0xff, 0xda});
    put16(v, 6 + 2 * nc);
    v.push_back((uint8_t)nc);
    for (int c = 0; c < nc; ++c) v.insert(v.end(), {(uint8_t)(c + 1), 0x00});
    v.insert(v.end(), {0, 63, 0});
    return v;
}

}  // namespace

struct dvc_jpeg {
    dvc::JpegGeom g{};
    dvc::JpegTables tab{};
    std::vector<uint8_t> header;
    int device = -1, max_batch = 1, chan = 3;
    uint32_t flags = 0;
    uint64_t bound = 0;
    dvc_host::HandleStream stream;   // the caller's (may be NULL = legacy default) or our own
    dvc_host::DevMem mem;
    dvc::JpegTables* d_tab = nullptr;
    dvc::JpegBufs b{};
    // host-pointer mode: staged frames (rows of ip bytes), output slots, sizes
    uint8_t *d_in = nullptr, *d_out = nullptr;
    uint32_t* d_sizes = nullptr;
    size_t ip = 0;
    // stream output (dvc_jpeg_encode_stream): the header on the device (uploaded by
    // the first call), the end of the launch groups so far, and in host-pointer
    // mode one group's samples and offsets (allocated by the first call)
    uint8_t* d_header = nullptr;
    bool header_up = false;
    uint64_t* d_carry = nullptr;
    uint8_t* d_sout = nullptr;
    uint64_t* d_offs = nullptr;
    // rate handles (dvc_jpeg_create_rate): b.rate is set, the search has `rounds` rounds
    int rounds = 0;
};

namespace {

// One launch group (m <= max_batch frames, one table group) up to its packed
// segments: frames [staged ->] levels -> [tables ->] boff, segbits -> scratch, seglen;
// on a rate handle frames -> coef -> the group's quality -> levels.
int pack_group(dvc_jpeg* h, const uint8_t* in, size_t pitch, size_t frame_stride, int m)
{
    const dvc::JpegGeom& g = h->g;
    hipStream_t st = h->stream.s;
    const uint8_t* kd = in;
    size_t kp = pitch, kfs = frame_stride;
    if (!(h->flags & DVC_FLAG_DEVICE_PTRS)) {   // frames up, rows of ip bytes
        HIP_OK(dvc_host::stage_rows_h2d(h->d_in, h->ip, in, pitch, frame_stride, (size_t)h->chan * g.W, g.H, m, st));
        kd = h->d_in;
        kp = h->ip;
        kfs = h->ip * g.H;
    }
    HIP_OK(dvc::jpeg_launch_dct(kd, kp, kfs, m, g, h->d_tab, h->b, st));
    if (h->b.rate) {   // the same launches whatever the data: the search runs on the device
        for (int r = 0; r < h->rounds; ++r) {
            HIP_OK(dvc::jpeg_launch_rate_bits(m, g, h->d_tab, h->b, st));
            HIP_OK(dvc::jpeg_launch_rate_step(m, r, h->rounds, g, h->d_tab, h->b, st));
        }
        HIP_OK(dvc::jpeg_launch_quant(m, g, h->d_tab, h->b, st));
    }
    if (h->b.opt) {   // this run of frames is one table group
        HIP_OK(dvc::jpeg_launch_hist(m, g, h->b, st));
        HIP_OK(dvc::jpeg_launch_huff_build(g, h->b, st));
    }
    HIP_OK(dvc::jpeg_launch_bits(m, g, h->d_tab, h->b, st));
    HIP_OK(dvc::jpeg_launch_pack(m, g, h->d_tab, h->b, st));
    return DVC_OK;
}

}  // namespace

extern "C" {

int dvc_jpeg_bound(int width, int height, int fmt, size_t* bytes)
{
    dvc::JpegGeom g{};
    if (!bytes) return fail(DVC_E_INVALID, "NULL argument");
    if (!geometry(width, height, fmt, &g)) return fail(DVC_E_INVALID, "frame %dx%d format %d invalid", width, height, fmt);
    *bytes = (size_t)frame_bound(g);
    return DVC_OK;
}

namespace {

// dvc_jpeg_create (target_bytes 0: one quality = q_min = q_max) and dvc_jpeg_create_rate.
int create(int width, int height, int fmt, size_t target_bytes, int q_min, int q_max, int max_batch, int device,
           void* hip_stream, uint32_t flags, dvc_jpeg** out)
{
    const bool rate = target_bytes != 0;
    const int quality = q_min;
    if (!out) return fail(DVC_E_INVALID, "NULL argument");
    if (fmt == DVC_FMT_I420 || fmt == DVC_FMT_NV12)
        return fail(DVC_E_UNSUPPORTED, "the encoder takes DVC_FMT_BGR or DVC_FMT_GRAY frames (JFIF is full-range)");
    dvc::JpegGeom g{};
    if (!geometry(width, height, fmt, &g)) return fail(DVC_E_INVALID, "frame %dx%d format %d invalid", width, height, fmt);
    if (!rate && (quality < 1 || quality > 100)) return fail(DVC_E_INVALID, "quality %d outside 1..100", quality);
    if (rate && (q_min < 1 || q_max > 100 || q_min > q_max))
        return fail(DVC_E_INVALID, "quality range %d..%d outside 1 <= q_min <= q_max <= 100", q_min, q_max);
    if (max_batch < 0 || max_batch > DVC_MAX_BATCH) return fail(DVC_E_INVALID, "max_batch %d outside 1..%d", max_batch,
                                                                DVC_MAX_BATCH);
    const bool opt = flags & DVC_FLAG_JPEG_OPT_HUFFMAN;
    const uint64_t bound = frame_bound(g) + (rate ? DVC_JPEG_RATE_PREFIX_MAX : opt ? DVC_JPEG_OPT_PREFIX_MAX : 0);   // what a frame's slot may need
    if (bound > 0x7fffffffull) return fail(DVC_E_UNSUPPORTED, "frame %dx%d too large", width, height);
    dvc_jpeg* h = new dvc_jpeg();
    h->g = g;
    h->device = device;
    h->max_batch = max_batch ? max_batch : 1;
    h->flags = flags;
    h->chan = g.gray ? 1 : 3;
    h->bound = bound;
    fill_tables(quality, &h->tab);
    h->header = make_header(g, h->tab, opt, rate);
    h->rounds = rate ? dvc::rate_rounds(q_min, q_max) : 0;
    *out = h;
    if (device < 0) return DVC_OK;   // host-only handle: dvc_jpeg_header alone
    *out = nullptr;
    hipError_t e = hipSetDevice(device);
    const size_t mb = h->max_batch, nblk = (size_t)g.nseg * g.bps, nseg = g.nseg;
    h->ip = ((size_t)h->chan * g.W + 3) & ~(size_t)3;
    dvc_host::DevMem& mem = h->mem;
    if (e == hipSuccess) e = h->stream.open(hip_stream, flags & DVC_FLAG_JOIN_STREAM);
    if (e == hipSuccess) e = mem.alloc(&h->d_tab, sizeof(dvc::JpegTables));
    if (e == hipSuccess) e = hipMemcpy(h->d_tab, &h->tab, sizeof(dvc::JpegTables), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mem.alloc(&h->b.levels, mb * nblk * 64 * sizeof(int16_t));
    if (e == hipSuccess) e = mem.alloc(&h->b.boff, mb * nblk * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(&h->b.segbits, mb * nseg * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(&h->b.seglen, mb * nseg * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(&h->b.scratch, mb * nseg * (size_t)g.segcap);
    if (e == hipSuccess) e = mem.alloc(&h->b.overflow, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(h->b.overflow, 0, sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(&h->d_header, h->header.size());
    if (e == hipSuccess) e = mem.alloc(&h->d_carry, sizeof(uint64_t));
    if (e == hipSuccess && opt) {
        e = mem.alloc(&h->b.counts, dvc::kHuffTables * 256 * sizeof(unsigned long long));
        if (e == hipSuccess) e = mem.alloc(&h->b.opt, sizeof(dvc::JpegOptTables));
        if (e == hipSuccess) e = hipMemset(h->b.opt, 0, sizeof(dvc::JpegOptTables));
        if (e == hipSuccess) h->b.prefix = {h->b.opt->prefix, &h->b.opt->prefix_len, (uint32_t)dvc::kHuffPrefixCap};
    }
    if (e == hipSuccess && rate) {
        dvc::JpegRateState rs{};
        rs.target = target_bytes;
        rs.q_min = q_min;
        rs.q_max = q_max;
        rs.frame_fixed = (uint32_t)make_header(g, h->tab, false).size();
        std::memcpy(rs.base[0], dvc_jpeg_tab::kBaseLuma, 64);
        std::memcpy(rs.base[1], dvc_jpeg_tab::kBaseChroma, 64);
        dvc::rate_search_begin(&rs.search, q_min);
        e = mem.alloc(&h->b.coef, mb * nblk * 64 * sizeof(int16_t));
        if (e == hipSuccess) e = mem.alloc(&h->b.rate, sizeof(dvc::JpegRateState));
        if (e == hipSuccess) e = hipMemcpy(h->b.rate, &rs, sizeof(rs), hipMemcpyHostToDevice);
        if (e == hipSuccess) h->b.prefix = {h->b.rate->prefix, &h->b.rate->prefix_len, (uint32_t)dvc::kRatePrefixCap};
    }
    if (e == hipSuccess && !(flags & DVC_FLAG_DEVICE_PTRS)) {
        e = mem.alloc(&h->d_in, mb * h->ip * g.H);   // staged frames
        if (e == hipSuccess) e = mem.alloc(&h->d_out, mb * (size_t)h->bound);
        if (e == hipSuccess) e = mem.alloc(&h->d_sizes, mb * sizeof(uint32_t));
    }
    if (e != hipSuccess) {
        delete h;
        return dvc_host::create_failed(e, "jpeg create");
    }
    *out = h;
    return DVC_OK;
}

}  // namespace

int dvc_jpeg_create(int width, int height, int fmt, int quality, int max_batch, int device, void* hip_stream,
                    uint32_t flags, dvc_jpeg** out)
{
    return create(width, height, fmt, 0, quality, quality, max_batch, device, hip_stream, flags, out);
}

int dvc_jpeg_create_rate(int width, int height, int fmt, size_t target_bytes, int q_min, int q_max, int max_batch,
                         int device, void* hip_stream, uint32_t flags, dvc_jpeg** out)
{
    if (!target_bytes) return fail(DVC_E_INVALID, "a target of 0 bytes a frame");
    return create(width, height, fmt, target_bytes, q_min, q_max, max_batch, device, hip_stream, flags, out);
}

int dvc_jpeg_rate_stats(dvc_jpeg* h, struct dvc_jpeg_rate_stats* out)
{
    if (!h || !out) return fail(DVC_E_INVALID, "NULL argument");
    if (h->device < 0 || !h->b.rate) return fail(DVC_E_STATE, "the counters need a device handle of dvc_jpeg_create_rate");
    static_assert(sizeof(struct dvc_jpeg_rate_stats) == sizeof(dvc::RateStats), "the counters' layout");
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(h->stream.s));
    HIP_OK(hipMemcpy(out, &h->b.rate->stats, sizeof(*out), hipMemcpyDeviceToHost));
    return DVC_OK;
}

int dvc_jpeg_header(const dvc_jpeg* h, uint8_t* dst, size_t cap, size_t* n)
{
    if (!h || !n) return fail(DVC_E_INVALID, "NULL argument");
    *n = h->header.size();
    if (!dst) return DVC_OK;   // size query
    if (cap < h->header.size()) return fail(DVC_E_NOMEM, "header needs %zu bytes, %zu given", h->header.size(), cap);
    std::memcpy(dst, h->header.data(), h->header.size());
    return DVC_OK;
}

int dvc_jpeg_encode(dvc_jpeg* h, const uint8_t* frames, size_t pitch, size_t frame_stride, int n, uint8_t* out,
                    size_t out_stride, uint32_t* sizes)
{
    if (!h || !frames || !out || !sizes) return fail(DVC_E_INVALID, "NULL argument");
    if (h->device < 0) return fail(DVC_E_STATE, "a host-only handle cannot encode");
    if (n < 0) return fail(DVC_E_INVALID, "negative frame count");
    const dvc::JpegGeom& g = h->g;
    const size_t roww = (size_t)h->chan * g.W, H = g.H;
    if (pitch < roww) return fail(DVC_E_INVALID, "pitch invalid");
    if (n > 1 && frame_stride < pitch * (H - 1) + roww) return fail(DVC_E_INVALID, "frame stride invalid");
    HIP_OK(hipSetDevice(h->device));
    const bool devp = h->flags & DVC_FLAG_DEVICE_PTRS;
    hipStream_t st = h->stream.s;
    bool overflow = false;
    std::vector<uint32_t> hs((size_t)h->max_batch);
    for (int f0 = 0; f0 < n; f0 += h->max_batch) {
        const int m = std::min(h->max_batch, n - f0);
        const uint8_t* in = frames + (size_t)f0 * frame_stride;
        uint8_t* o = out + (size_t)f0 * out_stride;
        if (const int rc = pack_group(h, in, pitch, frame_stride, m)) return rc;
        if (devp) {
            HIP_OK(dvc::jpeg_launch_gather(m, g, h->b, o, out_stride, sizes + f0, st));
            continue;
        }
        const size_t slot = (size_t)std::min<uint64_t>(out_stride, h->bound);
        uint32_t hov = 0;
        HIP_OK(dvc::jpeg_launch_gather(m, g, h->b, h->d_out, slot, h->d_sizes, st));
        HIP_OK(hipMemcpyAsync(hs.data(), h->d_sizes, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(&hov, h->b.overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (hov) {
            overflow = true;
            HIP_OK(hipMemsetAsync(h->b.overflow, 0, sizeof(uint32_t), st));
        }
        for (int t = 0; t < m; ++t) {
            sizes[f0 + t] = hs[t];
            if (hs[t] <= slot)
                HIP_OK(hipMemcpyAsync(o + (size_t)t * out_stride, h->d_out + t * slot, hs[t], hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipStreamSynchronize(st));
    }
    if (overflow) return fail(DVC_E_NOMEM, "a frame's data exceeds out_stride %zu (sizes hold the needed lengths)",
                              out_stride);
    return DVC_OK;
}

int dvc_jpeg_encode_stream(dvc_jpeg* h, const uint8_t* frames, size_t pitch, size_t frame_stride, int n, uint8_t* out,
                           size_t cap, uint64_t* offsets)
{
    if (!h || !frames || !out || !offsets) return fail(DVC_E_INVALID, "NULL argument");
    if (h->device < 0) return fail(DVC_E_STATE, "a host-only handle cannot encode");
    if (n < 0) return fail(DVC_E_INVALID, "negative frame count");
    const dvc::JpegGeom& g = h->g;
    const size_t roww = (size_t)h->chan * g.W, H = g.H;
    if (pitch < roww) return fail(DVC_E_INVALID, "pitch invalid");
    if (n > 1 && frame_stride < pitch * (H - 1) + roww) return fail(DVC_E_INVALID, "frame stride invalid");
    const bool devp = h->flags & DVC_FLAG_DEVICE_PTRS;
    if (devp && ((uintptr_t)offsets & 7)) return fail(DVC_E_INVALID, "offsets not aligned to 8 bytes");
    HIP_OK(hipSetDevice(h->device));
    hipStream_t st = h->stream.s;
    const uint32_t hl = (uint32_t)h->header.size();
    const size_t mb = (size_t)h->max_batch;
    if (!h->header_up) {
        HIP_OK(hipMemcpyAsync(h->d_header, h->header.data(), hl, hipMemcpyHostToDevice, st));
        h->header_up = true;
    }
    if (!devp && !h->d_sout) {   // one group's samples, each at its worst case, and its offsets
        if (h->mem.alloc(&h->d_sout, mb * ((size_t)h->bound + hl)) != hipSuccess ||
            h->mem.alloc(&h->d_offs, (mb + 1) * sizeof(uint64_t)) != hipSuccess) {
            h->mem.release(h->d_sout);
            h->d_sout = nullptr;
            return fail(DVC_E_NOMEM, "no device memory to stage %zu samples", mb);
        }
    }
    if (n == 0) {
        if (devp) HIP_OK(hipMemsetAsync(offsets, 0, sizeof(uint64_t), st));
        else offsets[0] = 0;
        return DVC_OK;
    }
    bool overflow = false;
    std::vector<uint64_t> ho(mb + 1);
    for (int f0 = 0; f0 < n; f0 += h->max_batch) {
        const int m = std::min(h->max_batch, n - f0);
        if (const int rc = pack_group(h, frames + (size_t)f0 * frame_stride, pitch, frame_stride, m)) return rc;
        if (devp) {   // the carry stays on the device: nothing waits between groups
            HIP_OK(dvc::jpeg_launch_stream(m, f0 == 0, g, h->b, h->d_header, hl, h->d_carry, offsets + f0, nullptr, out,
                                           cap, st));
            continue;
        }
        HIP_OK(dvc::jpeg_launch_stream(m, f0 == 0, g, h->b, h->d_header, hl, h->d_carry, h->d_offs, h->d_offs,
                                       h->d_sout, cap, st));
        HIP_OK(hipMemcpyAsync(ho.data(), h->d_offs, (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        std::memcpy(offsets + f0, ho.data(), (m + 1) * sizeof(uint64_t));
        int fit = m;   // the samples that end inside cap come first
        while (fit > 0 && !dvc::stream_fits(ho[fit], cap)) --fit;
        if (fit < m) {
            overflow = true;
            HIP_OK(hipMemsetAsync(h->b.overflow, 0, sizeof(uint32_t), st));
        }
        if (ho[fit] > ho[0]) {
            HIP_OK(hipMemcpyAsync(out + ho[0], h->d_sout, ho[fit] - ho[0], hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
        }
    }
    if (overflow) return fail(DVC_E_NOMEM, "the samples exceed cap %zu (offsets hold the needed places)", cap);
    return DVC_OK;
}

int dvc_jpeg_sync(dvc_jpeg* h)
{
    if (!h) return fail(DVC_E_INVALID, "NULL handle");
    if (h->device < 0) return DVC_OK;
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(h->stream.s));
    if (h->flags & DVC_FLAG_DEVICE_PTRS) {   // an overflow of an asynchronous call is reported here
        uint32_t hov = 0;
        HIP_OK(hipMemcpy(&hov, h->b.overflow, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (hov) {
            HIP_OK(hipMemset(h->b.overflow, 0, sizeof(uint32_t)));
            return fail(DVC_E_NOMEM, "a frame's entropy data exceeded its output slot (sizes hold the needed lengths)");
        }
    }
    return DVC_OK;
}

int dvc_jpeg_opt_tables(dvc_jpeg* h, const uint64_t* counts, uint8_t* dht, size_t cap, size_t* n)
{
    if (!h || !counts || !n) return fail(DVC_E_INVALID, "NULL argument");
    if (h->device < 0 || !h->b.opt)
        return fail(DVC_E_STATE, "the table builder needs a device handle created with DVC_FLAG_JPEG_OPT_HUFFMAN");
    uint64_t total = 0;
    for (int k = 0; k < dvc::kHuffTables; ++k)
        for (int s = 0; s < 256; ++s) {
            const uint64_t c = counts[256 * k + s];
            if (!c) continue;
            const int size = s & 15;
            const bool ok = k & 1 ? (s == 0x00 || s == 0xF0 || (size >= 1 && size <= 10)) : s <= 11;
            if (!ok) return fail(DVC_E_INVALID, "a count on symbol 0x%02x of table %d, which the coder cannot emit", s, k);
            if (k >= 2 && h->g.gray) return fail(DVC_E_INVALID, "a class 1 count on a one-component handle");
            if (c > (1ull << 62) - total) return fail(DVC_E_INVALID, "the counts sum to 2^62 or more");
            total += c;
        }
    if (!total) return fail(DVC_E_INVALID, "every count is 0");
    HIP_OK(hipSetDevice(h->device));
    hipStream_t st = h->stream.s;
    dvc::JpegOptTables* d = h->b.opt;
    uint32_t len = 0;
    std::vector<uint8_t> prefix(sizeof(d->prefix));
    HIP_OK(hipMemcpyAsync(h->b.counts, counts, dvc::kHuffTables * 256 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_OK(dvc::jpeg_launch_huff_build(h->g, h->b, st, false));   // into the tables' own prefix
    HIP_OK(hipMemcpyAsync(&len, &d->prefix_len, sizeof(len), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(prefix.data(), d->prefix, prefix.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const size_t sos = 8 + 2 * (size_t)h->chan;   // the SOS header behind the DHT segment
    if (len < sos + 4 || len > prefix.size()) return fail(DVC_E_HIP, "the table builder returned %u bytes", len);
    *n = len - sos;
    if (!dht) return DVC_OK;   // size query
    if (cap < *n) return fail(DVC_E_NOMEM, "the DHT segment needs %zu bytes, %zu given", *n, cap);
    std::memcpy(dht, prefix.data(), *n);
    return DVC_OK;
}

void dvc_jpeg_destroy(dvc_jpeg* h)
{
    if (!h) return;
    if (h->device >= 0) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream.s);
    }
    delete h;
}

}  // extern "C"
