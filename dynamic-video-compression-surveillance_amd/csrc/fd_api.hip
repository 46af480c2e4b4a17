// fd_api.hip — the C-ABI (include/dvc.h) of the frame-differencing worker.
//
// Host side of one camera feed: owns the device state the reference keeps in
// Python locals (prev_gray fd:75-77,133; accumulated_mask fd:81,107), the
// contour-filter scratch, and the launch sequence of fd_kernels.hip for one
// frame (the body of the loop at frame_differencing.py:85-138). What it shares
// with the other handles — the error text, the filter and DCT tables, the
// arena of what a handle owns, the stream fork / sync, the frame contract — is
// host_common.h and host_frames.h; also here: the calls that belong to no
// handle (version, last error, device count, pinned memory, contour filter).
#include <hip/hip_runtime.h>
#include <cstdlib>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/dvc.h"
#include "fd_kernels.h"
#include "klaunch.h"
#include "host_common.h"
#include "fd_sched.h"
#include "yuv_kernels.h"
#include "tune.h"

using dvc_host::fail;
using dvc_host::dct_matrix;
using dvc_host::gauss_taps;
using dvc_sched::NSLOT;
using dvc_sched::GRAPH_OWN_CCL_FRAMES;

// One batch's launch sequence as a HIP graph (enqueue_batch's graph path, VERDICT
// r5 #4): the launches of the four stages as dvc::klaunch recorded them, one
// chain in stage order, with the event nodes of the batch's plan (fd_sched.h).
// A later batch of the same launch shape re-uses it with the arguments and the
// waited-for events that changed set in place.
struct FdGraph {
    std::vector<dvc::KNode> rec[4];          // front, contour filter, accumulate, output: arguments as set in ge
    std::vector<hipGraphNode_t> node[4];
    std::vector<std::pair<hipGraphNode_t, hipEvent_t>> wait[4];   // the plan's waits: node, the event it waits for now
    bool records[4] = {};                    // the stage records its event
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    uint64_t used = 0;                       // seq of its last launch (least recently used is replaced)
};
constexpr int NGRAPH = 4;                    // graphs kept per slot (launch shapes: frame count, outputs, format)

// Buffers of one batch in flight (max_batch frames): motion masks, contour-
// filter scratch, kept masks, the dilate -> accumulate -> out bits, and the
// staged input frames when the caller's cannot be read in place.
struct Slot {
    dvc::CclBufs c{};
    uint64_t *dblk = nullptr, *rblk = nullptr, *sbits = nullptr;    // fast back end (B = 4, 8)
    uint8_t* docc = nullptr;   // fast back end: block rows with dilated bits (BackArgs::docc)
    uint64_t *dbits = nullptr, *rbits = nullptr, *zbits = nullptr;  // generic back end (row-major planes)
    uint8_t* fin = nullptr;    // resized / re-pitched / converted input frames (pitch ip), allocated when needed
    uint8_t* fsrc = nullptr;   // YUV frames converted to BGR at the source size, before the resize (pitch sip)
    hipEvent_t ev[dvc_sched::NSTG] = {};   // recorded after each stage of its batch (fd_sched.h: which, and who waits)
    std::vector<FdGraph> graphs;   // the graph path's graphs of this slot's batches
    // the graph path's contour filter: the slot's own working set (S.c's
    // mbits / kbits / kocc with its own run index, parents and areas), so
    // consecutive batches' filters overlap instead of queueing on
    // one shared set; grown at the slot's graph batches (graph_ccl)
    dvc::CclBufs gc{};
    dvc_host::DevMem gc_mem;
    int gc_frames = 0;      // frames gc holds
};

// Host-pointer path: two staging sets, so chunk c+1's frames go up while chunk
// c computes and chunk c-1's outputs come down.
struct Stage {
    uint8_t *d_in = nullptr, *d_ov = nullptr, *d_cp = nullptr;   // device
    uint8_t *h_in = nullptr, *h_ov = nullptr, *h_cp = nullptr;   // pinned host
    hipEvent_t ev_h2d = nullptr;   // h_in may be refilled
    hipEvent_t ev_d2h = nullptr;   // h_ov / h_cp hold the chunk's outputs
    hipEvent_t ev_free = nullptr;  // d_in / d_ov / d_cp may be reused
    bool busy = false;             // ev_free / ev_d2h hold a chunk
    int m = 0;                     // its frames
    uint8_t *ov = nullptr, *cp = nullptr;   // its destination (pageable outputs)
    size_t ostride = 0;
};
constexpr int NSTAGE = 2;

struct dvc_fd {
    dvc_fd_params p{};
    int device = 0;
    hipStream_t stream = nullptr;  // prime + contour filter (internal)
    hipStream_t user = nullptr;    // the caller's stream (create's hip_stream; NULL = legacy default)
    bool has_user = false;         // join `user` (hip_stream given, or DVC_FLAG_JOIN_STREAM)
    hipEvent_t ev_user = nullptr, ev_join_out = nullptr, ev_join_acc = nullptr;
    hipStream_t s_front = nullptr;       // input staging + blur/threshold front (previous-gray recurrence)
    hipStream_t s_acc = nullptr;         // dilate + accumulate (accumulated-mask recurrence)
    hipStream_t s_out = nullptr;         // overlay + compressed frames
    dvc::RowGeom g{};
    int gs = 0;          // gray row stride: roundup(W, 4)
    int ip = 0;          // pitch of staged frames: 3 * gs
    int sw = 0, sh = 0;  // source frame size (resized to W x H when different)
    int sip = 0;         // pitch of staged source frames (host path): 3 * roundup(sw, 4)
    bool resize = false;
    int fmt = DVC_FMT_BGR;  // frame format handed to prime/step (DVC_FMT_*)
    bool fused8 = false;    // DVC_FD_FUSED8=1 at create: the fused front for block_size 8 (opt-in)
    bool acc_short = false;  // k_acc's short form: acc_fast_ok holds and DVC_ACC_GENERAL was not set at create
    int crows = 0;          // YUV: luma rows before the chroma planes (device-pointer frames)
    dvc::ResizeTab rt{};
    int B = 4, NBX = 0, NBY = 0, AP = 0;   // block size, blocks (ceil), acc pitch
    size_t ofb = 0;                        // bytes of one output frame: 3WH (BGR) or 3WH/2 (I420)
    bool fast = true;                      // B = 4, 8: block-field back end
    dvc::GaussTaps kprime{};
    dvc::DctMat M{};
    float* Mtab = nullptr;                 // generic DCT bases (device)
    bool primed = false;
    bool failed = false;                   // stopped at an odd-size DCT (DVC_E_ODD_DCT)
    uint64_t err_frame = 0;
    int max_batch = 1;
    int SW = 0;          // 64-block words per block row
    size_t sstride = 0;  // static-block bit words per frame
    uint64_t frames = 0;           // frames stepped
    dvc_sched::State sched;        // what the ordering plan of the next batch depends on (fd_sched.h)
    int last_n = 0;                // frames of the last batch
    Slot slot[NSLOT];
    Stage stage[NSTAGE];
    int next_stage = 0;
    // device state
    uint8_t* gray[2] = {nullptr, nullptr};  // previous blurred gray (fd:77, 133): gray[gcur], rows of gs
    int gcur = 0;
    uint8_t* acc = nullptr;        // accumulated mask (fd:81, 107), AP x NBY*B
    uint64_t* dbg_dil = nullptr;
    uint32_t* tmp32 = nullptr;
    uint8_t* gtmp = nullptr;
    unsigned long long* stats = nullptr;
    unsigned long long* err = nullptr;  // first feed frame index with an odd static block side (~0: none)
    uint8_t* h_acc = nullptr;
    // every device and pinned allocation and ordering event of the handle, its slots' (but gc_mem) and stages'
    dvc_host::DevMem mem;
    // dominant-kernel timing
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    bool last_fused = false;   // the last batch ran the fused front (KTIMING timed k_front, not k_out)
    bool graph_ok = true;      // short device-frame batches take the graph path (DVC_FD_GRAPH=0 at create: never)
    uint64_t graph_batches = 0, graph_builds = 0;   // batches launched as graphs, graphs built (dvc_fd_graph_stats)

    ~dvc_fd()
    {
        for (Slot& s : slot)
            for (FdGraph& G : s.graphs) {
                if (G.ge) (void)hipGraphExecDestroy(G.ge);
                if (G.g) (void)hipGraphDestroy(G.g);
            }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        for (hipStream_t st : {s_front, s_acc, s_out, stream})
            if (st) (void)hipStreamDestroy(st);
    }
    dvc_host::FrameFmt frame() const { return {fmt, sw, sh, crows}; }
    hipError_t sync() const { return dvc_host::sync_streams({stream, s_front, s_acc, s_out}); }
    // The caller's stream (if any) -> every internal stream: work the caller
    // queued before this call (e.g. the copy that produced the frames, or reads
    // of the previous outputs) happens before the call's kernels.
    hipError_t wait_user() const
    {
        return has_user ? dvc_host::fork_streams(user, ev_user, {stream, s_front, s_acc, s_out}) : hipSuccess;
    }
    // The stream a stage runs on (stage streams), and the one a slot's graphs are launched on
    hipStream_t stage_stream(int stage) const
    {
        return stage == dvc_sched::FRONT ? s_front : stage == dvc_sched::FILTER ? stream
             : stage == dvc_sched::ACCUM ? s_acc : s_out;
    }
    hipStream_t graph_stream(int slot) const { return stage_stream(dvc_sched::slot_stream(slot)); }
    // `s` waits for the plan's events
    hipError_t wait(hipStream_t s, const dvc_sched::Waits& w) const
    {
        hipError_t e = hipSuccess;
        for (int i = 0; i < w.n && e == hipSuccess; ++i) e = hipStreamWaitEvent(s, slot[w.e[i].slot].ev[w.e[i].stage], 0);
        return e;
    }
};

// Internal streams -> the caller's stream: work the caller queues after this
// call sees its outputs (overlay/compressed on s_out, acc_out on s_acc).
static hipError_t join_user(dvc_fd* h)
{
    if (!h->has_user) return hipSuccess;
    hipError_t e = hipEventRecord(h->ev_join_out, h->s_out);
    if (e == hipSuccess) e = hipEventRecord(h->ev_join_acc, h->s_acc);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->user, h->ev_join_out, 0);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->user, h->ev_join_acc, 0);
    return e;
}

// After a sync: did a frame stop at an odd-size DCT (fd:122, fd:140)?
static int check_stop(dvc_fd* h)
{
    if (h->failed) return DVC_E_ODD_DCT;
    unsigned long long e = ~0ull;
    HIP_OK(hipMemcpy(&e, h->err, sizeof(e), hipMemcpyDeviceToHost));
    if (e == ~0ull) return DVC_OK;
    h->failed = true;
    h->err_frame = e;
    return fail(DVC_E_ODD_DCT, "frame %llu: a static block with an odd side > 1 (OpenCV: Odd-size DCT's are not "
                               "implemented, fd:122)", e + 1);
}

// How the kernels can read these device frames in place (host_frames.h
// readable_in_place; never across a resize): 1 as BGR rows reaching 3 * gs
// bytes, 2 as 4:2:0 surfaces (no staged BGR copy, fd_kernels.h SrcFmt;
// DVC_FD_YUV_DIRECT=0 forces the staged conversion, A/B), 0 not at all.
static int in_place(const dvc_fd* h, const uint8_t* p, size_t pitch, size_t fstride, int n)
{
    static const int yuv_on = [] { const char* e = dvc::tune_env("DVC_FD_YUV_DIRECT"); return e ? atoi(e) : 1; }();
    const bool bgr = h->fmt == DVC_FMT_BGR;
    if (h->resize || !(bgr || yuv_on)) return 0;
    return dvc_host::readable_in_place(h->p.width, p, pitch, bgr ? (size_t)h->ip : 0, fstride, n) ? (bgr ? 1 : 2) : 0;
}

static bool host_pinned(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

static hipError_t alloc_fin(dvc_fd* h)
{
    hipError_t e = hipSuccess;
    for (Slot& s : h->slot) {
        if (!s.fin && e == hipSuccess) e = h->mem.alloc(&s.fin, (size_t)h->ip * h->g.H * h->max_batch);
        if (!s.fsrc && h->fmt != DVC_FMT_BGR && h->resize && e == hipSuccess)
            e = h->mem.alloc(&s.fsrc, (size_t)h->sip * h->sh * h->max_batch);
    }
    return e;
}

extern "C" {

int dvc_abi_version(void) { return DVC_ABI_VERSION; }

const char* dvc_last_error(void) { return dvc_host::last_error(); }

int dvc_device_count(int* count)
{
    if (!count) return fail(DVC_E_INVALID, "count is NULL");
    HIP_OK(hipGetDeviceCount(count));
    return DVC_OK;
}

int dvc_gaussian_taps_q8(int n, double sigma, uint16_t* taps)
{
    if (!taps || gauss_taps(n, sigma, taps) != 0) return fail(DVC_E_INVALID, "kernel size must be odd, 1..63");
    return DVC_OK;
}

int dvc_host_alloc(size_t bytes, void** out)
{
    if (!out) return fail(DVC_E_INVALID, "NULL argument");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(DVC_E_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return DVC_OK;
}

void dvc_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

int dvc_fd_create(const dvc_fd_params* prm, int device, void* hip_stream, dvc_fd** out)
{
    if (!prm || !out) return fail(DVC_E_INVALID, "NULL argument");
    const dvc_fd_params& p = *prm;
    if (p.width < 16 || p.height < 16 || p.width > 65520)
        return fail(DVC_E_INVALID, "frame %dx%d outside 16..65520 x >=16", p.width, p.height);
    if (p.src_width < 0 || p.src_height < 0 || p.src_width > 65520)
        return fail(DVC_E_INVALID, "source frame %dx%d invalid", p.src_width, p.src_height);
    // block_size: k_out_gen stages a block's two B x B float planes in LDS (B = 128: 128 KB);
    // kernel_size: the dilation shifts a row by at most 63 bits either way (anchor k/2)
    if (p.block < 1 || p.block > 128)
        return fail(DVC_E_UNSUPPORTED, "block_size %d: the GPU path implements 1..128", p.block);
    if (p.ksize < 1 || p.anchor < 0 || p.anchor >= p.ksize)
        return fail(DVC_E_INVALID, "dilation kernel %d (anchor %d) invalid", p.ksize, p.anchor);
    if (p.anchor > 63 || p.ksize - 1 - p.anchor > 63)
        return fail(DVC_E_UNSUPPORTED, "dilation kernel %d (anchor %d): the GPU path implements 1..127", p.ksize,
                    p.anchor);
    if (p.ithresh < -1 || p.ithresh > 255) return fail(DVC_E_INVALID, "ithresh %d outside -1..255", p.ithresh);
    if (!(p.quant == p.quant) || p.quant == 0.0f) return fail(DVC_E_INVALID, "quantization_level must be nonzero");
    if (p.in_format != DVC_FMT_BGR && p.in_format != DVC_FMT_I420 && p.in_format != DVC_FMT_NV12)
        return fail(DVC_E_INVALID, "in_format %d unknown", p.in_format);
    if (p.in_format != DVC_FMT_BGR) {
        const int sw = p.src_width ? p.src_width : p.width, sh = p.src_height ? p.src_height : p.height;
        if ((sw & 1) || (sh & 1)) return fail(DVC_E_INVALID, "4:2:0 frames %dx%d: sides must be even", sw, sh);
        if (p.chroma_rows && (p.chroma_rows < sh || (p.chroma_rows & 1)))
            return fail(DVC_E_INVALID, "chroma_rows %d: even and >= the frame height %d", p.chroma_rows, sh);
    }
    if ((p.flags & DVC_FLAG_OUT_I420) &&
        ((p.block != 4 && p.block != 8) || p.width % p.block || p.height % p.block))
        return fail(DVC_E_UNSUPPORTED, "I420 outputs need block_size 4 or 8 and a frame of whole blocks (%dx%d, b=%d)",
                    p.width, p.height, p.block);
    const int mb = p.max_batch == 0 ? 1 : (int)p.max_batch;
    if (p.max_batch > DVC_MAX_BATCH) return fail(DVC_E_INVALID, "max_batch %u outside 1..%d", p.max_batch, DVC_MAX_BATCH);
    dvc_fd* h = new dvc_fd();
    h->p = p;
    h->device = device;
    h->max_batch = mb;
    h->g.W = p.width;
    h->g.H = p.height;
    h->g.WW = (p.width + 63) / 64;
    h->g.CAP = p.width / 2 + 1;
    {   // the contour filter stages a band's run index in LDS: ~32k px per row at most
        int lds = 160 * 1024;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) lds = 160 * 1024;
        if (dvc::ccl_max_lds(h->g) > (size_t)lds) {
            delete h;
            return fail(DVC_E_UNSUPPORTED, "frame width %d: the contour filter's row index needs %zu B of LDS (max %d)",
                        p.width, dvc::ccl_max_lds(h->g), lds);
        }
        // k_out_gen stages one block's two B x B float planes (+ a flag word)
        const size_t gen_lds = (size_t)8 * p.block * p.block + 4;
        if (gen_lds > (size_t)lds) {
            delete h;
            return fail(DVC_E_UNSUPPORTED, "block_size %d: the output stage needs %zu B of LDS (max %d)", p.block,
                        gen_lds, lds);
        }
    }
    h->gs = (p.width + 3) & ~3;
    h->ip = 3 * h->gs;
    h->sw = p.src_width ? p.src_width : p.width;
    h->sh = p.src_height ? p.src_height : p.height;
    h->sip = 3 * ((h->sw + 3) & ~3);
    h->resize = h->sw != p.width || h->sh != p.height;
    h->fmt = p.in_format;
    {   // DVC_FD_FUSED8=1 (read per handle): the fused front for block_size 8 (see enqueue_batch)
        const char* e = getenv("DVC_FD_FUSED8");
        h->fused8 = e && atoi(e) != 0;
        // DVC_FD_GRAPH=0 (read per handle): every batch on the stage streams (tests compare both paths)
        const char* g = getenv("DVC_FD_GRAPH");
        h->graph_ok = !g || atoi(g) != 0;
        // DVC_ACC_GENERAL=1 (read per handle): k_acc's general form even where the short
        // form is exact (same bytes; the tests compare the two, dvc_fd_acc_form says which)
        const char* ag = getenv("DVC_ACC_GENERAL");
        h->acc_short = dvc::acc_fast_ok(p.alpha, p.beta, p.gamma) && !(ag && atoi(ag) != 0);
    }
    h->ofb = (p.flags & DVC_FLAG_OUT_I420) ? (size_t)p.width * p.height * 3 / 2 : (size_t)p.width * p.height * 3;
    h->crows = p.chroma_rows ? p.chroma_rows : h->sh;
    h->B = p.block;
    h->fast = dvc::fast_block(p.block);
    h->NBX = (p.width + p.block - 1) / p.block;
    h->NBY = (p.height + p.block - 1) / p.block;
    h->AP = (h->NBX * p.block + 3) & ~3;
    h->SW = (h->NBX + 63) / 64;
    h->sstride = (size_t)h->NBY * h->SW;
    if (gauss_taps(p.prime_ksize, p.prime_sigma, h->kprime.t) != 0) {
        delete h;
        return fail(DVC_E_INVALID, "prime blur size %d must be odd, 1..63", p.prime_ksize);
    }
    h->kprime.n = p.prime_ksize;
    if (h->fast) dct_matrix(p.block, h->M);
    auto bad = [&](hipError_t e, const char* what) {
        delete h;
        return dvc_host::create_failed(e, what);
    };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return bad(e, "hipSetDevice");
    h->user = (hipStream_t)hip_stream;
    h->has_user = hip_stream != nullptr || (p.flags & DVC_FLAG_JOIN_STREAM);
    // four internal streams — contour filter, front, accumulate, output —
    // within the default 4 hardware queues (a queue shared by two stages
    // serialises them); priorities: the HBM-bound output stage (the stream that
    // is busy the whole period) high, the front low, the latency-bound contour
    // filter and accumulate chains in between ("lnnh" vs round 1's "lhhn":
    // +0.1..1 % in interleaved A/Bs with the nontemporal outputs, k_out's
    // in-pipeline frac 0.38 -> 0.39). The caller's stream (if
    // any) is only joined: each call waits for the work queued on it before the
    // call, and work queued on it after the call waits for the call's outputs.
    int plo = 0, phi = 0;
    (void)hipDeviceGetStreamPriorityRange(&plo, &phi);
    // priorities of the front, contour-filter, accumulate and output streams:
    // 'l'ow, 'n'ormal, 'h'igh; DVC_PRIO overrides for sweeps (default "lnnh")
    static const char* prio = [] { const char* e = dvc::tune_env("DVC_PRIO"); return e && strlen(e) == 4 ? e : "lnnh"; }();
    auto level = [&](char c) { return c == 'l' ? plo : c == 'h' ? phi : 0; };
    auto mk = [](hipStream_t* st, int pr) { return hipStreamCreateWithPriority(st, hipStreamNonBlocking, pr); };
    if ((e = mk(&h->stream, level(prio[1]))) != hipSuccess) return bad(e, "hipStreamCreate");
    for (hipEvent_t* ev : {&h->ev_user, &h->ev_join_out, &h->ev_join_acc})
        if ((e = h->mem.event(ev)) != hipSuccess) return bad(e, "hipEventCreate");
    for (auto sp : {std::make_pair(&h->s_front, level(prio[0])), std::make_pair(&h->s_acc, level(prio[2])),
                    std::make_pair(&h->s_out, level(prio[3]))})
        if ((e = mk(sp.first, sp.second)) != hipSuccess) return bad(e, "hipStreamCreate");
#ifdef DVC_EXPERIMENTS
    // DVC_CU_SPLIT=k (experiment build only): the contour filter, accumulate
    // and output / fix-up streams on k CUs spread evenly over the device, the
    // front on the others. The masked streams are built before the default
    // ones are released; they are blocking streams without priorities (the
    // CU-mask API takes neither).
    if (const char* cs = getenv("DVC_CU_SPLIT"); cs && *cs) {
        int ncu = 256;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        const int k = std::max(1, std::min(atoi(cs), ncu - 1));
        std::vector<uint32_t> ma((ncu + 31) / 32, 0u), mb((ncu + 31) / 32, 0u);
        for (int i = 0; i < ncu; ++i) {
            const bool a = (long long)i * k / ncu != (long long)(i + 1) * k / ncu;
            (a ? ma : mb)[i / 32] |= 1u << (i % 32);
        }
        const uint32_t nw = (uint32_t)ma.size() * 32;
        hipStream_t ns[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < 4; ++i)
            if ((e = hipExtStreamCreateWithCUMask(&ns[i], nw, i < 3 ? ma.data() : mb.data())) != hipSuccess) {
                for (int k2 = 0; k2 < i; ++k2) (void)hipStreamDestroy(ns[k2]);
                return bad(e, "hipExtStreamCreateWithCUMask");
            }
        hipStream_t* olds[4] = {&h->stream, &h->s_acc, &h->s_out, &h->s_front};
        for (int i = 0; i < 4; ++i) {
            (void)hipStreamDestroy(*olds[i]);
            *olds[i] = ns[i];
        }
    }
#endif
    const size_t W = p.width, H = p.height, N = W * H, WW = h->g.WW;
    const size_t nfield = (size_t)h->NBX * h->NBY;   // block fields per frame
    for (int k = 0; k < NSLOT; ++k) {
        Slot& s = h->slot[k];
        size_t sz[dvc::CclBufs::NARR];
        dvc::CclBufs::sizes(h->g, mb, sz);
        void **ptrs[dvc::CclBufs::NARR], **ptrs0[dvc::CclBufs::NARR];
        s.c.ptrs(ptrs);
        h->slot[0].c.ptrs(ptrs0);
        // Only the motion bits (written by the front of a later batch while this
        // one's contour filter runs) and the kept bits (read by the accumulate
        // stage after it) belong to a slot; the filter's run index, parents
        // and areas (~17 MB per 1080p frame) are touched only
        // inside the contour-filter stage, whose batches run one after another
        // on the handle's stream: one set serves all slots.
        for (int i = 0; i < dvc::CclBufs::NARR; ++i) {
            if (dvc::CclBufs::working_set(i) && k > 0) *ptrs[i] = *ptrs0[i];   // slot 0's
            else if ((e = h->mem.alloc(ptrs[i], sz[i])) != hipSuccess) return bad(e, "hipMalloc");
        }
        // rows of the kept mask with bits (k_paint -> dilate); KEEP_PLANES reads
        // the kept mask back, so every row is written then
        if ((e = h->mem.alloc(&s.c.kocc, H * (size_t)mb)) != hipSuccess) return bad(e, "hipMalloc");
        s.c.kfull = (p.flags & DVC_FLAG_KEEP_PLANES) ? 1 : 0;
        if (h->fast) {   // block fields: u16 (B = 4) / u64 (B = 8) per block
            const size_t fb = p.block == 4 ? 2 : 8;
            if ((e = h->mem.alloc(&s.docc, (size_t)h->NBY * mb)) != hipSuccess) return bad(e, "hipMalloc");
            if ((e = h->mem.alloc(&s.dblk, fb * nfield * mb)) != hipSuccess) return bad(e, "hipMalloc");
            if ((e = h->mem.alloc(&s.rblk, fb * nfield * mb)) != hipSuccess) return bad(e, "hipMalloc");
            if ((e = h->mem.alloc(&s.sbits, 8 * h->sstride * (size_t)mb)) != hipSuccess) return bad(e, "hipMalloc");
        } else {
            for (uint64_t** q : {&s.dbits, &s.rbits, &s.zbits})
                if ((e = h->mem.alloc(q, 8 * H * WW * (size_t)mb)) != hipSuccess) return bad(e, "hipMalloc");
        }
        for (hipEvent_t& ev : s.ev)
            if ((e = h->mem.event(&ev)) != hipSuccess) return bad(e, "hipEventCreate");
    }
    // staged input frames: always needed to resize or when rows are not whole quads
    if (h->resize || p.width % 4 || h->fmt != DVC_FMT_BGR) {
        if ((e = alloc_fin(h)) != hipSuccess) return bad(e, "hipMalloc");
    }
    const size_t accb = (size_t)h->AP * h->NBY * p.block;
    struct { void** ptr; size_t bytes; } allocs[] = {
        {(void**)&h->gray[0], (size_t)h->gs * H}, {(void**)&h->gray[1], (size_t)h->gs * H}, {(void**)&h->acc, accb},
        {(void**)&h->stats, 8 * 4 * 64}, {(void**)&h->err, 8},
    };
    for (auto& a : allocs)
        if ((e = h->mem.alloc(a.ptr, a.bytes)) != hipSuccess) return bad(e, "hipMalloc");
    for (Slot& s : h->slot) s.c.stats = h->stats;
    {   // DCT bases of length B, W % B, H % B (the generic back end / partial edge blocks)
        const int B = p.block, bw = p.width % B, bh = p.height % B;
        std::vector<float> tab((size_t)B * B + bw * bw + bh * bh);
        // (the computed form also for B = 4, 8: not the tables of dct_const.h)
        const auto basis = dvc_host::dct_basis;
        basis(B, tab.data());
        if (bw) basis(bw, tab.data() + B * B);
        if (bh) basis(bh, tab.data() + B * B + bw * bw);
        if ((e = h->mem.alloc(&h->Mtab, 4 * tab.size())) != hipSuccess) return bad(e, "hipMalloc");
        if ((e = hipMemcpy(h->Mtab, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice)) != hipSuccess)
            return bad(e, "hipMemcpy");
    }
    if (h->resize) {
        std::vector<int> tx(3 * W), ty(3 * H);
        dvc::resize_tables(h->sw, h->sh, p.width, p.height, tx.data(), ty.data(), &h->rt.area2x, &h->rt.simd_end);
        h->rt.sw = h->sw;
        h->rt.sh = h->sh;
        h->rt.dw = p.width;
        h->rt.dh = p.height;
        int *dx = nullptr, *dy = nullptr;
        if ((e = h->mem.alloc(&dx, 4 * tx.size())) != hipSuccess) return bad(e, "hipMalloc");
        h->rt.xo = dx;
        if ((e = h->mem.alloc(&dy, 4 * ty.size())) != hipSuccess) return bad(e, "hipMalloc");
        h->rt.yo = dy;
        if ((e = hipMemcpy(dx, tx.data(), 4 * tx.size(), hipMemcpyHostToDevice)) != hipSuccess) return bad(e, "hipMemcpy");
        if ((e = hipMemcpy(dy, ty.data(), 4 * ty.size(), hipMemcpyHostToDevice)) != hipSuccess) return bad(e, "hipMemcpy");
    }
    if (p.flags & DVC_FLAG_KEEP_PLANES) {
        if ((e = h->mem.alloc(&h->dbg_dil, 8 * H * WW)) != hipSuccess) return bad(e, "hipMalloc");
    }
    if (!(p.flags & DVC_FLAG_DEVICE_PTRS)) {
        const size_t Fi = (size_t)h->sip * h->sh * mb, Fo = 3 * N * (size_t)mb;
        for (Stage& st : h->stage) {
            if ((e = h->mem.alloc(&st.d_in, Fi)) != hipSuccess) return bad(e, "hipMalloc");
            if ((e = h->mem.alloc(&st.d_ov, Fo)) != hipSuccess) return bad(e, "hipMalloc");
            if ((e = h->mem.alloc(&st.d_cp, Fo)) != hipSuccess) return bad(e, "hipMalloc");
            if ((e = h->mem.alloc_pinned(&st.h_in, Fi)) != hipSuccess) return bad(e, "hipHostMalloc");
            if ((e = h->mem.alloc_pinned(&st.h_ov, Fo)) != hipSuccess) return bad(e, "hipHostMalloc");
            if ((e = h->mem.alloc_pinned(&st.h_cp, Fo)) != hipSuccess) return bad(e, "hipHostMalloc");
            for (hipEvent_t* ev : {&st.ev_h2d, &st.ev_d2h, &st.ev_free})
                if ((e = h->mem.event(ev)) != hipSuccess) return bad(e, "hipEventCreate");
        }
        if ((e = h->mem.alloc_pinned(&h->h_acc, N)) != hipSuccess) return bad(e, "hipHostMalloc");
    }
    if ((e = hipMemsetAsync(h->stats, 0, 8 * 4 * 64, h->stream)) != hipSuccess) return bad(e, "hipMemset");
    if ((e = hipMemsetAsync(h->err, 0xff, 8, h->stream)) != hipSuccess) return bad(e, "hipMemset");
    // the acc padding of partial blocks stays 0 for good
    if ((e = hipMemsetAsync(h->acc, 0, accb, h->stream)) != hipSuccess) return bad(e, "hipMemset");
    // the OUTSIDE gap node of every frame slice is its own root before any
    // k_band runs (its over-budget path may walk through it)
    {
        size_t sz[dvc::CclBufs::NARR];
        dvc::CclBufs::sizes(h->g, mb, sz);
        if ((e = hipMemsetAsync(h->slot[0].c.gpar, 0, sz[dvc::CclBufs::I_GPAR], h->stream)) != hipSuccess) return bad(e, "hipMemset");
    }
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return bad(e, "hipStreamSynchronize");
    *out = h;
    return DVC_OK;
}

}  // extern "C"

// Frames the kernels read: the caller's in place, or staged into slot S's
// buffer on s_front (re-pitched, or resized — cv2.resize, fd:74,91), behind
// the batch's plan's waits (the slot's previous batch is out).
// `sf` (nullable: the prime's single frame is always staged as BGR) receives
// how the kernels read the frames: BGR, or the 4:2:0 surfaces in place.
static int stage_input(dvc_fd* h, Slot& S, const uint8_t* src, size_t pitch, size_t fstride, int n,
                       const uint8_t** d, int* dp, size_t* dfs, int crows, dvc::SrcFmt* sf)
{
    if (sf) *sf = dvc::SrcFmt{DVC_FMT_BGR, 0, 0, 0};
    const int direct = in_place(h, src, pitch, fstride, n);
    if (direct == 1) {
        *d = src;
        *dp = (int)pitch;
        *dfs = fstride;
        return DVC_OK;
    }
    if (sf && direct == 2) {
        const dvc::YuvLayout L = dvc::yuv_layout(src, pitch, h->fmt, crows, fstride);
        *sf = dvc::SrcFmt{h->fmt, L.uoff, L.voff, L.cpitch};
        *d = src;
        *dp = (int)pitch;
        *dfs = fstride;
        return DVC_OK;
    }
    if (!S.fin) HIP_OK(alloc_fin(h));
    const size_t H = h->g.H, fs = (size_t)h->ip * H;
    if (h->fmt != DVC_FMT_BGR) {
        // the decoder's 4:2:0 surfaces -> BGR (cvtColor, what VideoCapture.read()
        // returns, fd:87), at the source size when a resize follows
        const dvc::YuvLayout L = dvc::yuv_layout(src, pitch, h->fmt, crows, fstride);
        const size_t sfs = (size_t)h->sip * h->sh;
        HIP_OK(dvc::launch_yuv420_to_bgr(L, h->sw, h->sh, n, h->resize ? S.fsrc : S.fin, h->resize ? h->sip : h->ip,
                                         h->resize ? sfs : fs, h->s_front));
        if (h->resize) HIP_OK(dvc::launch_resize(S.fsrc, h->sip, sfs, S.fin, h->ip, fs, n, h->rt, h->s_front));
    } else if (h->resize) {
        HIP_OK(dvc::launch_resize(src, (int)pitch, fstride, S.fin, h->ip, fs, n, h->rt, h->s_front));
    } else if (n == 1 || fstride == pitch * H) {
        HIP_OK(hipMemcpy2DAsync(S.fin, h->ip, src, pitch, 3 * (size_t)h->g.W, H * n, hipMemcpyDeviceToDevice,
                                h->s_front));
    } else {
        for (int t = 0; t < n; ++t)
            HIP_OK(hipMemcpy2DAsync(S.fin + t * fs, h->ip, src + t * fstride, pitch, 3 * (size_t)h->g.W, H,
                                    hipMemcpyDeviceToDevice, h->s_front));
    }
    *d = S.fin;
    *dp = h->ip;
    *dfs = fs;
    return DVC_OK;
}

// The tail of dvc_fd_prime / dvc_fd_set_state, on s_front behind the new state:
// a new run starts, its counters and the odd-DCT stop reset.
static int start_run(dvc_fd* h)
{
    HIP_OK(hipMemsetAsync(h->stats, 0, 8 * 4 * 64, h->s_front));
    HIP_OK(hipMemsetAsync(h->err, 0xff, 8, h->s_front));
    HIP_OK(hipStreamSynchronize(h->s_front));
    h->frames = h->err_frame = 0;
    h->sched = dvc_sched::State{};   // (its caller has synced every stream)
    h->last_n = 0;
    h->primed = true;
    h->failed = false;
    return DVC_OK;
}

extern "C" {

int dvc_fd_prime(dvc_fd* h, const uint8_t* bgr, size_t pitch)
{
    if (!h || !bgr) return fail(DVC_E_INVALID, "NULL argument");
    if (!dvc_host::pitch_ok(h->frame(), pitch)) return fail(DVC_E_INVALID, "pitch %zu invalid", pitch);
    HIP_OK(hipSetDevice(h->device));
    const size_t W = h->p.width, H = h->p.height;
    if (!h->tmp32) {
        HIP_OK(h->mem.alloc(&h->tmp32, 4 * W * H));
        HIP_OK(h->mem.alloc(&h->gtmp, (size_t)h->gs * H));
    }
    HIP_OK(h->sync());  // no batch of a previous run may still be in flight
    HIP_OK(h->wait_user());
    for (dvc_sched::SlotState& s : h->sched.slot) s.recorded = false;
    for (Stage& s : h->stage) s.busy = false;
    const uint8_t* src = bgr;
    size_t sp = pitch;
    int crows = h->crows;
    if (!(h->p.flags & DVC_FLAG_DEVICE_PTRS)) {
        Stage& st = h->stage[0];
        dvc_host::pack_host_frame(h->frame(), bgr, pitch, st.h_in, h->sip);
        HIP_OK(hipMemcpyAsync(st.d_in, st.h_in, (size_t)h->sip * h->sh, hipMemcpyHostToDevice, h->s_front));
        src = st.d_in;
        sp = h->fmt == DVC_FMT_BGR ? h->sip : h->sw;
        crows = h->sh;
    }
    const uint8_t* d = nullptr;
    int dp = 0;
    size_t dfs = 0;
    int rc = stage_input(h, h->slot[0], src, sp, 0, 1, &d, &dp, &dfs, crows, nullptr);
    if (rc) return rc;
    HIP_OK(dvc::launch_prime(d, dp, h->gtmp, h->tmp32, h->gray[h->gcur], h->p.width, h->p.height, h->gs, h->kprime,
                             h->s_front));
    HIP_OK(hipMemsetAsync(h->acc, 0, (size_t)h->AP * h->NBY * h->B, h->s_front));
    return start_run(h);
}

// Resume a feed (checkpoint / resume): the state the reference
// carries from frame to frame — the previous blurred gray (fd:77,93,133) and
// the accumulated mask (fd:81,107), host H x W planes as dvc_fd_read_plane
// exports them (DVC_PLANE_GRAY, DVC_PLANE_ACC). Like dvc_fd_prime it starts a
// new run: counters and the odd-DCT stop are reset.
int dvc_fd_set_state(dvc_fd* h, const uint8_t* prev_gray, const uint8_t* acc)
{
    if (!h || !prev_gray || !acc) return fail(DVC_E_INVALID, "NULL argument");
    HIP_OK(hipSetDevice(h->device));
    const size_t W = h->p.width, H = h->p.height;
    HIP_OK(h->sync());  // no batch of a previous run may still be in flight
    HIP_OK(h->wait_user());
    for (dvc_sched::SlotState& s : h->sched.slot) s.recorded = false;
    for (Stage& s : h->stage) s.busy = false;
    HIP_OK(hipMemcpy2DAsync(h->gray[h->gcur], h->gs, prev_gray, W, W, H, hipMemcpyHostToDevice, h->s_front));
    // the acc rows have pitch AP; the padding of partial blocks stays 0 (create)
    HIP_OK(hipMemcpy2DAsync(h->acc, h->AP, acc, W, W, H, hipMemcpyHostToDevice, h->s_front));
    return start_run(h);
}

}  // extern "C"

// The slot's own contour-filter working set for short graph batches (Slot::gc):
// ~17 MB a 1080p frame, grown to the batch (powers of two up to
// min(max_batch, GRAPH_OWN_CCL_FRAMES) frames), so per-frame calls hold four
// one-frame sets. A graph keeps the old pointers until its next launch sets
// the changed arguments.
static int graph_ccl(dvc_fd* h, int k, int n)
{
    Slot& S = h->slot[k];
    if (n <= S.gc_frames) return DVC_OK;
    int cap = 1;
    while (cap < n) cap *= 2;
    cap = std::min(cap, std::min(h->max_batch, GRAPH_OWN_CCL_FRAMES));
    if (!S.gc_mem.dev.empty()) {
        // the slot's last batch is done with the set
        if (h->sched.slot[k].recorded) HIP_OK(hipEventSynchronize(S.ev[dvc_sched::OUTPUT]));
        S.gc_mem.free_all();
        S.gc_frames = 0;
    }
    size_t sz[dvc::CclBufs::NARR];
    dvc::CclBufs::sizes(h->g, cap, sz);
    S.gc = S.c;
    void** ptrs[dvc::CclBufs::NARR];
    S.gc.ptrs(ptrs);
    for (int i = 0; i < dvc::CclBufs::NARR; ++i) {
        if (!dvc::CclBufs::working_set(i)) continue;
        const hipError_t e = S.gc_mem.alloc(ptrs[i], sz[i]);
        if (e != hipSuccess) {
            S.gc_mem.free_all();
            return dvc_host::create_failed(e, "graph contour-filter set");
        }
    }
    // every frame slice's OUTSIDE gap node is its own root before any k_band (as at create)
    HIP_OK(hipMemsetAsync(S.gc.gpar, 0, sz[dvc::CclBufs::I_GPAR], h->graph_stream(k)));
    S.gc_frames = cap;
    return DVC_OK;
}

static hipKernelNodeParams node_params(const dvc::KNode& kn, std::vector<void*>& pp)
{
    hipKernelNodeParams kp{};
    kp.func = const_cast<void*>(kn.f);
    kp.gridDim = kn.grid;
    kp.blockDim = kn.block;
    kp.sharedMemBytes = kn.shm;
    kn.params(pp);
    kp.kernelParams = pp.data();
    return kp;
}

// The graph path of one batch (device frames read in place, no KTIMING): the
// four stages' launches as recorded (dvc::klaunch) are matched against this
// slot's graphs by launch shape and launched as one graph on the slot's graph
// stream. A call then costs one graph launch and a few argument updates
// instead of nine launches and eleven event operations across four streams
// (~80 us of host time a call, profiles/r6_fd_per_call_*). The chain's wait
// and record nodes and the waits before the launch are the plan's (fd_sched.h).
static int enqueue_graph(dvc_fd* h, int k, std::vector<dvc::KNode> (&rec)[4], const dvc_sched::Plan& pl)
{
    Slot& S = h->slot[k];
    const bool recorded = h->sched.slot[k].recorded;
    const hipEvent_t ev_out = S.ev[dvc_sched::OUTPUT];
    auto event = [&](dvc_sched::Ev e) { return h->slot[e.slot].ev[e.stage]; };
    FdGraph* G = nullptr;
    for (FdGraph& x : S.graphs) {
        bool same = true;
        for (int sg = 0; sg < 4 && same; ++sg) {
            same = x.rec[sg].size() == rec[sg].size() && (int)x.wait[sg].size() == pl.stage[sg].n &&
                   x.records[sg] == pl.record[sg];
            for (size_t u = 0; same && u < rec[sg].size(); ++u) same = x.rec[sg][u].same_shape(rec[sg][u]);
        }
        if (same) {
            G = &x;
            break;
        }
    }
    std::vector<void*> pp;
    if (G) {
        // the exec's previous launch (batch i-4, this slot's) must have read its
        // arguments before they are overwritten: wait for it on the host (it is
        // four batches back, so the device keeps three batches queued meanwhile)
        if (recorded) HIP_OK(hipEventSynchronize(ev_out));
        for (int sg = 0; sg < 4; ++sg) {
            for (size_t u = 0; u < rec[sg].size(); ++u) {
                dvc::KNode& cur = G->rec[sg][u];
                if (cur.args == rec[sg][u].args) continue;
                cur.args.swap(rec[sg][u].args);
                const hipKernelNodeParams kp = node_params(cur, pp);
                HIP_OK(hipGraphExecKernelNodeSetParams(G->ge, G->node[sg][u], &kp));
            }
            for (int u = 0; u < pl.stage[sg].n; ++u) {   // the waits whose event differs from the one the node holds
                const hipEvent_t e = event(pl.stage[sg].e[u]);
                if (G->wait[sg][u].second == e) continue;
                HIP_OK(hipGraphExecEventWaitNodeSetEvent(G->ge, G->wait[sg][u].first, e));
                G->wait[sg][u].second = e;
            }
        }
    } else {
        if ((int)S.graphs.size() >= NGRAPH) {   // replace the least recently used one
            size_t lru = 0;
            for (size_t u = 1; u < S.graphs.size(); ++u)
                if (S.graphs[u].used < S.graphs[lru].used) lru = u;
            if (recorded) HIP_OK(hipEventSynchronize(ev_out));
            (void)hipGraphExecDestroy(S.graphs[lru].ge);
            (void)hipGraphDestroy(S.graphs[lru].g);
            S.graphs.erase(S.graphs.begin() + (long)lru);
        }
        FdGraph NG;
        // a failed build leaves nothing behind: the graph is kept only once instantiated
        struct Drop {
            FdGraph& x;
            bool keep = false;
            ~Drop()
            {
                if (keep) return;
                if (x.ge) (void)hipGraphExecDestroy(x.ge);
                if (x.g) (void)hipGraphDestroy(x.g);
            }
        } drop{NG};
        G = &NG;
        HIP_OK(hipGraphCreate(&G->g, 0));
        hipGraphNode_t last = nullptr;   // one chain: every node depends on the one before
        auto dep = [&]() { return last ? 1u : 0u; };
        for (int sg = 0; sg < 4; ++sg) {
            hipGraphNode_t nd = nullptr;
            // the accumulate stage's waits stand before its last kernel only (k_acc:
            // the accumulated mask); k_dilate, when the stage has it, reads this
            // batch's kept mask alone
            const size_t wat = sg == dvc_sched::ACCUM && !rec[sg].empty() ? rec[sg].size() - 1 : 0;
            for (size_t u = 0; u <= rec[sg].size(); ++u) {
                for (int w = 0; u == wat && w < pl.stage[sg].n; ++w) {
                    const hipEvent_t e = event(pl.stage[sg].e[w]);
                    HIP_OK(hipGraphAddEventWaitNode(&nd, G->g, last ? &last : nullptr, dep(), e));
                    G->wait[sg].emplace_back(nd, e);
                    last = nd;
                }
                if (u == rec[sg].size()) break;
                const hipKernelNodeParams kp = node_params(rec[sg][u], pp);
                HIP_OK(hipGraphAddKernelNode(&nd, G->g, last ? &last : nullptr, dep(), &kp));
                G->node[sg].push_back(nd);
                last = nd;
            }
            G->records[sg] = pl.record[sg];
            if (pl.record[sg]) {
                HIP_OK(hipGraphAddEventRecordNode(&nd, G->g, last ? &last : nullptr, dep(), S.ev[sg]));
                last = nd;
            }
            G->rec[sg].swap(rec[sg]);
        }
        HIP_OK(hipGraphInstantiate(&G->ge, G->g, nullptr, nullptr, 0));
        drop.keep = true;
        S.graphs.push_back(std::move(NG));
        G = &S.graphs.back();
        h->graph_builds++;
    }
    HIP_OK(h->wait(h->graph_stream(k), pl.pre));
    HIP_OK(hipGraphLaunch(G->ge, h->graph_stream(k)));
    G->used = h->sched.seq;
    h->graph_batches++;
    return DVC_OK;
}

// Enqueue one batch of n <= max_batch frames in slot seq % NSLOT: four stages
// (front, contour filter, dilate + accumulate, outputs) on the four stage
// streams or, for device frames read in place, as one graph (enqueue_graph) —
// the same kernels and arguments either way. Which path, and which events each
// stage waits for and records, is dvc_sched::plan (fd_sched.h, with the buffers
// each stage touches); this function executes the plan.
// With the kept mask on chip (fuse_paint_dilate) the filter stage ends in
// k_paint_dilate and the accumulate stage is k_acc alone; the events stay as
// they are (the filter's is recorded after k_paint_dilate, whose reads of the
// filter set are the batch's last, as they were k_paint's).
static int enqueue_batch(dvc_fd* h, const uint8_t* src, size_t pitch, size_t fstride, int n, uint8_t* ov, uint8_t* cp,
                         size_t ostride, int crows)
{
    const int k = (int)(h->sched.seq % NSLOT);
    Slot& S = h->slot[k];
#ifdef DVC_ABLATION
    // DVC_FD_SKIP (stage ablation for profiling only, results are wrong when
    // set): bit 0 front, 1 contour filter, 2 dilate + accumulate, 3 output.
    // Only in the ablation build (tools/build_variant.sh <out> -DDVC_ABLATION),
    // never in the shipping library.
    static const int skip = [] {
        const char* e = getenv("DVC_FD_SKIP");
        const int v = e ? atoi(e) : 0;
        if (v) std::fprintf(stderr, "dvc: DVC_FD_SKIP=%d set: stages skipped, outputs are wrong (profiling only)\n", v);
        return v;
    }();
#else
    constexpr int skip = 0;
#endif
    const bool timed = h->p.flags & DVC_FLAG_KTIMING;
    const int direct = in_place(h, src, pitch, fstride, n);   // 0: staged, 2: read as 4:2:0 surfaces
    const int opitch = 3 * h->p.width;
    const int obytes = (opitch % 4) || (ostride % 4) || ((uintptr_t)ov & 3) || ((uintptr_t)cp & 3);
    const bool out_i420 = h->p.flags & DVC_FLAG_OUT_I420;
    // fused front (fd_kernels.h FrontOut): block_size 4, BGR frames or 4:2:0
    // surfaces read in place (or staged), BGR outputs in dword rows or I420
    // frames (DVC_FLAG_OUT_I420: the front and k_fix4 write BGR2YUV_I420);
    // DVC_FD_FUSED=0 turns it off (A/B)
    static const int fuse_env = [] { const char* e = dvc::tune_env("DVC_FD_FUSED"); return e ? atoi(e) : 1; }();
    // (B = 4: k_fix4 scans a block row's static words in one wave, SW <= 64;
    // B = 8, opt-in with DVC_FD_FUSED8=1: BGR frames, fixed up by k_out<8>'s
    // per-block pass. Not the default: the 8x8 DCT at four lanes a block makes
    // the VALU-bound front the period — 268-270 k against 288 k Mpx/s for the
    // one-pass k_out<8> at the __main__ kwargs, experiments/README.md)
    const bool fused = fuse_env && !(h->p.flags & DVC_FLAG_FD_UNFUSED) && !obytes && (ov || cp) &&
                       ((h->B == 4 && h->SW <= 64) || (h->B == 8 && h->fused8 && direct != 2 && !out_i420));
    dvc_sched::Request rq;
    rq.n = n;
    {   // the byte ranges this batch's outputs cover (frames of ostride, the last one ofb bytes)
        const size_t span = n > 0 ? (size_t)(n - 1) * ostride + h->ofb : 0;
        rq.olo[0] = (uintptr_t)ov;
        rq.ohi[0] = ov ? (uintptr_t)ov + span : 0;
        rq.olo[1] = (uintptr_t)cp;
        rq.ohi[1] = cp ? (uintptr_t)cp + span : 0;
    }
    rq.staged = direct == 0;
    // (DVC_FD_GRAPH=0 at create turns the graph path off)
    rq.graph_ok = h->graph_ok && (h->p.flags & DVC_FLAG_DEVICE_PTRS) && !timed && !skip;
    rq.fused = fused;
    const dvc_sched::Plan pl = dvc_sched::plan(h->sched, rq);
    if (!pl.graph) HIP_OK(h->wait(h->s_front, pl.pre));
    const uint8_t* d = nullptr;
    int dp = 0;
    size_t dfs = 0;
    dvc::SrcFmt sf{};
    int rc = stage_input(h, S, src, pitch, fstride, n, &d, &dp, &dfs, crows, &sf);
    if (rc) return rc;
    dvc::FrontOut fo{};
    if (fused) {
        fo.ov = ov;
        fo.cp = cp;
        fo.opitch = opitch;
        fo.ostride = ostride;
        fo.quant = h->p.quant;
        fo.qinv = 1.0 / (double)h->p.quant;
        fo.M = h->M;
        fo.B = h->B;
        fo.i420 = out_i420 ? 1 : 0;
    }
    dvc::BackArgs a{};
    a.g = h->g;
    a.bgr = d;
    a.pitch = dp;
    a.fstride = dfs;
    a.sf = sf;
    a.acc = h->acc;
    a.ap = h->AP;
    a.overlay = ov;
    a.compressed = cp;
    a.opitch = opitch;
    a.ostride = ostride;
    a.obytes = obytes;
    a.out_i420 = out_i420 ? 1 : 0;
    a.kbits = S.c.kbits;
    a.kocc = S.c.kocc;
    a.docc = S.docc;
    a.dblk = S.dblk;
    a.rblk = S.rblk;
    a.sbits = S.sbits;
    a.SW = h->SW;
    a.sstride = h->sstride;
    a.dbits = S.dbits;
    a.rbits = S.rbits;
    a.zbits = S.zbits;
    a.B = h->B;
    a.NBX = h->NBX;
    a.NBY = h->NBY;
    a.n = n;
    a.ksize = h->p.ksize;
    a.anchor = h->p.anchor;
    a.alpha = h->p.alpha;
    a.beta = h->p.beta;
    a.gamma = h->p.gamma;
    a.quant = h->p.quant;
    a.qinv = 1.0 / (double)h->p.quant;
    a.acc0_fixed = dvc::acc_zero_fixed(h->p.alpha, h->p.beta, h->p.gamma);
    a.acc_fast = h->acc_short;
    const float dil1 = std::fmaf(255.0f, h->p.beta, h->p.gamma);
    std::memcpy(&a.dil1_bits, &dil1, 4);
    a.M = h->M;
    a.Mtab = h->Mtab;
    a.stats = h->stats;
    a.dbg_dil = h->dbg_dil;
    a.err = h->err;
    a.frame0 = h->frames;
    h->last_fused = fused;
    // the kept mask stays on chip: the filter stage ends in k_paint_dilate,
    // which writes the slot's dblk / docc, and the accumulate stage is k_acc
    // alone (DVC_FLAG_FD_KEPT_PLANE: k_paint -> kbits -> k_dilate instead)
    const bool onchip = !(h->p.flags & DVC_FLAG_FD_KEPT_PLANE) && dvc::fuse_paint_dilate(S.c, a);
    if (pl.graph && !pl.shared) {
        rc = graph_ccl(h, k, n);
        if (rc) return rc;
    }
    auto launch = [&](int sg, hipStream_t z) {
        switch (sg) {
        case dvc_sched::FRONT:
            return dvc::launch_front(d, dp, dfs, sf, n, h->gray[h->gcur], h->gray[h->gcur ^ 1], h->gs, S.c.mbits, h->g,
                                     h->p.ithresh, z, fused ? &fo : nullptr);
        case dvc_sched::FILTER:
            return dvc::launch_ccl(pl.shared ? S.c : S.gc, h->g, n, h->p.min_area2, z, onchip ? &a : nullptr);
        case dvc_sched::ACCUM: return dvc::launch_accumulate(a, z, onchip);
        default: return dvc::launch_out(a, z, fused);
        }
    };
    if (pl.graph) {
        std::vector<dvc::KNode> rec[4];
        hipError_t e[4];
        for (int sg = 0; sg < 4; ++sg) {
            dvc::g_krec = &rec[sg];
            e[sg] = launch(sg, h->graph_stream(k));
        }
        dvc::g_krec = nullptr;
        for (hipError_t x : e) HIP_OK(x);
        rc = enqueue_graph(h, k, rec, pl);
        if (rc) return rc;
    } else {
        // KTIMING: events around the dominant HBM kernel — the fused front on
        // s_front, else k_out on s_out
        const int tk = !timed ? -1 : fused ? dvc_sched::FRONT : dvc_sched::OUTPUT;
        while (timed && h->ev.size() < h->ev_used + 2) {
            hipEvent_t e;
            HIP_OK(hipEventCreate(&e));
            h->ev.push_back(e);
        }
        for (int sg = 0; sg < 4; ++sg) {
            hipStream_t z = h->stage_stream(sg);
            HIP_OK(h->wait(z, pl.stage[sg]));
            if (sg == tk) HIP_OK(hipEventRecord(h->ev[h->ev_used], z));
            if (!(skip >> sg & 1)) HIP_OK(launch(sg, z));
            if (sg == tk) {
                HIP_OK(hipEventRecord(h->ev[h->ev_used + 1], z));
                h->ev_used += 2;
            }
            if (pl.record[sg]) HIP_OK(hipEventRecord(S.ev[sg], z));
        }
    }
    dvc_sched::advance(h->sched, rq, pl);
    h->gcur ^= 1;
    h->frames += (uint64_t)n;
    h->last_n = n;
    return DVC_OK;
}

// Host-pointer chunk finished on the device: copy its pageable outputs out.
static int drain_stage(dvc_fd* h, Stage& st)
{
    if (!st.busy) return DVC_OK;
    HIP_OK(hipEventSynchronize(st.ev_d2h));
    const size_t N3 = h->ofb;
    for (int t = 0; t < st.m; ++t) {
        if (st.ov) std::memcpy(st.ov + (size_t)t * st.ostride, st.h_ov + (size_t)t * N3, N3);
        if (st.cp) std::memcpy(st.cp + (size_t)t * st.ostride, st.h_cp + (size_t)t * N3, N3);
    }
    st.busy = false;
    return DVC_OK;
}

// n frames in chunks of max_batch. Device pointers: enqueued, asynchronous.
// Host pointers: two staging sets pipeline the chunks — the frames of chunk
// c+1 are copied into pinned memory and sent up while chunk c computes and
// chunk c-1's outputs come down; pinned caller buffers (dvc_host_alloc) are
// DMA'd directly with no CPU copy. Returns once every output has landed.
static int run_frames(dvc_fd* h, const uint8_t* bgr, size_t pitch, size_t fstride, int n, uint8_t* overlay,
                      uint8_t* compressed, size_t ostride, uint8_t* acc_out)
{
    if (!h || !bgr) return fail(DVC_E_INVALID, "NULL argument");
    if (!h->primed) return fail(DVC_E_STATE, "step before dvc_fd_prime");
    if (h->failed) return fail(DVC_E_STATE, "the feed stopped at an odd-size DCT (frame %llu); prime again",
                               (unsigned long long)h->err_frame + 1);
    if (n < 0) return fail(DVC_E_INVALID, "negative frame count");
    const size_t W = h->p.width, H = h->p.height, N = W * H, srow = 3 * (size_t)h->sw;
    const bool yuv = h->fmt != DVC_FMT_BGR;
    if (!dvc_host::pitch_ok(h->frame(), pitch)) return fail(DVC_E_INVALID, "pitch %zu invalid", pitch);
    if (n > 1 && fstride < dvc_host::frame_span(h->frame(), pitch))
        return fail(DVC_E_INVALID, "frame stride %zu invalid", fstride);
    if (n > 1 && (overlay || compressed) && ostride < h->ofb)
        return fail(DVC_E_INVALID, "output frame stride %zu invalid", ostride);
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(h->wait_user());
    const bool devp = h->p.flags & DVC_FLAG_DEVICE_PTRS;
    if (devp) {
        const uint64_t first = h->sched.seq;
        for (int f0 = 0; f0 < n; f0 += h->max_batch) {
            const int m = std::min(h->max_batch, n - f0);
            int rc = enqueue_batch(h, bgr + (size_t)f0 * fstride, pitch, fstride, m,
                                   overlay ? overlay + (size_t)f0 * ostride : nullptr,
                                   compressed ? compressed + (size_t)f0 * ostride : nullptr, ostride, h->crows);
            if (rc) return rc;
        }
        // the acc copy and the caller's join follow the call's graph batches, which
        // ran on their slots' streams
        const dvc_sched::Join j = dvc_sched::join(h->sched, first, acc_out != nullptr, h->has_user);
        HIP_OK(h->wait(h->s_acc, j.acc));
        HIP_OK(h->wait(h->s_out, j.out));
        if (acc_out) HIP_OK(hipMemcpy2DAsync(acc_out, W, h->acc, h->AP, W, H, hipMemcpyDeviceToDevice, h->s_acc));
        if (j.record_acc)
            HIP_OK(hipEventRecord(h->slot[(h->sched.seq - 1) % NSLOT].ev[dvc_sched::ACCUM], h->s_acc));
        HIP_OK(join_user(h));
        return DVC_OK;
    }
    // page-locked frames are DMA'd directly; YUV ones only when already compact
    // (luma rows of W, chroma right after them), else repacked on the host
    const bool pin_in = host_pinned(bgr) && (!yuv || (pitch == (size_t)h->sw && h->crows == h->sh));
    const bool pin_out = (!overlay || host_pinned(overlay)) && (!compressed || host_pinned(compressed));
    const size_t N3 = h->ofb, sfs = (size_t)h->sip * h->sh;
    for (int f0 = 0; f0 < n; f0 += h->max_batch) {
        const int m = std::min(h->max_batch, n - f0);
        Stage& st = h->stage[h->next_stage];
        h->next_stage = (h->next_stage + 1) % NSTAGE;
        int rc = drain_stage(h, st);   // the chunk that used this set two chunks ago
        if (rc) return rc;
        const uint8_t* in = bgr + (size_t)f0 * fstride;
        uint8_t* ov = overlay ? overlay + (size_t)f0 * ostride : nullptr;
        uint8_t* cp = compressed ? compressed + (size_t)f0 * ostride : nullptr;
        HIP_OK(hipStreamWaitEvent(h->s_front, st.ev_free, 0));   // d_in / d_ov / d_cp of two chunks ago are done
        if (pin_in && yuv) {
            const size_t fb = dvc::yuv_frame_bytes(h->sw, h->sh);
            for (int t = 0; t < m; ++t)
                HIP_OK(hipMemcpyAsync(st.d_in + t * sfs, in + (size_t)t * fstride, fb, hipMemcpyHostToDevice,
                                      h->s_front));
        } else if (pin_in) {
            for (int t = 0; t < m; ++t)
                HIP_OK(hipMemcpy2DAsync(st.d_in + t * sfs, h->sip, in + (size_t)t * fstride, pitch, srow, h->sh,
                                        hipMemcpyHostToDevice, h->s_front));
        } else {
            HIP_OK(hipEventSynchronize(st.ev_h2d));   // h_in's previous upload is done
            for (int t = 0; t < m; ++t)
                dvc_host::pack_host_frame(h->frame(), in + (size_t)t * fstride, pitch, st.h_in + t * sfs, h->sip);
            HIP_OK(hipMemcpyAsync(st.d_in, st.h_in, (size_t)m * sfs, hipMemcpyHostToDevice, h->s_front));
            HIP_OK(hipEventRecord(st.ev_h2d, h->s_front));
        }
        rc = enqueue_batch(h, st.d_in, yuv ? h->sw : h->sip, sfs, m, ov ? st.d_ov : nullptr, cp ? st.d_cp : nullptr, N3,
                           h->sh);
        if (rc) return rc;
        if (pin_out) {
            if (ov) HIP_OK(hipMemcpy2DAsync(ov, ostride, st.d_ov, N3, N3, m, hipMemcpyDeviceToHost, h->s_out));
            if (cp) HIP_OK(hipMemcpy2DAsync(cp, ostride, st.d_cp, N3, N3, m, hipMemcpyDeviceToHost, h->s_out));
        } else {
            if (ov) HIP_OK(hipMemcpyAsync(st.h_ov, st.d_ov, (size_t)m * N3, hipMemcpyDeviceToHost, h->s_out));
            if (cp) HIP_OK(hipMemcpyAsync(st.h_cp, st.d_cp, (size_t)m * N3, hipMemcpyDeviceToHost, h->s_out));
        }
        HIP_OK(hipEventRecord(st.ev_d2h, h->s_out));
        HIP_OK(hipEventRecord(st.ev_free, h->s_out));
        st.busy = !pin_out && (ov || cp);
        st.m = m;
        st.ov = ov;
        st.cp = cp;
        st.ostride = ostride;
    }
    for (Stage& st : h->stage) {
        int rc = drain_stage(h, st);
        if (rc) return rc;
    }
    if (acc_out) {
        HIP_OK(hipMemcpy2DAsync(h->h_acc, W, h->acc, h->AP, W, H, hipMemcpyDeviceToHost, h->s_acc));
        HIP_OK(hipStreamSynchronize(h->s_acc));
        std::memcpy(acc_out, h->h_acc, N);
    }
    HIP_OK(h->sync());
    HIP_OK(join_user(h));
    return check_stop(h);
}

extern "C" {

int dvc_fd_step(dvc_fd* h, const uint8_t* bgr, size_t pitch, uint8_t* overlay, uint8_t* compressed,
                uint8_t* acc_out)
{
    return run_frames(h, bgr, pitch, 0, 1, overlay, compressed, 0, acc_out);
}

int dvc_fd_step_batch(dvc_fd* h, const uint8_t* bgr, size_t pitch, size_t frame_stride, int n, uint8_t* overlay,
                      uint8_t* compressed, size_t out_stride)
{
    return run_frames(h, bgr, pitch, frame_stride, n, overlay, compressed, out_stride, nullptr);
}

int dvc_fd_sync(dvc_fd* h)
{
    if (!h) return fail(DVC_E_INVALID, "NULL handle");
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(h->sync());
    return check_stop(h);
}

int dvc_fd_get_stats(dvc_fd* h, dvc_fd_stats* out)
{
    if (!h || !out) return fail(DVC_E_INVALID, "NULL argument");
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(h->sync());
    (void)check_stop(h);
    unsigned long long s[4];
    HIP_OK(dvc_host::fold_stats(h->stats, s));
    out->frames = h->failed ? std::min<uint64_t>(h->frames, h->err_frame) : h->frames;
    out->motion_px = s[1];
    out->components = s[2];
    out->static_blocks = s[3];
    return DVC_OK;
}

int dvc_fd_read_plane(dvc_fd* h, int plane, uint8_t* dst)
{
    if (!h || !dst) return fail(DVC_E_INVALID, "NULL argument");
    if (!h->primed) return fail(DVC_E_STATE, "read_plane before dvc_fd_prime");
    if (!h->frames && plane != DVC_PLANE_GRAY && plane != DVC_PLANE_ACC)
        return fail(DVC_E_STATE, "no frame stepped yet");
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(h->sync());
    const size_t W = h->p.width, H = h->p.height, WW = h->g.WW;
    if (plane == DVC_PLANE_GRAY) {
        HIP_OK(hipMemcpy2D(dst, W, h->gray[h->gcur], h->gs, W, H, hipMemcpyDeviceToHost));
        return DVC_OK;
    }
    if (plane == DVC_PLANE_ACC) {
        HIP_OK(hipMemcpy2D(dst, W, h->acc, h->AP, W, H, hipMemcpyDeviceToHost));
        return DVC_OK;
    }
    // the last frame of the last batch
    const dvc::CclBufs c = h->slot[(h->sched.seq - 1) % NSLOT].c.frame((size_t)h->last_n - 1, h->g);
    const uint64_t* src = plane == DVC_PLANE_MOTION ? c.mbits
                        : plane == DVC_PLANE_FILTERED ? c.kbits
                        : plane == DVC_PLANE_DILATED ? h->dbg_dil : nullptr;
    if (plane != DVC_PLANE_MOTION && plane != DVC_PLANE_FILTERED && plane != DVC_PLANE_DILATED)
        return fail(DVC_E_INVALID, "unknown plane %d", plane);
    if (!src) return fail(DVC_E_STATE, "plane %d needs DVC_FLAG_KEEP_PLANES", plane);
    HIP_OK(dvc_host::read_bit_plane(src, W, H, WW, dst));
    return DVC_OK;
}

int dvc_fd_ktime(dvc_fd* h, double* total_ms, uint64_t* launches, int reset)
{
    if (!h) return fail(DVC_E_INVALID, "NULL handle");
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(h->sync());
    hipError_t e = hipSuccess;
    const double t = dvc_host::ktime_sum(h->ev, h->ev_used, &e);
    HIP_OK(e);
    if (total_ms) *total_ms = t;
    if (launches) *launches = h->ev_used / 2;
    if (reset) h->ev_used = 0;
    return DVC_OK;
}

int dvc_fd_graph_stats(const dvc_fd* h, uint64_t* batches, uint64_t* builds)
{
    if (!h) return fail(DVC_E_INVALID, "NULL handle");
    if (batches) *batches = h->graph_batches;
    if (builds) *builds = h->graph_builds;
    return DVC_OK;
}

int dvc_fd_ktime_kernel(const dvc_fd* h)
{
    if (!h) return fail(DVC_E_INVALID, "NULL handle");
    return h->last_fused ? DVC_KTIME_FRONT_FUSED : DVC_KTIME_OUT;
}

int dvc_fd_acc_form(const dvc_fd* h)
{
    if (!h) return fail(DVC_E_INVALID, "NULL handle");
    if (!dvc::fast_block(h->B)) return DVC_ACC_FORM_ROWS;
    return h->acc_short ? DVC_ACC_FORM_SHORT : DVC_ACC_FORM_GENERAL;
}

void dvc_fd_destroy(dvc_fd* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)h->sync();
    delete h;
}

int dvc_contour_filter(const uint8_t* mask, int width, int height, int64_t min_area2, int device,
                       uint8_t* filtered, uint64_t* components)
{
    if (!mask || !filtered) return fail(DVC_E_INVALID, "NULL argument");
    if (width < 4 || height < 4 || width > 65520)
        return fail(DVC_E_INVALID, "mask %dx%d: sides must be 4..65520", width, height);
    HIP_OK(hipSetDevice(device));
    dvc::RowGeom g{width, height, (width + 63) / 64, width / 2 + 1};
    const size_t W = width, H = height, WW = g.WW;
    std::vector<uint64_t> bits(H * WW, 0);
    for (size_t y = 0; y < H; ++y)
        for (size_t x = 0; x < W; ++x)
            if (mask[y * W + x]) bits[y * WW + x / 64] |= 1ull << (x % 64);
    dvc::CclBufs c{};
    size_t sz[dvc::CclBufs::NARR];
    void** ptrs[dvc::CclBufs::NARR];
    dvc::CclBufs::sizes(g, 1, sz);
    c.ptrs(ptrs);
    unsigned long long* stats = nullptr;
    dvc_host::DevMem mem;   // every allocation is checked before any launch; freed on return
    hipError_t e = mem.alloc(&stats, 8 * 4 * 64);
    for (int i = 0; i < dvc::CclBufs::NARR && e == hipSuccess; ++i) e = mem.alloc(ptrs[i], sz[i]);
    if (e != hipSuccess) return fail(DVC_E_NOMEM, "hipMalloc failed");
    c.stats = stats;
    hipStream_t s = nullptr;
    e = hipMemcpy(c.mbits, bits.data(), 8 * H * WW, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(stats, 0, 8 * 4 * 64);
    if (e == hipSuccess) e = hipMemset(c.gpar, 0, sz[dvc::CclBufs::I_GPAR]);
    if (e == hipSuccess) e = dvc::launch_ccl(c, g, 1, min_area2, s);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long st[4];
    if (e == hipSuccess) e = dvc_host::fold_stats(stats, st);
    if (e == hipSuccess) e = dvc_host::read_bit_plane(c.kbits, W, H, WW, filtered);   // writes only when it succeeds
    if (e != hipSuccess) return fail(DVC_E_HIP, "contour filter: %s", hipGetErrorString(e));
    if (components) *components = st[2];
    return DVC_OK;
}

}  // extern "C"
