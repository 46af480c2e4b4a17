// fd_sched.h — which events each stage of an FD batch waits for and records:
// the ordering policy of fd_api.hip in one place, plain C++ (no HIP header).
// fd_api.hip executes the plan and decides nothing itself; the host check
// (tools/fd_sched_host_check.cc, tests/test_fd_sched.py) feeds sequences of
// requests through it and asserts, from the buffer table below, that any two
// stage executions that touch one buffer, one of them writing, are ordered.
//
// A batch i runs in slot i % NSLOT as four stages. An event is named
// (slot, stage): fd_api.hip's Slot::ev[stage], recorded after that stage of the
// slot's latest batch. A wait for a slot's event refers to the record that is
// the latest when the wait is issued, so a stage that waits for its own slot's
// later stage means the slot's previous batch (i - NSLOT).
//   stage streams: front on s_front, filter on the handle's stream, accumulate
//       on s_acc, output on s_out; each stage waits, launches, records. The two
//       recurrences (previous gray, accumulated mask) are stream order.
//   graph: the four stages are one chain on the slot's own stream (slot k:
//       handle's stream, s_acc, s_out, s_front), with wait and record nodes in
//       the chain; the recurrences come from the previous batch's events.
#pragma once
#include <cstdint>

#ifndef DVC_GRAPH_OWN_CCL_FRAMES
#define DVC_GRAPH_OWN_CCL_FRAMES 128
#endif

namespace dvc_sched {

// Batches in flight: four slots (the graph path launches each slot's batches
// on its own stream, so up to four short batches overlap; the stage streams
// keep the four stages of four batches in flight).
constexpr int NSLOT = 4;
// graph batches up to this many frames run their contour filter on the slot's
// own working set (consecutive batches' filters overlap; four sets of up to
// 128 1080p frames are ~9 GB); longer ones on the shared set the stage
// streams use, after its previous user's filter
constexpr int GRAPH_OWN_CCL_FRAMES = DVC_GRAPH_OWN_CCL_FRAMES;

enum { FRONT, FILTER, ACCUM, OUTPUT, NSTG };

// The stream a slot's graphs are launched on, as the stage whose stream it is:
// one of the four per slot (each its own hardware queue at the default 4), so
// consecutive batches' graphs overlap — batch i's filter beside batch i+1's front
constexpr int slot_stream(int slot) { return slot == 0 ? FILTER : slot == 1 ? ACCUM : slot == 2 ? OUTPUT : FRONT; }

// The host check's control build (-DDVC_SCHED_BEFORE_FIXES) leaves out the three
// orderings that the schedule lacked before this header, so the check can show
// that it finds them: a caller's stream joined only to the call's last graph
// batch, unfused graph batches that overwrite one output set, and the copy of
// the accumulated mask against the next call's accumulate on another stream.
#ifdef DVC_SCHED_BEFORE_FIXES
constexpr bool CLOSED = false;
#else
constexpr bool CLOSED = true;
#endif

// ------------------------------------------------------------- buffers ----
// What a stage reads and writes. Per slot: FIN, MBITS, OWN_SET, KEPT, RESULT;
// per handle: the two gray planes, SHARED_SET, ACC; OUTPUTS are the request's
// byte ranges; FRAMES are the caller's and only read. The filter runs on
// SHARED_SET or OWN_SET (Plan::shared). stats and err are atomics, left out.
enum Buf {
    GRAY_CUR,    // previous blurred gray, gray[cur]
    GRAY_NEXT,   // gray[cur ^ 1]: the next batch's GRAY_CUR
    FRAMES,      // the input frames, where read in place
    FIN,         // the slot's staged frames (fin / fsrc)
    MBITS,       // motion bits
    SHARED_SET,  // the filter's working set all slots share
    OWN_SET,     // the slot's own (Slot::gc)
    KEPT,        // dblk / docc, or kbits / kocc
    ACC,         // the accumulated mask
    RESULT,      // rblk / sbits (generic back end: dbits / rbits / zbits)
    OUTPUTS,     // overlay and compressed frames
    NBUF
};
constexpr int STAGING = NSTG;   // pseudo-stage: on s_front before the front, when the frames are staged

struct Access {
    unsigned reads, writes;   // bit per Buf
};
constexpr unsigned bit(Buf b) { return 1u << b; }

constexpr Access access(int stage, bool fused, bool staged, bool shared)
{
    const unsigned in = bit(staged ? FIN : FRAMES), set = bit(shared ? SHARED_SET : OWN_SET);
    return stage == STAGING ? Access{bit(FRAMES), bit(FIN)}
         : stage == FRONT   ? Access{bit(GRAY_CUR) | in, bit(GRAY_NEXT) | bit(MBITS) | (fused ? bit(OUTPUTS) : 0u)}
         : stage == FILTER  ? Access{bit(MBITS) | set, set | bit(KEPT)}
         : stage == ACCUM   ? Access{bit(KEPT) | bit(ACC), bit(ACC) | bit(RESULT)}
                            : Access{bit(RESULT) | in, bit(OUTPUTS)};
}

// --------------------------------------------------------------- state ----
struct SlotState {
    bool recorded = false;   // its events hold a batch the slot's next user must wait for
    bool graph = false;      // that batch ran as a graph
    bool shared = false;     // its filter ran on the shared set (and recorded the filter event)
    // the output bytes it writes ([lo, hi) of overlay and compressed; empty when not requested)
    uintptr_t olo[2] = {0, 0}, ohi[2] = {0, 0};
};

struct State {   // State{} after a sync of every stream: a new run
    SlotState slot[NSLOT];
    uint64_t seq = 0;          // batches launched
    bool prev_graph = false;   // the last one ran as a graph
};

struct Request {
    int n = 0;                                   // frames
    uintptr_t olo[2] = {0, 0}, ohi[2] = {0, 0};  // output byte ranges, as in SlotState
    bool staged = false;     // the kernels cannot read the frames in place
    bool graph_ok = false;   // graphs on, device pointers, not timed, no stage ablated
    bool fused = false;      // the front writes the outputs speculatively, the output stage fixes them up
};

// ---------------------------------------------------------------- plan ----
struct Ev {
    int8_t slot, stage;
};
inline bool operator==(Ev a, Ev b) { return a.slot == b.slot && a.stage == b.stage; }

struct Waits {
    static constexpr int MAX = NSLOT + 2;   // the stream front: front(P), filter(S), every slot's output
    int n = 0;
    Ev e[MAX] = {};
    void add(int slot, int stage)
    {
        const Ev x{(int8_t)slot, (int8_t)stage};
        for (int i = 0; i < n; ++i)
            if (e[i] == x) return;
        e[n++] = x;
    }
    void add(const Waits& w)
    {
        for (int i = 0; i < w.n; ++i) add(w.e[i].slot, w.e[i].stage);
    }
};

struct Plan {
    bool graph = false;    // one graph on the slot's stream, else the stage streams
    bool shared = false;   // the filter runs on the shared working set
    // before anything of the batch starts: on the slot's stream before the graph
    // launch; on s_front before staging (there these are the front's waits)
    Waits pre;
    // before the stage, on its stream or as nodes in the chain (accumulate in a
    // graph: before the stage's last kernel, k_acc; a k_dilate before it touches
    // only the slot's own KEPT, free since `pre`)
    Waits stage[NSTG];
    bool record[NSTG] = {};   // the stage records its event
};

// The plan of the next batch (S its slot, P the previous batch's). Only the
// last NSLOT batches have events; they reach every earlier one, since a batch
// waits for its slot's previous batch and the stage streams run in order.
inline Plan plan(const State& st, const Request& rq)
{
    Plan p;
    const int s = (int)(st.seq % NSLOT), pv = (int)((st.seq + NSLOT - 1) % NSLOT);
    const SlotState &S = st.slot[s], &P = st.slot[pv];
    Waits over;   // batches in flight whose output bytes overlap this one's
    for (int k = 1; k < NSLOT; ++k) {
        const int q = (int)((st.seq + NSLOT - k) % NSLOT);
        const SlotState& Q = st.slot[q];
        bool hit = false;
        for (int u = 0; u < 2; ++u)
            for (int v = 0; v < 2; ++v)
                hit = hit || (rq.ohi[u] > rq.olo[u] && Q.ohi[v] > Q.olo[v] && rq.olo[u] < Q.ohi[v] && Q.olo[v] < rq.ohi[u]);
        if (Q.recorded && hit) over.add(q, OUTPUT);
    }
    // Not a graph: a long batch whose outputs overlap a batch in flight (one
    // output set re-used). Its front then waits for that batch's whole chain, a
    // path the stage streams run ~3 % faster (experiments/README.md round 6).
    p.graph = rq.graph_ok && !rq.staged && (rq.n <= GRAPH_OWN_CCL_FRAMES || over.n == 0);
    if (p.graph) {
        p.shared = rq.n > GRAPH_OWN_CCL_FRAMES;
        // every buffer of the slot is free; and no earlier batch still writes
        // these output bytes (a fused front writes them before the earlier
        // fix-up has run; the output stages of graph batches run on different
        // streams in no order of their own)
        if (S.recorded) p.pre.add(s, OUTPUT);
        if (rq.fused || CLOSED) p.pre.add(over);
        // the recurrences, and the shared set's previous user: the previous
        // batch's filter when it ran there, else its accumulate (which follows
        // every earlier batch's accumulate, each after its filter). The nodes are
        // there whether or not P holds a batch: a graph is re-used across runs.
        p.stage[FRONT].add(pv, FRONT);
        if (p.shared) p.stage[FILTER].add(pv, P.recorded && P.graph && !P.shared ? ACCUM : FILTER);
        p.stage[ACCUM].add(pv, ACCUM);
        // (an own-set filter records nothing: an event node costs ~5 us of the chain's latency)
        for (int sg = 0; sg < NSTG; ++sg) p.record[sg] = sg != FILTER || p.shared;
        return p;
    }
    p.shared = true;
    if (st.prev_graph) {   // the stage streams take up the recurrences from the previous batch's events
        p.pre.add(pv, FRONT);
        p.stage[FILTER].add(pv, P.shared ? FILTER : ACCUM);
        p.stage[ACCUM].add(pv, ACCUM);
        p.stage[OUTPUT].add(pv, OUTPUT);
    }
    if (S.recorded) {
        p.pre.add(s, S.graph ? OUTPUT : FILTER);               // MBITS is free
        if (rq.staged || rq.fused) p.pre.add(s, OUTPUT);       // FIN is; every fix-up up to the slot's is done
    }
    if (rq.fused) p.pre.add(over);
    p.stage[FILTER].add(s, FRONT);
    if (S.recorded) p.stage[FILTER].add(s, ACCUM);   // KEPT is free
    p.stage[ACCUM].add(s, FILTER);
    if (S.recorded) p.stage[ACCUM].add(s, OUTPUT);   // RESULT is free
    p.stage[OUTPUT].add(s, ACCUM);
    for (bool& r : p.record) r = true;
    return p;
}

// The batch is enqueued.
inline void advance(State& st, const Request& rq, const Plan& p)
{
    SlotState& S = st.slot[st.seq % NSLOT];
    S.recorded = true;
    S.graph = p.graph;
    S.shared = p.shared;
    for (int u = 0; u < 2; ++u) {
        S.olo[u] = rq.olo[u];
        S.ohi[u] = rq.ohi[u];
    }
    st.prev_graph = p.graph;
    st.seq++;
}

// The end of a call whose first batch had sequence number `first`: what s_acc
// waits for before the copy of the accumulated mask, and s_out, before the
// caller's stream is joined to both. A graph batch's stages ran on its slot's
// stream, so the call's graph batches are joined one by one (the last NSLOT
// reach the earlier ones).
struct Join {
    Waits acc, out;
    // With no caller's stream to fork the next call from, the copy is ordered
    // before the next batch's accumulate by recording accumulate(last) again
    // behind it on s_acc (the stage streams alone would do: s_acc runs in order).
    bool record_acc = false;
};

inline Join join(const State& st, uint64_t first, bool acc_out, bool has_user)
{
    Join j;
    if (!acc_out && !has_user) return j;
    const int last = (int)((st.seq + NSLOT - 1) % NSLOT);
    j.record_acc = CLOSED && acc_out && !has_user && st.slot[last].recorded;
    if (st.prev_graph) {
        j.acc.add(last, ACCUM);
        j.out.add(last, OUTPUT);
    }
    for (uint64_t k = 1; CLOSED && has_user && k <= NSLOT && k <= st.seq - first; ++k) {
        const int q = (int)((st.seq - k) % NSLOT);
        if (st.slot[q].graph) j.out.add(q, OUTPUT);
    }
    return j;
}

}  // namespace dvc_sched
