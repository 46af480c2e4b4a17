"""The FD ordering plan (csrc/fd_sched.h) on the CPU: tools/fd_sched_host_check.cc
feeds every sequence of up to 9 batches through the plan the way fd_api.hip
executes it, builds what happens before what (stream order, event records and
waits, graph chains, the caller's fork and join) and counts the pairs of stage
executions that touch one buffer, one of them writing, with no order between
them: none. The same program built with -DDVC_SCHED_BEFORE_FIXES (the plan
without the orderings it added to the schedule it transcribes) must find the
gaps, so the count of zero means something. The plans of a few fixed sequences
are pinned to a literal table: a change of any ordering fails by name."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, name, *flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, "-o", str(exe),
                    os.path.join(ROOT, "tools", "fd_sched_host_check.cc")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("fd_sched"), "fd_sched_host_check")


def _ordered(rep):
    assert rep["closed"] is True
    assert rep["one_call_of_8"] == 0 and rep["unfused_one_set_12"] == 0
    ex = rep["exhaustive"]
    assert ex["max_batches"] == 9 and ex["sequences"] > 5_000_000
    assert ex["pairs"] == 0 and ex["by_kind"] == {}, ex["by_kind"]


def test_every_sequence_is_ordered(report):
    _ordered(report)


def test_every_sequence_is_ordered_under_sanitizers(tmp_path):
    _ordered(_run(tmp_path, "fd_sched_host_check_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def test_the_check_finds_the_gaps_the_plan_closed(tmp_path):
    """Without the plan's added orderings: one call of eight one-frame graph
    batches on a caller's stream leaves batch 4's output stage (on the filter
    stream, which nothing joined follows) unordered with the caller's read;
    twelve unfused per-frame graph calls into one output set leave the output
    stages of (i, i+1), (i, i+2), (i, i+3) unordered, 11 + 10 + 9 pairs; and,
    with no caller's stream, the copy of the accumulated mask on s_acc is
    unordered with the next call's accumulate on another stream. Nothing else."""
    rep = _run(tmp_path, "fd_sched_host_check_before", "-DDVC_SCHED_BEFORE_FIXES")
    assert rep["closed"] is False
    assert rep["one_call_of_8"] == 1
    assert rep["unfused_one_set_12"] == 30
    kinds = rep["exhaustive"]["by_kind"]
    assert set(kinds) == {"output/read/outputs", "output/output/outputs", "acc_copy/accumulate/acc"}, kinds
    assert all(v > 0 for v in kinds.values())


# ------------------------------------------------------- pinned plans ----
# (slot, path, before the batch, front, filter, accumulate, output, records)
# as fd_api.hip had them before the plan was a header, F/C/A/O = the front /
# filter / accumulate / output event. Written out by hand from that code:
#   stage streams, batch i >= 4 in slot S: s_front waits filter(S) (the motion
#   bits are free; output(S) when the slot's batch was a graph), and output(S)
#   when staging or fused, and the overlapping outputs when fused; the filter
#   waits front(S new), accumulate(S old); accumulate waits filter(S new),
#   output(S old); output waits accumulate(S new). After a graph batch P each
#   stage stream first waits P's event of its stage (the filter: P's
#   accumulate if P's filter ran on its own set).
#   graph, batch in slot S after P: before the launch output(S) and the
#   overlapping outputs; in the chain front waits front(P), accumulate waits
#   accumulate(P), a shared-set filter waits filter(P) (accumulate(P) after an
#   own-set graph batch) and only then records C.
S, GO, GS = "stream", "graph, own set", "graph, shared set"


def _stream_fill(k):      # the first four stream batches: nothing to wait for but the batch's own stages
    return (k, S, "", "", f"front({k})", f"filter({k})", f"accumulate({k})", "FCAO")


def _stream_steady(k):
    return (k, S, f"filter({k}) output({k})", "", f"front({k}) accumulate({k})", f"filter({k}) output({k})",
            f"accumulate({k})", "FCAO")


def _graph_short(k, pre):
    p = (k + 3) % 4
    return (k, GO, pre, f"front({p})", "", f"accumulate({p})", "", "FAO")


def _graph_long(k, pre, filt=None):
    p = (k + 3) % 4
    return (k, GS, pre, f"front({p})", filt or f"filter({p})", f"accumulate({p})", "", "FCAO")


_ONE_SET = [_graph_short(0, ""), _graph_short(1, "output(0)"), _graph_short(2, "output(1) output(0)"),
            _graph_short(3, "output(2) output(1) output(0)"),
            _graph_short(0, "output(0) output(3) output(2) output(1)"),
            _graph_short(1, "output(1) output(0) output(3) output(2)")]

PLANS = {
    # fused, frames in place, distinct outputs
    "stream": [_stream_fill(0), _stream_fill(1), _stream_fill(2), _stream_fill(3), _stream_steady(0), _stream_steady(1)],
    # staging waits output(S) as fusing does; the stage streams need no overlap waits (s_out runs in order)
    "stream_staged_unfused_one_set": [_stream_fill(0), _stream_fill(1), _stream_fill(2), _stream_fill(3),
                                      _stream_steady(0), _stream_steady(1)],
    # per-frame graph calls into one output set
    "graph_short_one_set": _ONE_SET,
    # ... unfused: the same waits (before the plan: output(S) alone, the output stages unordered)
    "graph_short_unfused_one_set": _ONE_SET,
    "graph_long": [_graph_long(0, ""), _graph_long(1, ""), _graph_long(2, ""), _graph_long(3, ""),
                   _graph_long(0, "output(0)"), _graph_long(1, "output(1)")],
    # a long batch whose outputs overlap a batch in flight takes the streams
    "graph_long_two_sets": [
        _graph_long(0, ""), _graph_long(1, ""),
        (2, S, "front(1) output(0)", "", "filter(1) front(2)", "accumulate(1) filter(2)", "output(1) accumulate(2)",
         "FCAO"),
        (3, S, "output(1)", "", "front(3)", "filter(3)", "accumulate(3)", "FCAO"),
    ],
    # short graph, long graph, stream, short graph, staged stream, long graph, short graph, stream
    "mixed": [
        _graph_short(0, ""),
        _graph_long(1, "", "accumulate(0)"),
        (2, S, "front(1)", "", "filter(1) front(2)", "accumulate(1) filter(2)", "output(1) accumulate(2)", "FCAO"),
        _graph_short(3, ""),
        (0, S, "front(3) output(0)", "", "accumulate(3) front(0) accumulate(0)", "accumulate(3) filter(0) output(0)",
         "output(3) accumulate(0)", "FCAO"),
        _graph_long(1, "output(1)"),
        _graph_short(2, "output(2)"),
        (3, S, "front(2) output(3)", "", "accumulate(2) front(3) accumulate(3)", "accumulate(2) filter(3) output(3)",
         "output(2) accumulate(3)", "FCAO"),
    ],
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_is_the_pinned_one(report, name):
    got = [(b["slot"], b["path"], *(" ".join(b[k]) for k in ("pre", "front", "filter", "accumulate", "output")),
            b["records"]) for b in report["plans"][name]]
    assert got == PLANS[name]


def test_every_printed_plan_is_pinned(report):
    assert sorted(report["plans"]) == sorted(PLANS)
