"""CPU side of the history delta (gns_ex_hist_rollup_between, gns_ex_movers): HistPlan::between
in a stand-alone program built with ASan + UBSan, the truth module against hand-written cases,
the header and the ctypes binding of the two calls, and the Python argument errors that come
before any device call."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from history_delta_truth import (M64, StoredTruth, delta_truth, group_signed, movers_truth, rowlog_delta, rowlog_sets,
                                 signed, window_sets)
from history_rollup_truth import RowLog
from history_truth import HistoryTruth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "go2netspectra_amd", "csrc")
HEADER = os.path.join(HERE, "..", "include", "gns_sketch.h")
I64 = np.iinfo(np.int64)

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "gns_histplan.hpp"

// commands, one per line:  a <t> <n>  publish a snapshot of n rows
//   b <has0> <t0> <has1> <t1>  between(has0 ? &t0 : null, has1 ? &t1 : null): prints
//                              b bad empty s0 s1 minus_end scan_end
//   t <before> <fold> <nbase>  trim_plan + trimmed(nbase) unless a noop; the plan is replaced
int main() {
    gns::HistPlan p;
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        long long a = 0, b = 0;
        unsigned long long u = 0;
        int h0 = 0, h1 = 0, fold = 0;
        switch (cmd) {
        case 'a':
            if (std::scanf("%lld %llu", &a, &u) != 2) return 2;
            if (p.append_check((int64_t)a, u) != gns::HIST_OK) return 4;
            p.publish((int64_t)a, u);
            break;
        case 'b': {
            if (std::scanf("%d %lld %d %lld", &h0, &a, &h1, &b) != 4) return 2;
            const int64_t t0 = (int64_t)a, t1 = (int64_t)b;
            const gns::HistPlan::Between w = p.between(h0 ? &t0 : nullptr, h1 ? &t1 : nullptr);
            std::printf("b %d %d %lld %lld %llu %llu\n", w.bad ? 1 : 0, w.empty ? 1 : 0, (long long)w.s0, (long long)w.s1,
                        (unsigned long long)w.minus_end, (unsigned long long)w.scan_end);
            break;
        }
        case 't': {
            if (std::scanf("%lld %d %llu", &a, &fold, &u) != 3) return 2;
            const gns::HistPlan::Trim t = p.trim_plan((int64_t)a, fold != 0);
            if (!t.noop) p = p.trimmed(t, u);
            break;
        }
        default: return 3;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("histdelta")
    src, exe = tmp / "histdelta_driver.cpp", str(tmp / "histdelta_driver")
    src.write_text(DRIVER)
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-3000:]
        return [[int(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines()]
    return run


# --- HistPlan::between ---
TSX = [-(1 << 62), -5, -4, 0, 7, 1 << 40]
ROWSX = [3, 0, 10, 0, 0, 257]  # snapshots without rows among them, one inside every longer window


def model_between(ts, rows, T0, T1):
    """[bad, empty, s0, s1, minus_end, scan_end] as the issue's semantics define them."""
    if T0 is not None and T1 is not None and T0 > T1:
        return [1, 1, -1, -1, 0, 0]
    s = lambda T: sum(1 for t in ts if t <= T) - 1
    s1 = len(ts) - 1 if T1 is None else s(T1)
    s0 = -1 if T0 is None else min(s(T0), s1)
    if s1 < 0 or s0 == s1:
        return [0, 1, s0, s1, 0, 0]
    return [0, 0, s0, s1, sum(rows[:s0 + 1]), sum(rows[:s1 + 1])]


def ask(T0, T1):
    return f"b {int(T0 is not None)} {T0 or 0} {int(T1 is not None)} {T1 or 0}"


def test_between_at_every_boundary(driver):
    times = sorted({t + d for t in TSX for d in (-1, 0, 1)} | {-(1 << 63), (1 << 63) - 1}) + [None]
    pairs = [(a, b) for a in times for b in times]
    out = driver([ask(5, 4), ask(4, 4), ask(None, None), ask(3, None)] + [f"a {t} {n}" for t, n in zip(TSX, ROWSX)] +
                 [ask(a, b) for a, b in pairs])
    # an empty plan: T0 > T1 is bad, everything else is empty
    assert out[:4] == [[1, 1, -1, -1, 0, 0]] + [[0, 1, -1, -1, 0, 0]] * 3
    kinds = set()
    for (a, b), got in zip(pairs, out[4:]):
        want = model_between(TSX, ROWSX, a, b)
        assert got == want, (a, b, got, want)
        bad, empty, s0, s1, minus_end, scan_end = got
        kinds.add("bad" if bad else "before" if s1 < 0 else "same" if s0 == s1 else "open" if s0 < 0 else "window")
        if not bad and not empty:
            assert minus_end <= scan_end
    assert kinds == {"bad", "before", "same", "open", "window"}
    # equal times; before the first snapshot; an empty snapshot inside the window
    assert model_between(TSX, ROWSX, 0, 0)[:2] == [0, 1] and model_between(TSX, ROWSX, -(1 << 63), TSX[0] - 1)[:2] == [0, 1]
    assert model_between(TSX, ROWSX, -5, 7) == [0, 0, 1, 4, 3, 13]  # snapshots 3 and 4 hold no rows
    assert model_between(TSX, ROWSX, -4, 7) == [0, 0, 2, 4, 13, 13]  # a window of empty snapshots scans, selects nothing
    assert model_between(TSX, ROWSX, 1 << 41, None) == [0, 1, 5, 5, 0, 0]  # a start after the newest snapshot


def test_between_after_a_trim(driver):
    pub = [f"a {t} {n}" for t, n in zip(TSX, ROWSX)]
    # fold: snapshots 0..2 become one base of 11 rows under -4; drop: snapshots 0..2 are gone
    for fold, nbase, ts, rows in ((1, 11, [-4, 0, 7, 1 << 40], [11, 0, 0, 257]), (0, 0, [0, 7, 1 << 40], [0, 0, 257])):
        times = [-(1 << 62), -5, -4, -1, 0, 7, 8, 1 << 40, None]
        pairs = [(a, b) for a in times for b in times if a is None or b is None or a <= b]
        out = driver(pub + [f"t 0 {fold} {nbase}"] + [ask(a, b) for a, b in pairs])
        for (a, b), got in zip(pairs, out):
            assert got == model_between(ts, rows, a, b), (fold, a, b)
        if fold:  # a start before the base is no start at all
            i, j = pairs.index((-5, None)), pairs.index((None, None))
            assert out[i] == out[j] == [0, 0, -1, 3, 0, 268]


# --- the truth module against hand-written cases ---
def truth_of(snaps, full=None):
    tr = HistoryTruth(["SrcIP", "SrcPort"]) if full is None else StoredTruth(["SrcIP", "SrcPort"], full)
    for ts, export in snaps:
        tr.record(ts, export)
    return tr


A, B, C = "10.0.0.1-1", "10.0.0.1-2", "10.0.0.2-1"
ip = lambda d: bytes(10) + b"\xff\xff" + bytes([10, 0, 0, d])


def test_truth_by_hand():
    # rows are (start, end, packets, bytes); at 20 A grows, B is unchanged, C appears; at 30 A returns smaller
    snaps = [(10, {A: (5, 6, 2, 200), B: (1, 9, 1, 10)}),
             (20, {A: (5, 8, 3, 300), B: (1, 9, 1, 10), C: (-7, 7, 4, 40)}),
             (30, {A: (50, 60, 1, 100), B: (1, 9, 1, 10), C: (-7, 7, 4, 40)})]
    whole, delta = truth_of(snaps), truth_of(snaps, full=[True, False, False])
    assert len(whole.ts) == 8 and len(delta.ts) == 5  # the delta store skips the unchanged rows
    for tr in (whole, delta):
        rows, n = delta_truth(tr, 10, 20, ["SrcIP", "SrcPort"])
        assert rows == [(ip(1) + b"\0\1", 5, 8, 1, 100), (ip(2) + b"\0\1", -7, 7, 4, 40)]
        assert n == (5 if tr is whole else 3)  # whole views: B's plus and minus row cancel and are still selected
        assert delta_truth(tr, None, 20, ["SrcIP"])[0] == [(ip(1), 1, 9, 4, 310), (ip(2), -7, 7, 4, 40)]
        assert delta_truth(tr, 20, 30, ["SrcIP"])[0] == [(ip(1), 1 if tr is whole else 50, 60, (-2) & M64, (-200) & M64)]
        assert delta_truth(tr, 10, 30, ["SrcIP", "SrcPort"])[0] == [
            (ip(1) + b"\0\1", 50, 60, (-1) & M64, (-100) & M64), (ip(2) + b"\0\1", -7, 7, 4, 40)]
        for T0, T1 in ((10, 10), (12, 19), (5, 9), (30, None), (31, 40)):
            assert delta_truth(tr, T0, T1, ["SrcIP"]) == ([], 0), (T0, T1)
        assert delta_truth(tr, 5, 10, ["SrcIP"]) == delta_truth(tr, None, 10, ["SrcIP"]) == ([(ip(1), 1, 9, 3, 210)], 2)
    plus, minus = window_sets(delta, 10, 30)
    assert (plus, minus) == ([3, 4], [0])  # A's newest row and C's; A's first row.  A's middle row lived only inside
    # the times of a coarser group: whole views widen them by the plus rows of unchanged flows
    assert delta_truth(whole, 20, 30, ["SrcIP"])[0][0][1:3] == (1, 60) and delta_truth(delta, 20, 30, ["SrcIP"])[0][0][1:3] == (50, 60)


def test_group_signed_and_movers_by_hand():
    keys = np.array([[1], [1], [2], [3], [3], [4]], np.uint8)
    u = lambda xs: np.array(xs, np.uint64)
    # plus rows: key 1 (x2), 2, 3; minus rows: key 3 (equal packets), key 4 (no plus row)
    rows = group_signed(keys, [5, -5, 0, 1, 9, 9], [6, 7, 0, 2, 9, 9], u([1, 2, 1 << 63, 5, 5, 1]), u([10, 20, 1, 7, 9, 1 << 63]), 4,
                        keep_zero=True)
    assert rows == [(b"\1", -5, 7, 3, 30), (b"\2", 0, 0, 1 << 63, 1), (b"\3", 1, 2, 0, M64 - 1),
                    (b"\4", int(I64.max), int(I64.min), M64, 1 << 63)]
    kept = [r for r in rows if r[3] != 0]
    assert signed(1 << 63) == -(1 << 63) and signed(M64) == -1 and signed(5) == 5
    assert movers_truth(kept, 0) == [(b"\2", -(1 << 63)), (b"\1", 3), (b"\4", -1)]
    assert movers_truth(kept, 1) == [(b"\4", -(1 << 63)), (b"\1", 30), (b"\2", 1)]
    assert movers_truth(kept, 0, 1) == [(b"\1", 3)] and movers_truth(kept, 0, -1, 2) == [(b"\2", -(1 << 63))]
    assert movers_truth(kept, 1, 0, 0, 2) == [(b"\4", -(1 << 63)), (b"\1", 30)]
    assert movers_truth(rows, 1) == movers_truth(kept, 1)  # a group whose packets did not change is no flow
    ties = [(b"\2", 0, 0, 5, 0), (b"\1", 0, 0, (-5) & M64, 0), (b"\3", 0, 0, 5, 0)]
    assert movers_truth(ties, 0, 0, 1, 2) == [(b"\1", -5), (b"\2", 5)]  # equal magnitudes: key bytes ascending


def test_rowlog_truth_by_hand():
    log = RowLog(["Protocol"])
    k = lambda *xs: np.array([[x] for x in xs], np.uint8)
    u = lambda xs: np.array(xs, np.uint64)
    log.append(1, k(6, 17), [1, 2], [3, 4], u([5, 5]), u([50, 50]))
    log.append(2, k(17, 1), [2, -9], [8, 9], u([5, 1]), u([70, 1]))
    assert rowlog_sets(log, 1, 2) == ([(1, 0), (1, 1)], [(0, 1)])
    assert rowlog_delta(log, 1, 2, ["Protocol"]) == ([(b"\x01", -9, 9, 1, 1)], 3)  # 17: packets 5 -> 5, no flow
    assert rowlog_delta(log, 1, 2, ["Protocol"], keep_zero=True)[0][1] == (b"\x11", 2, 8, 0, 20)
    assert rowlog_delta(log, None, None, ["Protocol"])[0] == log.rollup(None, ["Protocol"])
    assert rowlog_delta(log, 2, None, ["Protocol"]) == ([], 0) and rowlog_delta(log, 0, 1, ["Protocol"])[1] == 2


# --- the header, the binding, the Python surface ---
def test_header_declares_the_calls_and_lib_binds_them():
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.findall(r"\bint\s+gns_ex_hist_rollup_between\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert len(m) == 1, "gns_ex_hist_rollup_between is not declared exactly once"
    args = [a.strip() for a in m[0].split(",") if a.strip()]
    assert len(args) == 6 and args[0].startswith("gns_ex *") and args[1].startswith("gns_ex_hist *")
    assert "int64_t *start_ns" in args[2] and "int64_t *end_ns" in args[3] and "gns_prefix" in args[4] and "uint64_t" in args[5]
    m = re.findall(r"\bint\s+gns_ex_movers\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert len(m) == 1 and len([a for a in m[0].split(",") if a.strip()]) == 8 and "int64_t *values" in m[0]
    assert "a delta roll-up between two times" not in raw
    from go2netspectra_amd import _lib
    assert {"gns_ex_hist_rollup_between", "gns_ex_movers"} <= set(_lib.EXPORTED)
    L = _lib.load()  # (the library needs no GPU to load; a failure here is a failure)
    fn = L.gns_ex_hist_rollup_between
    assert fn.restype is ct.c_int and fn.argtypes == [ct.c_void_p] * 6
    out = (ct.c_uint64 * 2)(3, 4)
    assert fn(None, None, None, None, None, out) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()
    assert (out[0], out[1]) == (3, 4)
    n = ct.c_uint64(0)
    assert L.gns_ex_movers(None, 0, 0, 1, 0, None, None, ct.byref(n)) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()


def test_python_surface_and_argument_errors_come_first():
    from go2netspectra_amd import Change, ExactAggregator, ExactHistory, ExactTask
    from go2netspectra_amd import signed as lib_signed
    p = inspect.signature(ExactAggregator.rollup_from_history).parameters
    assert list(p)[1:] == ["hist", "end_time", "prefix", "start_time"] and p["start_time"].default is None
    p = inspect.signature(ExactHistory.delta).parameters
    assert [p[k].default for k in ("key_fields", "prefix", "start_time", "end_time")] == [None] * 4
    p = inspect.signature(ExactAggregator.movers).parameters
    assert [p[k].default for k in ("direction", "threshold", "limit")] == [0, 1, 0]
    assert inspect.signature(ExactHistory.aggregate).parameters["start_time"].default is None
    for name in ("rollup", "aggregate_flows", "movers"):
        assert inspect.signature(getattr(ExactTask, name)).parameters["start_time"].default is None, name
    assert Change() == Change(0, 0, 0)
    a = np.array([1, M64, 1 << 63], np.uint64)
    assert lib_signed(a).tolist() == [1, -1, -(1 << 63)] and lib_signed(M64 - 1) == -2 and lib_signed(7) == 7
    # no handle and no library: the checks come before any call
    h = ExactHistory.__new__(ExactHistory)
    h._h, h._L, h.key_fields, h.key_bytes, h.device = None, None, ["SrcIP", "Protocol"], 17, 0
    with pytest.raises(ValueError, match="DstIP"):
        h.delta(["DstIP"])
    with pytest.raises(ValueError, match="start_time"):
        h.delta(start_time=5, end_time=4)
    with pytest.raises(ValueError):
        h.delta(["SrcIP"], prefix={"SrcIP": 33}, start_time=1)
    with pytest.raises(ValueError):
        h.delta(start_time=1 << 63)
    with pytest.raises(ValueError, match="start_time"):
        h.aggregate([{}], start_time=3, end_time=2)
    with pytest.raises(ValueError, match="metric"):
        h.movers(["SrcIP"], 2, start_time=1)
    with pytest.raises(ValueError, match="direction"):
        h.movers(["SrcIP"], 0, direction=2, start_time=1)
    for kw in ({"threshold": -1}, {"limit": -1}, {"threshold": 1 << 64}):
        with pytest.raises(ValueError, match="unsigned"):
            h.movers(["SrcIP"], 0, start_time=1, **kw)
    agg = ExactAggregator.__new__(ExactAggregator)
    agg._h, agg._L, agg.key_fields, agg.key_bytes, agg.device = None, None, ["SrcIP"], 16, 0
    with pytest.raises(ValueError, match="start_time"):
        agg.rollup_from_history(h, end_time=-1, start_time=0)
    other = ExactHistory.__new__(ExactHistory)
    other._h, other._L, other.key_fields, other.key_bytes, other.device = None, None, ["SrcIP"], 16, 1
    with pytest.raises(ValueError, match="device"):
        agg.rollup_from_history(other, start_time=0)
    for bad in (lambda: agg.movers(2), lambda: agg.movers(0, direction=-2), lambda: agg.movers(0, threshold=-1),
                lambda: agg.movers(0, limit=-1)):
        with pytest.raises(ValueError):
            bad()
    task = ExactTask.__new__(ExactTask)
    task.name_, task.key_fields, task.agg = "t", ["SrcIP"], agg
    for call in (lambda: task.rollup("r", ["SrcIP"], start_time=5), lambda: task.aggregate_flows(start_time=5),
                 lambda: task.movers(0, 5, start_time=5)):
        with pytest.raises(ValueError, match="history"):
            call()
    task.history = h
    with pytest.raises(ValueError, match="start_time"):
        task.movers(0, 5, start_time=5, end_time=4)
    with pytest.raises(ValueError, match="start_time"):
        task.aggregate_flows(start_time=5, end_time=4)
