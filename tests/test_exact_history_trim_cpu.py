"""Trim, export and restore of the exact history without a GPU: the trimmed truth of
history_trim_truth.py against hand-written rows; HistPlan::trim_plan / trimmed in a stand-alone
program built with ASan + UBSan; the header and the ctypes binding of the three new calls; the
file part of an ExactHistory checkpoint; the Python argument errors that come before any device
call."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from go2netspectra_amd import ExactHistory, ExactTask, Manager, Summary, _lib, checkpoint
from history_truth import HistoryTruth
from history_trim_truth import counts, delta_truth, expired, trimmed_truth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "go2netspectra_amd", "csrc")
HEADER = os.path.join(HERE, "..", "include", "gns_sketch.h")

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "gns_histplan.hpp"

// commands, one per line:  a <t> <n>  publish a snapshot of n rows    r  a fresh plan
//   p <before> <fold>  trim_plan: prints c R d noop
//   t <before> <fold> <nbase>  trim_plan + trimmed(nbase) unless a noop: prints the new plan as
//                              S rows, then S lines "s <ts> <end_rows>"; the plan is replaced
int main() {
    gns::HistPlan p;
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        long long a = 0;
        unsigned long long u = 0;
        int fold = 0;
        switch (cmd) {
        case 'a':
            if (std::scanf("%lld %llu", &a, &u) != 2) return 2;
            if (p.append_check((int64_t)a, u) != gns::HIST_OK) return 4;
            p.publish((int64_t)a, u);
            break;
        case 'p': {
            if (std::scanf("%lld %d", &a, &fold) != 2) return 2;
            const gns::HistPlan::Trim t = p.trim_plan((int64_t)a, fold != 0);
            std::printf("p %llu %llu %u %d\n", (unsigned long long)t.c, (unsigned long long)t.R, t.d, t.noop ? 1 : 0);
            break;
        }
        case 't': {
            if (std::scanf("%lld %d %llu", &a, &fold, &u) != 3) return 2;
            const gns::HistPlan::Trim t = p.trim_plan((int64_t)a, fold != 0);
            if (!t.noop) p = p.trimmed(t, u);
            std::printf("t %zu %llu\n", p.ts.size(), (unsigned long long)p.rows);
            for (size_t i = 0; i < p.ts.size(); i++)
                std::printf("s %lld %llu\n", (long long)p.ts[i], (unsigned long long)p.end_rows[i]);
            break;
        }
        case 'r': p = gns::HistPlan(); break;
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
    tmp = tmp_path_factory.mktemp("histtrim")
    src, exe = tmp / "histtrim_driver.cpp", str(tmp / "histtrim_driver")
    src.write_text(DRIVER)
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-3000:]
        return [[int(x) if re.fullmatch(r"-?\d+", x) else x for x in ln.split()] for ln in r.stdout.splitlines()]
    return run


# --- trim_plan / trimmed ---
TSX = [-(1 << 62), -5, -4, 0, 7, 1 << 40]
ROWSX = [3, 0, 10, 0, 0, 257]  # snapshots without rows among them


def model_plan(ts, rows, before, fold):
    """(c, R, d, noop) as DESIGN section 4c defines them: c snapshots lie before ``before``, R rows in them."""
    c = sum(1 for t in ts if t < before)
    R = sum(rows[:c])
    d = c - 1 if fold and c else c
    return c, R, d, int(c == 0 or (fold and c == 1))


def model_trimmed(ts, rows, before, fold, nbase):
    c, R, d, noop = model_plan(ts, rows, before, fold)
    if noop:
        return list(ts), list(rows)
    if fold:
        return [ts[c - 1]] + ts[c:], [nbase] + rows[c:]
    return ts[c:], rows[c:]


def test_trim_plan_at_every_boundary(driver):
    befores = sorted({t + d for t in TSX for d in (-1, 0, 1)} | {-(1 << 63), (1 << 63) - 1})
    lines = ["p 0 0", "p 0 1", "p -9223372036854775808 1", "t 5 1 0", "t 5 0 0"]  # an empty plan: nothing expires
    lines += [f"a {t} {n}" for t, n in zip(TSX, ROWSX)]
    lines += [f"p {b} {f}" for b in befores for f in (0, 1)]
    out = driver(lines)
    assert out[:5] == [["p", 0, 0, 0, 1]] * 3 + [["t", 0, 0]] * 2
    k = 5
    seen_c = set()
    for b in befores:
        for f in (0, 1):
            c, R, d, noop = model_plan(TSX, ROWSX, b, f)
            assert out[k] == ["p", c, R, d, noop], (b, f)
            seen_c.add(c)
            k += 1
    assert seen_c == set(range(len(TSX) + 1))  # below the first ... above the last
    assert k == len(out)


def test_trimmed_plans(driver):
    befores = sorted({t + d for t in TSX for d in (-1, 0, 1)} | {-(1 << 63), (1 << 63) - 1})
    for fold in (0, 1):
        for b in befores:
            for nbase in ((0,) if not fold else (0, 1, 9)):
                c, R, _, noop = model_plan(TSX, ROWSX, b, fold)
                if fold and nbase > R:
                    continue
                out = driver([f"a {t} {n}" for t, n in zip(TSX, ROWSX)] + [f"t {b} {fold} {nbase}"])
                ts, rows = model_trimmed(TSX, ROWSX, b, fold, nbase)
                ends = [sum(rows[:i + 1]) for i in range(len(rows))]
                assert out[0] == ["t", len(ts), sum(rows)], (b, fold, nbase)
                assert out[1:] == [["s", t, e] for t, e in zip(ts, ends)], (b, fold, nbase)
                if fold and c == 1:  # the base is snapshot 0 itself: a no-op
                    assert noop and ts == TSX
    # a chain: fold, append two more, drop everything, start anew at an earlier time
    out = driver([f"a {t} {n}" for t, n in zip(TSX, ROWSX)] +
                 ["t 0 1 7", f"a {(1 << 40) + 1} 5", f"a {(1 << 40) + 2} 0", "t 8 0 0", f"t {(1 << 62)} 0 0", "a -100 2", "t 0 1 1"])
    blocks, cur = [], None
    for o in out:
        if o[0] == "t":
            cur = [o]
            blocks.append(cur)
        else:
            cur.append(o)
    assert blocks[0] == [["t", 4, 264], ["s", -4, 7], ["s", 0, 7], ["s", 7, 7], ["s", 1 << 40, 264]]
    assert blocks[1] == [["t", 3, 262], ["s", 1 << 40, 257], ["s", (1 << 40) + 1, 262], ["s", (1 << 40) + 2, 262]]
    assert blocks[2] == [["t", 0, 0]]
    assert blocks[3] == [["t", 1, 2], ["s", -100, 2]]  # fold with c == 1: untouched


# --- the trimmed truth against hand-written rows ---
def hand_truth():
    tr = HistoryTruth(["SrcIP", "DstPort"])
    # a appears in every snapshot; b ONLY in the expired ones; c comes back SMALLER at 30 (a reset
    # in between); d appears at 20; snapshot 25 has no rows
    tr.record(10, {"10.1.2.3-80": (100, 200, 5, 500), "10.1.9.9-80": (50, 60, 2, 20), "10.2.0.1-443": (-7, 300, 9, 90)})
    tr.record(20, {"10.1.2.3-80": (100, 250, 8, 800), "2001:db8::1-53": (1, 2, 1, 7)})
    tr.record(30, {"10.1.2.3-80": (400, 450, 1, 10), "10.2.0.1-443": (500, 600, 3, 30)})
    return tr, [10, 20, 25, 30]


def test_trimmed_truth_on_hand_written_rows():
    S = Summary
    tr, times = hand_truth()
    assert [expired(times, b) for b in (9, 10, 11, 20, 21, 25, 26, 30, 31)] == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    same, t0 = trimmed_truth(tr, times, 10, True)
    assert t0 == times and same.ts == tr.ts and same.key == tr.key
    # drop the first two snapshots: b is forgotten, c's old larger row is gone
    d, td = trimmed_truth(tr, times, 21, False)
    assert td == [25, 30] and counts(d) == (2, 2)
    assert d.summary({}, 29) == S() and d.summary({}, None) == S(2, 4, 40, 400, 600, 3, 30)
    assert d.summary({"SrcIP": "10.1.9.9"}, None) == S()
    assert d.summary({"SrcIP": "10.2.0.1"}, None) == S(1, 3, 30, 500, 600, 3, 30)
    # fold them: the base holds the four rows live at 20 under time 20; b stays, a's first row goes
    f, tf = trimmed_truth(tr, times, 21, True)
    assert tf == [20, 25, 30] and counts(f) == (6, 4) and f.ts == [20, 20, 20, 20, 30, 30]
    assert f.key[:4] == ["10.1.9.9-80", "10.2.0.1-443", "10.1.2.3-80", "2001:db8::1-53"]  # stored order kept
    assert f.summary({}, 19) == S()
    for T in (20, 25, 29, 30, None):  # the present is unchanged
        a, b = f.summary({}, T), tr.summary({}, T)
        assert (a.flows, a.packets, a.bytes) == (b.flows, b.packets, b.bytes), T
        assert f.export_at(T) == tr.export_at(T) and f.heavy(1, 0, 0, T) == tr.heavy(1, 0, 0, T)
    # TraceFlow of c still sees its larger row of snapshot 10 (it was live at 20)
    assert f.summary({"SrcIP": "10.2.0.1"}, None) == tr.summary({"SrcIP": "10.2.0.1"}, None) == S(1, 3, 30, -7, 600, 9, 90)
    # fold past the reset: c's larger row is folded away, so TraceFlow's max changes
    g, tg = trimmed_truth(tr, times, 31, True)
    assert tg == [30] and counts(g) == (4, 4) and set(g.ts) == {30}
    assert g.summary({"SrcIP": "10.2.0.1"}, None) == S(1, 3, 30, 500, 600, 3, 30)
    assert tr.summary({"SrcIP": "10.2.0.1"}, None).max_packets == 9
    assert g.export_at(None) == tr.export_at(None) and g.export_at(29) == {}
    # past the last under drop: empty
    e, te = trimmed_truth(tr, times, 31, False)
    assert te == [] and counts(e) == (0, 0)
    # a chain of trims equals one trim
    h1, th1 = trimmed_truth(*trimmed_truth(tr, times, 11, True), 26, True)
    h2, th2 = trimmed_truth(tr, times, 26, True)
    assert th1 == th2 == [25, 30] and h1.rows_at(None) == h2.rows_at(None) and h1.ts == h2.ts and h1.key == h2.key


def test_delta_truth_keeps_the_touched_rows():
    tr = HistoryTruth(["SrcIP"])
    tr.record(1, {"10.0.0.1": (1, 2, 3, 4), "10.0.0.2": (5, 6, 7, 8)})
    tr.record(2, {"10.0.0.1": (1, 2, 3, 4), "10.0.0.2": (5, 9, 8, 9)})   # .1 untouched
    tr.record(3, {"10.0.0.1": (1, 2, 3, 4)})                               # after a reset: stored although equal
    tr.record(4, {"10.0.0.1": (1, 2, 3, 4), "10.0.0.3": (1, 1, 1, 1)})
    d = delta_truth(tr, [1, 2, 3, 4], reset_after=2)
    assert list(zip(d.ts, d.key)) == [(1, "10.0.0.1"), (1, "10.0.0.2"), (2, "10.0.0.2"), (3, "10.0.0.1"), (4, "10.0.0.3")]
    for T in (0, 1, 2, 3, 4, None):
        assert d.summary({}, T) == tr.summary({}, T) and d.rows_at(T) == tr.rows_at(T)


# --- the header and the binding ---
THREE = ["gns_ex_hist_trim", "gns_ex_hist_export", "gns_ex_hist_append_rows"]


def test_header_declares_the_three_calls_and_lib_binds_them():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = _lib.load()
    for name, want in zip(THREE, (4, 8, 9)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, f"{name} is not declared"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert nargs == want and name in _lib.EXPORTED
        assert len(getattr(L, name).argtypes) == nargs, name
    assert ExactHistory.STATS[7] == "rows_trimmed" and len(ExactHistory.STATS) == 8


# --- the file part of a history checkpoint ---
def test_history_file_round_trip(tmp_path):
    assert checkpoint.PARAMS["ExactHistory"] == ["key_fields", "key_bytes"]
    assert checkpoint.ARRAYS["ExactHistory"] == ["keys", "start", "end", "pkts", "bytes", "written", "times"]
    hist = ExactHistory.__new__(ExactHistory)  # no handle: describe reads the layout only
    hist._h, hist.key_fields, hist.key_bytes = None, ["Protocol", "SrcIP"], 17
    meta = checkpoint.describe(hist)
    assert meta == {"format": 1, "class": "ExactHistory", "key_fields": ["Protocol", "SrcIP"], "key_bytes": 17}
    rng = np.random.default_rng(3)
    n = 9
    arrays = {"keys": rng.integers(0, 256, (n, 17)).astype(np.uint8), "start": rng.integers(-50, 50, n).astype(np.int64),
              "end": rng.integers(-50, 50, n).astype(np.int64), "pkts": rng.integers(1, 9, n).astype(np.uint64),
              "bytes": np.full(n, (1 << 64) - 1, np.uint64), "written": np.array([0, 0, 0, 2, 2, 3, 3, 3, 3], np.uint32),
              "times": np.array([-(1 << 63), -1, 0, 5, (1 << 63) - 1], np.int64)}
    path = str(tmp_path / "h.history.npz")
    checkpoint.write(path, meta, arrays)
    meta2, got = checkpoint.read(path)
    checkpoint.check_meta(meta2, meta)
    assert set(got) == set(arrays)
    for k, v in arrays.items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k
    # rows of one snapshot are contiguous; snapshots 1 and 4 have none
    assert checkpoint.history_slices(got["written"], 5) == [(0, 3), (3, 3), (3, 5), (5, 9), (9, 9)]
    assert checkpoint.history_slices(np.zeros(0, np.uint32), 2) == [(0, 0), (0, 0)]
    for bad in ([0, 2, 1], [0, 5]):
        with pytest.raises(ValueError, match="written"):
            checkpoint.history_slices(np.array(bad, np.uint32), 5)
    other = dict(meta, key_fields=["SrcIP"], key_bytes=16)
    with pytest.raises(ValueError, match="'key_fields' differs"):
        checkpoint.check_meta(meta2, other)
    with pytest.raises(ValueError, match="'class' differs"):
        checkpoint.check_meta(meta2, dict(meta, **{"class": "ExactAggregator"}))


# --- Python argument errors, before any device call ---
def test_trim_and_retain_argument_checks():
    hist = ExactHistory.__new__(ExactHistory)  # no handle: the checks below come first
    hist._h, hist._L, hist.key_bytes = None, None, 16
    for bad in (1 << 63, -(1 << 63) - 1):
        with pytest.raises(ValueError, match="before .* int64"):
            hist.trim(bad)
    with pytest.raises(ValueError, match=r"keys must be \[n, 16\]"):
        hist.append_rows(np.zeros((2, 4), np.uint8), [1, 1], [2, 2], [1, 1], [1, 1], 5)
    with pytest.raises(ValueError, match="differ in length"):
        hist.append_rows(np.zeros((2, 16), np.uint8), [1, 1], [2, 2], [1], [1, 1], 5)
    with pytest.raises(ValueError, match="timestamp_ns .* int64"):
        hist.append_rows(np.zeros((0, 16), np.uint8), [], [], [], [], 1 << 63)
    task = ExactTask.__new__(ExactTask)
    task.name_, task.key_fields, task.agg = "t", ["SrcIP"], None
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="retain"):
            task.keep_history(retain=bad)
    assert getattr(task, "history", None) is None
    for call in (task.save_history, task.restore_history):
        with pytest.raises(ValueError, match="keep_history"):
            call("nowhere.npz")
    mgr = Manager.__new__(Manager)

    class Group:
        Tasks = [task]
    mgr.groups = [Group()]
    with pytest.raises(ValueError, match="retain"):
        mgr.keep_history(retain=0)
