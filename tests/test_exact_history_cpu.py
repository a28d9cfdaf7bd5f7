"""The exact history without a GPU: gns_histplan.hpp (the timestamp table, s(T), the append
checks, the capacity arithmetic) in a stand-alone program built with ASan + UBSan; the truth
model of history_truth.py against hand-written rows; the header and the ctypes binding of the
nine gns_ex_hist_* calls; the Python argument errors that come before any device call."""
import bisect
import os
import re
import shutil
import subprocess

import pytest

from go2netspectra_amd import ExactHistory, ExactTask, Manager, Summary, _lib
from history_truth import HistoryTruth, parse_prefix

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "go2netspectra_amd", "csrc")
HEADER = os.path.join(HERE, "..", "include", "gns_sketch.h")

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "gns_histplan.hpp"

// commands, one per line:  a <t> <n>  append_check + publish    q <T>  s(T), rows as of it
//   n  s(NULL)   c <cap> <need>  hist_row_capacity   i <flows>  hist_index_slots   r  a fresh plan
//   f <rows>  pretend the log holds that many rows (the 2^32 - 2 limit without 2^32 appends)
int main() {
    gns::HistPlan p;
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        long long a = 0;
        unsigned long long u = 0, w = 0;
        switch (cmd) {
        case 'a': {
            if (std::scanf("%lld %llu", &a, &u) != 2) return 2;
            const int rc = p.append_check((int64_t)a, u);
            if (rc == gns::HIST_OK) p.publish((int64_t)a, u);
            std::printf("a %d %zu %llu\n", rc, p.ts.size(), (unsigned long long)p.rows);
            break;
        }
        case 'q': {
            if (std::scanf("%lld", &a) != 1) return 2;
            const int64_t t = (int64_t)a, s = p.as_of(&t);
            std::printf("q %lld %llu\n", (long long)s, (unsigned long long)p.rows_as_of(s));
            break;
        }
        case 'n': std::printf("n %lld %llu\n", (long long)p.as_of(nullptr), (unsigned long long)p.rows_as_of(p.as_of(nullptr))); break;
        case 'c':
            if (std::scanf("%llu %llu", &u, &w) != 2) return 2;
            std::printf("c %llu\n", (unsigned long long)gns::hist_row_capacity(u, w));
            break;
        case 'i':
            if (std::scanf("%llu", &u) != 1) return 2;
            std::printf("i %llu\n", (unsigned long long)gns::hist_index_slots(u));
            break;
        case 'f':
            if (std::scanf("%llu", &u) != 1) return 2;
            p.rows = u;
            break;
        case 'r': p = gns::HistPlan(); break;
        default: return 3;
        }
    }
    return 0;
}
"""

MAXROWS = (1 << 32) - 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("histplan")
    src, exe = tmp / "histplan_driver.cpp", str(tmp / "histplan_driver")
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


def test_header_includes_no_hip():
    txt = open(os.path.join(CSRC, "gns_histplan.hpp")).read()
    assert "#include <hip" not in txt and "__device__" not in txt and "__global__" not in txt


def test_as_of_is_the_newest_snapshot_at_or_before_t(driver):
    ts = [-(1 << 62), -5, -4, 0, 7, 1 << 40, (1 << 63) - 1]
    rows = [3, 0, 10, 1, 0, 257, 64]
    probes = sorted({t + d for t in ts for d in (-1, 0, 1) if -(1 << 63) <= t + d < (1 << 63)} | {-(1 << 63), 100})
    lines = ["n", "q 0", "q -9223372036854775808"]  # an empty table: no snapshot at any time
    lines += [f"a {t} {n}" for t, n in zip(ts, rows)] + ["n"] + [f"q {T}" for T in probes]
    out = driver(lines)
    assert out[:3] == [["n", -1, 0], ["q", -1, 0], ["q", -1, 0]]
    ends = [sum(rows[:i + 1]) for i in range(len(rows))]
    for i, o in enumerate(out[3:3 + len(ts)]):
        assert o == ["a", 0, i + 1, ends[i]]
    assert out[3 + len(ts)] == ["n", len(ts) - 1, ends[-1]]
    for T, o in zip(probes, out[4 + len(ts):]):
        s = bisect.bisect_right(ts, T) - 1  # below the first: -1; at, between, above: the one at or before
        assert o == ["q", s, ends[s] if s >= 0 else 0], T
    assert len(out) == 4 + len(ts) + len(probes)


def test_non_increasing_timestamps_and_full_logs_are_rejected(driver):
    out = driver(["a -10 5", "a -10 1", "a -11 1", "a -9223372036854775808 1", "a -9 2",
                  "r", "a -9223372036854775808 0", "a -9223372036854775808 0", "a -9223372036854775807 1",
                  "r", f"f {MAXROWS - 2}", "a 1 3", "a 1 2", "a 2 1", "a 2 0"])
    assert out == [["a", 0, 1, 5], ["a", 1, 1, 5], ["a", 1, 1, 5], ["a", 1, 1, 5], ["a", 0, 2, 7],
                   ["a", 0, 1, 0], ["a", 1, 1, 0], ["a", 0, 2, 1],  # the smallest int64 is a legal first timestamp
                   ["a", 3, 0, MAXROWS - 2], ["a", 0, 1, MAXROWS], ["a", 3, 1, MAXROWS], ["a", 0, 2, MAXROWS]]


def test_capacities_double_until_they_fit(driver):
    cases = [(0, 0), (0, 1), (0, 5), (256, 256), (256, 257), (256, 513), (256, 1 << 20), (1, MAXROWS),
             ((1 << 31), (1 << 31) + 1), (MAXROWS, MAXROWS), (3, 4), (3, 7)]
    flows = [0, 1, 31, 32, 33, 64, 1000, 1 << 20, (1 << 20) + 1]
    out = driver([f"c {c} {n}" for c, n in cases] + [f"i {f}" for f in flows])
    for (cap, need), o in zip(cases, out):
        want = cap
        if need > cap:
            want = max(cap, 1)
            while want < need:
                want = MAXROWS if want > MAXROWS // 2 else want * 2
        assert o == ["c", want], (cap, need)
        assert want >= need and want <= MAXROWS
    for f, o in zip(flows, out[len(cases):]):
        want = 64
        while want < 2 * f:
            want *= 2
        assert o == ["i", want], f


# --- the truth model against hand-written rows ---
def test_truth_model_on_hand_written_rows():
    tr = HistoryTruth(["SrcIP", "DstPort"])
    # a appears in every snapshot; b only in the first; c comes back SMALLER at 30 (a reset in
    # between); d is IPv6 and appears at 20
    tr.record(10, {"10.1.2.3-80": (100, 200, 5, 500), "10.1.9.9-80": (50, 60, 2, 20), "10.2.0.1-443": (-7, 300, 9, 90)})
    tr.record(20, {"10.1.2.3-80": (100, 250, 8, 800), "2001:db8::1-53": (1, 2, 1, (1 << 64) - 1)})
    tr.record(30, {"10.1.2.3-80": (400, 450, 1, 10), "10.2.0.1-443": (500, 600, 3, 30)})
    S = Summary
    assert tr.summary({}, 9) == S() and tr.export_at(9) == {} and tr.heavy(0, 0, 0, 9) == []
    assert tr.summary({}, 10) == S(3, 16, 610, -7, 300, 9, 500)
    assert tr.summary({}, 19) == tr.summary({}, 10)
    # at 20: a's newer row replaces its older one in the sums; the byte sum wraps mod 2^64
    assert tr.summary({}, 20) == S(4, 2 + 9 + 8 + 1, (20 + 90 + 800 + (1 << 64) - 1) % (1 << 64), -7, 300, 9, (1 << 64) - 1)
    # at 30 and None: a and c are live with their NEWER, SMALLER rows; min / max still see the older ones
    for T in (30, 31, None):
        assert tr.summary({}, T) == S(4, 1 + 2 + 3 + 1, (10 + 20 + 30 + (1 << 64) - 1) % (1 << 64), -7, 600, 9, (1 << 64) - 1)
        assert tr.summary({"SrcIP": "10.2.0.1"}, T) == S(1, 3, 30, -7, 600, 9, 90)  # TraceFlow: max_packets 9 > the live 3
        assert tr.summary({"SrcIP": "10.1.0.0/16"}, T) == S(2, 3, 30, 50, 450, 8, 800)
        assert tr.export_at(T)["10.1.2.3-80"] == (400, 450, 1, 10)
    assert tr.summary({"SrcIP": "10.1.2.3", "DstPort": 80}, 25) == S(1, 8, 800, 100, 250, 8, 800)
    assert tr.summary({"SrcIP": "10.0.0.0/8"}, 10).flows == 3 and tr.summary({"SrcIP": "0.0.0.0/0"}, 20).flows == 3
    assert tr.summary({"SrcIP": "::/0"}, 20).flows == 4 and tr.summary({"SrcIP": "2001:db8::/120"}, 20).flows == 1
    assert tr.summary({"SrcIP": "2001:db8::100/120"}, None) == S()
    assert tr.summary({"Protocol": 6}, None) == S()  # not a column of this layout
    assert tr.summary({"DstPort": 81}, None) == S()
    kb = lambda ip, port: (bytes(10) + b"\xff\xff" + bytes(ip)) + port.to_bytes(2, "big")
    assert tr.heavy(0, 0, 0, 10) == [(kb([10, 2, 0, 1], 443), 9), (kb([10, 1, 2, 3], 80), 5), (kb([10, 1, 9, 9], 80), 2)]
    assert tr.heavy(0, 3, 1, 20) == [(kb([10, 2, 0, 1], 443), 9)]
    assert [v for _, v in tr.heavy(0, 0, 0, None)] == [3, 2, 1, 1]
    assert tr.heavy(0, 0, 0, None)[2][0] < tr.heavy(0, 0, 0, None)[3][0]  # a tie: key bytes ascending
    assert len(tr.rows_at(20)) == 4 and (kb([10, 1, 2, 3], 80), 100, 250, 8, 800) in tr.rows_at(20)
    assert parse_prefix("10.1.0.0/16") == (bytes(10) + b"\xff\xff" + bytes([10, 1, 0, 0]), 112)
    assert parse_prefix("2001:db8::/32")[1] == 32


# --- the header and the binding ---
NINE = ["gns_ex_hist_create", "gns_ex_hist_destroy", "gns_ex_hist_append", "gns_ex_hist_times", "gns_ex_hist_stats",
        "gns_ex_hist_aggregate", "gns_ex_hist_aggregate_cidr", "gns_ex_hist_heavy_hitters", "gns_ex_hist_snapshot"]


def test_header_declares_the_nine_calls_and_lib_binds_them():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = _lib.load()
    for name in NINE:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, f"{name} is not declared"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.EXPORTED
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs, (name, nargs, fn.argtypes)
    assert re.search(r"typedef struct gns_ex_hist_params\s*\{\s*gns_layout key;\s*uint64_t max_rows, max_flows;\s*int device;\s*\}", txt)
    import ctypes as ct
    assert ct.sizeof(_lib.ExHistParams) == ct.sizeof(_lib.Layout) + 4 + 8 + 8 + 8  # (layout padded to 8, int padded)


# --- Python argument errors, before any device call ---
def bare_task():
    task = ExactTask.__new__(ExactTask)
    task.name_, task.key_fields, task.agg = "t", ["SrcIP"], None
    return task


def test_end_time_without_a_history_still_raises():
    task = bare_task()
    task.history = None
    for call in (lambda: task.trace_flow({"SrcIP": "1.2.3.4"}, end_time=5),
                 lambda: task.aggregate_flows(src_ip="1.2.3.4", end_time=5),
                 lambda: task.aggregate_flows_many([dict(protocol=6), dict(protocol=17, end_time=5)]),
                 lambda: task.heavy_hitters(0, 10, end_time=0)):
        with pytest.raises(ValueError, match="end_time is not supported"):
            call()


def test_record_without_keep_history_raises():
    task = bare_task()
    with pytest.raises(ValueError, match="keep_history"):
        task.record(1)
    task.history = None
    with pytest.raises(ValueError, match="keep_history"):
        task.record(1, full=True)
    mgr = Manager.__new__(Manager)

    class Group:
        Tasks = [task]
    mgr.groups = [Group()]
    with pytest.raises(ValueError, match="record: task t has no history"):
        mgr.record(5)


def test_history_argument_checks():
    hist = ExactHistory.__new__(ExactHistory)  # no handle: the checks below come first
    hist._h, hist._L, hist.key_bytes = None, None, 16
    with pytest.raises(ValueError, match="metric 2"):
        hist.heavy_hitters(2)
    with pytest.raises(ValueError, match="unsigned"):
        hist.heavy_hitters(0, limit=-1)
    with pytest.raises(ValueError, match="unsigned"):
        hist.heavy_hitters(1, threshold=-1)
    with pytest.raises(ValueError, match="end_time .* int64"):
        hist.heavy_hitters(0, end_time=1 << 63)
    with pytest.raises(ValueError, match="end_time .* int64"):
        hist.aggregate([{}], end_time=-(1 << 63) - 1)
    with pytest.raises(TypeError, match="ExactView"):
        hist.append(object(), 5)
    with pytest.raises(ValueError, match="unsigned"):
        ExactHistory(["SrcIP"], max_rows=-1)
    task = bare_task()

    class Hist:  # a history stands in: the limit check still comes before it is asked
        def heavy_hitters(self, *a, **k):
            raise AssertionError("not reached")
    task.history = Hist()
    with pytest.raises(ValueError, match="negative limit"):
        task.heavy_hitters(0, -1, end_time=5)
    assert task.heavy_hitters(0, 0, end_time=5) == [] and task.heavy_hitters(7, 3, end_time=5) == []
