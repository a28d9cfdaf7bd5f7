"""The heavy-hitter history without a GPU: the truth model of heavy_history_truth.py against a
hand-written table; gns_hhplan.hpp (per-lane row counts under shared timestamps) in a
stand-alone program built with ASan + UBSan; the header and the ctypes binding of the
gns_hh_hist_* calls; the Python argument errors that come before any device call; a Manager
without heavy histories behaves as before."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from go2netspectra_amd import HeavyHistory, Manager, SketchTask, _lib
from go2netspectra_amd.heavy_history import pack_rows
from heavy_history_truth import HeavyTruth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "go2netspectra_amd", "csrc")
HEADER = os.path.join(HERE, "..", "include", "gns_sketch.h")
MAXROWS = (1 << 32) - 2


# --- the truth model against a hand-written table ---
def key(port_a, port_b):  # SrcPort, DstPort
    return port_a.to_bytes(2, "big") + port_b.to_bytes(2, "big")


def test_truth_model_on_hand_written_rows():
    tr = HeavyTruth(["SrcPort", "DstPort"])
    a, b, c, d, e = key(1, 80), key(2, 80), key(3, 443), key(4, 53), key(0, 9)
    # 12 rows.  a is listed every time; b only at 10 (no tombstone: it stays); c comes back SMALLER
    # at 30 (a reset in between); d and e tie with c's new value at 30; type 1 is its own table
    tr.record(10, {0: [(a, 100), (b, 70), (c, 90)], 1: [(a, 5000)]})
    tr.record(20, {0: [(a, 150), (d, 40)], 1: [(b, 7), (d, 0)]})
    tr.record(30, {0: [(a, 20), (c, 40), (e, 40)], 1: [(a, 1)]})
    assert len(tr.rows) == 12 and tr.times == [10, 20, 30]
    assert tr.query(0, end_time=9) == [] and tr.query(1, end_time=9) == [] and tr.query(2) == []
    assert tr.query(0, end_time=10) == [("1 80", 100), ("3 443", 90), ("2 80", 70)]
    assert tr.query(0, end_time=19) == tr.query(0, end_time=10)
    # at 20: b and c are missing from the list and stay with their last listed values
    assert tr.query(0, end_time=20) == [("1 80", 150), ("3 443", 90), ("2 80", 70), ("4 53", 40)]
    # at 30 / None: a and c are superseded by SMALLER values; e, c, d tie at 40 in key-byte order
    for T in (30, 31, None):
        assert tr.query(0, end_time=T) == [("2 80", 70), ("0 9", 40), ("3 443", 40), ("4 53", 40), ("1 80", 20)]
        # a limit inside the run of 40s cuts it in key-byte order
        assert tr.query(0, limit=2, end_time=T) == [("2 80", 70), ("0 9", 40)]
        assert tr.query(0, limit=3, end_time=T) == [("2 80", 70), ("0 9", 40), ("3 443", 40)]
        assert tr.query(0, threshold=40, end_time=T) == tr.query(0, limit=4, end_time=T)
        # type independence: type 1 never saw c and e, its rows of a and d are its own; value 0 is a legal row
        assert tr.query(1, end_time=T) == [("2 80", 7), ("1 80", 1), ("4 53", 0)]
        assert tr.query(1, threshold=1, end_time=T) == [("2 80", 7), ("1 80", 1)]
    assert tr.query(1, end_time=20) == [("1 80", 5000), ("2 80", 7), ("4 53", 0)]
    assert tr.query_bytes(0, limit=1) == [(b, 70)]
    assert tr.probe_times() == [9, 10, 15, 20, 25, 30, None]


# --- gns_hhplan.hpp in a host-only program under ASan + UBSan ---
DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "gns_hhplan.hpp"

// commands, one per line:
//   a <t> <k> (<type> <n>){k}  append_check; when it passes: add_lane of every type with rows, publish
//   q <type> <T>  s(T), the lane's rows as of it     n <type>  the same for NULL
//   f <type> <rows>  pretend the lane holds that many rows     l  lanes, snapshots, total rows
int main() {
    gns::HhHistPlan p;
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        long long a = 0;
        unsigned long long u = 0, w = 0;
        switch (cmd) {
        case 'a': {
            unsigned k = 0;
            if (std::scanf("%lld %u", &a, &k) != 2 || k > 300) return 2;
            uint32_t types[300];
            uint64_t ns[300];
            for (unsigned i = 0; i < k; i++) {
                if (std::scanf("%llu %llu", &u, &w) != 2) return 2;
                types[i] = (uint32_t)u;
                ns[i] = w;
            }
            const int rc = p.append_check((int64_t)a, types, ns, k);
            if (rc == gns::HIST_OK) {
                uint32_t pt[300];
                uint64_t pn[300];
                unsigned np = 0;
                for (unsigned i = 0; i < k; i++)
                    if (ns[i]) { p.add_lane(types[i]); pt[np] = types[i]; pn[np] = ns[i]; np++; }
                p.publish((int64_t)a, pt, pn, np);
            }
            std::printf("a %d %zu %llu\n", rc, p.t.ts.size(), (unsigned long long)p.t.rows);
            break;
        }
        case 'q': {
            if (std::scanf("%llu %lld", &u, &a) != 2) return 2;
            const int64_t t = (int64_t)a, s = p.t.as_of(&t);
            std::printf("q %lld %llu\n", (long long)s, (unsigned long long)p.rows_as_of(p.lane((uint32_t)u), s));
            break;
        }
        case 'n': {
            if (std::scanf("%llu", &u) != 1) return 2;
            const int64_t s = p.t.as_of(nullptr);
            std::printf("n %lld %llu\n", (long long)s, (unsigned long long)p.rows_as_of(p.lane((uint32_t)u), s));
            break;
        }
        case 'f':
            if (std::scanf("%llu %llu", &u, &w) != 2) return 2;
            p.lanes[(size_t)p.add_lane((uint32_t)u)].rows = w;
            break;
        case 'l': std::printf("l %zu %zu %llu\n", p.lanes.size(), p.t.ts.size(), (unsigned long long)p.t.rows); break;
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
    tmp = tmp_path_factory.mktemp("hhplan")
    src, exe = tmp / "hhplan_driver.cpp", str(tmp / "hhplan_driver")
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


def test_plan_header_includes_no_hip():
    txt = open(os.path.join(CSRC, "gns_hhplan.hpp")).read()
    assert "#include <hip" not in txt and "__device__" not in txt and "__global__" not in txt


def test_lanes_share_the_timestamps_and_count_their_own_rows(driver):
    # type 0 from the start; type 2 joins at the third snapshot (no rows before); the second snapshot is empty;
    # type 255 appears once; type 7 is named without rows and gets no lane
    out = driver(["n 0", "q 0 5",
                  "a -10 1 0 3", "a -5 0", "a 0 2 0 4 2 6", "a 7 3 255 1 2 1 7 0", "l",
                  "q 0 -11", "q 0 -10", "q 0 -6", "q 0 -5", "q 0 0", "q 0 6", "q 0 7", "n 0",
                  "q 2 -10", "q 2 -1", "q 2 0", "q 2 7", "n 2",
                  "q 255 0", "q 255 7", "q 255 100", "q 7 100", "q 9 100", "n 300"])
    assert out == [["n", -1, 0], ["q", -1, 0],
                   ["a", 0, 1, 3], ["a", 0, 2, 3], ["a", 0, 3, 13], ["a", 0, 4, 15], ["l", 3, 4, 15],
                   ["q", -1, 0], ["q", 0, 3], ["q", 0, 3], ["q", 1, 3], ["q", 2, 7], ["q", 2, 7], ["q", 3, 7], ["n", 3, 7],
                   ["q", 0, 0], ["q", 1, 0], ["q", 2, 6], ["q", 3, 7], ["n", 3, 7],
                   ["q", 2, 0], ["q", 3, 1], ["q", 3, 1], ["q", 3, 0], ["q", 3, 0], ["n", 3, 0]]


def test_plan_rejections_change_nothing(driver):
    out = driver(["a 5 1 0 2",
                  "a 5 1 0 1", "a 4 1 1 1",              # timestamp not after the last: 1
                  "a 6 2 3 1 3 1",                        # a type twice: 5
                  "a 6 1 256 1", "a 6 1 4294967295 0",    # a type outside 0..255: 4
                  "l", f"f 1 {MAXROWS - 1}",
                  "a 6 2 0 1 1 2",                        # lane 1 would pass 2^32 - 2 rows: 3
                  "a 6 2 0 1 1 1", "l"])
    assert out == [["a", 0, 1, 2], ["a", 1, 1, 2], ["a", 1, 1, 2], ["a", 5, 1, 2], ["a", 4, 1, 2], ["a", 4, 1, 2],
                   ["l", 1, 1, 2], ["a", 3, 1, 2], ["a", 0, 2, 4], ["l", 2, 2, 4]]


# --- the header and the binding ---
CALLS = ["gns_hh_hist_create", "gns_hh_hist_destroy", "gns_hh_hist_append", "gns_hh_hist_heavy_hitters",
        "gns_hh_hist_heavy_rows", "gns_hh_hist_times", "gns_hh_hist_stats", "gns_hh_hist_export"]


def test_header_declares_the_calls_and_lib_binds_them():
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load()
    for name in CALLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, f"{name} is not declared"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.EXPORTED
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs, (name, nargs, fn.argtypes)
    assert re.search(r"typedef struct gns_hh_hist gns_hh_hist;", txt)
    assert re.search(r"typedef struct gns_hh_hist_params\s*\{\s*uint32_t key_bytes;\s*uint64_t max_rows, max_flows;\s*int device;\s*\}", txt)
    assert re.search(r"typedef struct gns_hh_list\s*\{\s*uint32_t type;\s*const uint8_t \*rows;\s*uint64_t n;\s*\}", txt)
    assert ct.sizeof(_lib.HhHistParams) == 32 and ct.sizeof(_lib.HhList) == 24
    assert "a history of the sketch tasks' heavy-hitter lists. */" not in raw  # the exact history's "not offered" clause
    assert "querier.go:191-248" in raw and "writer_clickhouse.go:86-138" in raw


# --- Python argument errors, before any device call ---
def bare_history(K=4):
    h = HeavyHistory.__new__(HeavyHistory)  # no handle: the checks below come first
    h._h, h._L, h.key_bytes, h.device, h._hint = None, None, K, 0, {}
    return h


def test_python_argument_errors_come_first():
    h = bare_history(4)
    rows = np.zeros((3, 8), np.uint8)
    with pytest.raises(ValueError, match="negative limit"):
        h.heavy_hitters(0, limit=-1)
    with pytest.raises(ValueError, match="negative limit"):
        h.heavy_hitters_rows_device(0, limit=-1)
    for bad in (-1, 256, 1.5, True):
        with pytest.raises(ValueError, match="UInt8"):
            h.heavy_hitters(bad)
        with pytest.raises(ValueError, match="UInt8"):
            h.append(5, {bad: rows})
    with pytest.raises(ValueError, match="unsigned"):
        h.heavy_hitters(0, threshold=-1)
    with pytest.raises(ValueError, match="end_time .* int64"):
        h.heavy_hitters(0, end_time=1 << 63)
    with pytest.raises(ValueError, match="timestamp_ns .* int64"):
        h.append(-(1 << 63) - 1, {0: rows})
    for width in (7, 9, 4):
        with pytest.raises(ValueError, match=r"must be \[n, 8\]"):
            h.append(5, {0: np.zeros((3, width), np.uint8)})
    with pytest.raises(ValueError, match=r"flows must be \[n, 4\]"):
        h.append(5, {0: (np.zeros((3, 5), np.uint8), np.zeros(3, np.uint32))})
    with pytest.raises(ValueError, match="u32"):
        h.append(5, {0: (np.zeros((1, 4), np.uint8), np.array([1 << 32], np.uint64))})

    class FakeDevice:  # stands in for a device tensor: the mix is refused before any device call
        is_cuda, dtype, shape = True, None, (3, 8)
    import torch
    FakeDevice.dtype = torch.uint8
    fake = FakeDevice()
    fake.dim, fake.device, fake.contiguous, fake.data_ptr = (lambda: 2), torch.device("cuda", 0), (lambda: fake), (lambda: 0)
    with pytest.raises(ValueError, match="mix of host and device"):
        h.append(5, {0: fake, 1: rows})
    with pytest.raises(ValueError, match="key_bytes"):
        HeavyHistory(0)
    with pytest.raises(ValueError, match="key_bytes"):
        HeavyHistory(38)
    with pytest.raises(ValueError, match="unsigned"):
        HeavyHistory(4, max_rows=-1)
    # pack_rows: little-endian values behind the flow bytes
    p = pack_rows(np.array([[1, 2, 3, 4]], np.uint8), np.array([0x0A0B0C0D], np.uint32), 4)
    assert p.tolist() == [[1, 2, 3, 4, 0x0D, 0x0C, 0x0B, 0x0A]]
    assert pack_rows(np.zeros((0, 4), np.uint8), np.zeros(0, np.uint32), 4).shape == (0, 8)


def bare_task(name="s"):
    task = SketchTask.__new__(SketchTask)
    task.name_, task.flow_fields, task.flow_size, task.sketch = name, ["SrcPort", "DstPort"], 4, None
    return task


def test_task_calls_without_a_heavy_history_raise():
    task = bare_task()
    for call in (lambda: task.record_heavy(5), lambda: task.query_heavy_hitters(0, 10),
                 lambda: task.query_heavy_hitters(0, 0), lambda: task.save_heavy_history("x"),
                 lambda: task.restore_heavy_history("x")):
        with pytest.raises(ValueError, match="keep_heavy_history"):
            call()

    class Hist:  # a history stands in: the limit check still comes before it is asked
        def heavy_hitters(self, *a, **k):
            raise AssertionError("not reached")
    task.heavy_history = Hist()
    with pytest.raises(ValueError, match="negative limit"):
        task.query_heavy_hitters(0, -1)
    assert task.query_heavy_hitters(0, 0, end_time=5) == []


def test_manager_without_heavy_histories_is_unchanged(tmp_path):
    saved = []

    class Plain:  # a task as the Manager sees it: no history of either kind attached
        def __init__(self, name):
            self.n = name

        def name(self):
            return self.n

        def save(self, path):
            saved.append(path)
            open(path, "wb").close()

        def restore(self, path):
            saved.append("r:" + path)

    sk = bare_task("sk")
    sk.save = lambda path: (saved.append(path), open(path, "wb").close())
    sk.restore = lambda path: saved.append("r:" + path)
    mgr = Manager.__new__(Manager)

    class Group:
        Tasks = [Plain("ex"), sk]
    mgr.groups = [Group()]
    paths = mgr.checkpoint(str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ["ex.npz", "sk.npz"]
    assert sorted(os.listdir(tmp_path)) == ["ex.npz", "sk.npz"]  # no .heavy.npz, no .history.npz
    mgr.restore(str(tmp_path))
    assert saved[2:] == ["r:" + paths[0], "r:" + paths[1]]
    assert mgr.record(5) == {}          # no task has `record`: the exact tasks' call is unaffected
    assert mgr.keep_history() == {}
    with pytest.raises(ValueError, match="record_heavy: task sk has no heavy history"):
        mgr.record_heavy(5)
