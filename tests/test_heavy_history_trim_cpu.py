"""Retention and point queries of the heavy-hitter history without a GPU: HhHistPlan::trim_plan /
trimmed (gns_hhplan.hpp) in a stand-alone host program against a Python model, for every cut of a
six-snapshot, two-lane table; the header and the binding of gns_hh_hist_trim / _query; the Python
argument errors that come before any C call; the truth helpers on hand-written rows."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from go2netspectra_amd import HeavyHistory, Manager, SketchTask, _lib
from heavy_history_trim_truth import assert_fold_keeps_answers, dropped, folded, log_of, point, trim_out
from heavy_history_truth import HeavyTruth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "go2netspectra_amd", "csrc")
HEADER = os.path.join(HERE, "..", "include", "gns_sketch.h")

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "gns_hhplan.hpp"

// commands, one per line:
//   a <t> <k> (<type> <n>){k}   append (add_lane of every type with rows, publish)
//   p <before> <fold>           trim_plan: c, R, d, fold, noop, then R of every lane
//   t <before> <fold> <nbase>{lanes}   trimmed, unless the plan is a noop (prints 1 for a noop)
//   d   ts..., total rows, t.end_rows..., then per lane: type, rows, end_rows...
int main() {
    gns::HhHistPlan p;
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        long long a = 0;
        unsigned long long u = 0, w = 0;
        int fold = 0;
        switch (cmd) {
        case 'a': {
            unsigned k = 0;
            if (std::scanf("%lld %u", &a, &k) != 2 || k > 300) return 2;
            uint32_t types[300], pt[300];
            uint64_t ns[300], pn[300];
            for (unsigned i = 0; i < k; i++) {
                if (std::scanf("%llu %llu", &u, &w) != 2) return 2;
                types[i] = (uint32_t)u;
                ns[i] = w;
            }
            const int rc = p.append_check((int64_t)a, types, ns, k);
            if (rc == gns::HIST_OK) {
                unsigned np = 0;
                for (unsigned i = 0; i < k; i++)
                    if (ns[i]) { p.add_lane(types[i]); pt[np] = types[i]; pn[np] = ns[i]; np++; }
                p.publish((int64_t)a, pt, pn, np);
            }
            std::printf("a %d\n", rc);
            break;
        }
        case 'p': {
            if (std::scanf("%lld %d", &a, &fold) != 2) return 2;
            const gns::HhHistPlan::Trim x = p.trim_plan((int64_t)a, fold != 0);
            std::printf("p %llu %llu %u %d %d", (unsigned long long)x.t.c, (unsigned long long)x.t.R, x.t.d, (int)x.t.fold,
                        (int)x.t.noop);
            for (uint64_t r : x.R) std::printf(" %llu", (unsigned long long)r);
            std::printf("\n");
            break;
        }
        case 't': {
            if (std::scanf("%lld %d", &a, &fold) != 2) return 2;
            std::vector<uint64_t> nbase;
            for (size_t l = 0; l < p.lanes.size(); l++) {
                if (std::scanf("%llu", &u) != 1) return 2;
                nbase.push_back(u);
            }
            const gns::HhHistPlan::Trim x = p.trim_plan((int64_t)a, fold != 0);
            if (!x.t.noop) p = p.trimmed(x, nbase);
            std::printf("t %d\n", (int)x.t.noop);
            break;
        }
        case 'd': {
            std::printf("d");
            for (int64_t t : p.t.ts) std::printf(" %lld", (long long)t);
            std::printf(" | %llu", (unsigned long long)p.t.rows);
            for (uint64_t e : p.t.end_rows) std::printf(" %llu", (unsigned long long)e);
            for (const gns::HhHistPlan::Lane &l : p.lanes) {
                std::printf(" | %u %llu", l.type, (unsigned long long)l.rows);
                for (uint64_t e : l.end_rows) std::printf(" %llu", (unsigned long long)e);
                if (p.lane(l.type) < 0 || &p.lanes[(size_t)p.lane(l.type)] != &l) return 4;
            }
            std::printf("\n");
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
    tmp = tmp_path_factory.mktemp("hhtrimplan")
    src, exe = tmp / "hhtrim_driver.cpp", str(tmp / "hhtrim_driver")
    src.write_text(DRIVER)
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r.stdout.splitlines()
    return run


# --- the Python model of the plan ---
TS = [-50, -3, 0, 10, 11, 1 << 40]
COUNTS = {0: [5, 0, 7, 1, 0, 4], 9: [0, 0, 0, 6, 2, 0]}  # type 9's lane is created at snapshot 3


class Model:
    def __init__(self):
        self.ts, self.lanes = [], []  # lanes: [type, rows of each snapshot], in creation order

    def append(self, t, lists):
        for type, n in lists:
            if n and type not in [l[0] for l in self.lanes]:
                self.lanes.append([type, [0] * len(self.ts)])
        for l in self.lanes:
            l[1].append(dict(lists).get(l[0], 0))
        self.ts.append(t)
        return "a {} {} {}".format(t, len(lists), " ".join(f"{ty} {n}" for ty, n in lists))

    def plan(self, before, fold):
        c = sum(t < before for t in self.ts)
        R = [sum(l[1][:c]) for l in self.lanes]
        return c, R, (c - 1 if fold and c else c), (c == 0 or (fold and c == 1))

    def trim(self, before, fold, nbase):
        c, R, d, noop = self.plan(before, fold)
        if noop:
            return
        for l, b in zip(self.lanes, nbase):
            l[1] = ([b] if fold else []) + l[1][c:]
        self.ts = ([self.ts[c - 1]] if fold else []) + self.ts[c:]

    def dump(self):
        """The driver's `d` line."""
        cum = lambda v: np.cumsum(v).tolist() if len(v) else []
        total = [sum(l[1][i] for l in self.lanes) for i in range(len(self.ts))]
        out = "d" + "".join(f" {t}" for t in self.ts) + " | " + " ".join(str(x) for x in [sum(total)] + cum(total))
        for type, counts in self.lanes:
            out += " | " + " ".join(str(x) for x in [type, sum(counts)] + cum(counts))
        return out


def table():
    m, cmds = Model(), []
    for i, t in enumerate(TS):
        cmds.append(m.append(t, [(ty, COUNTS[ty][i]) for ty in COUNTS if COUNTS[ty][i] or ty == 0]))
    return m, cmds


def cuts():
    out = [TS[0] - 1]
    for i, t in enumerate(TS):
        out += [t, t + 1]
    return out + [(1 << 63) - 1, -(1 << 63)]


def test_plan_header_still_compiles_without_hip():
    txt = open(os.path.join(CSRC, "gns_hhplan.hpp")).read()
    assert "#include <hip" not in txt and "__device__" not in txt and "__global__" not in txt
    assert "trim_plan" in txt and "trimmed" in txt


@pytest.mark.parametrize("fold", [0, 1])
def test_every_cut_of_a_two_lane_table(driver, fold):
    """Every c = 0..6 (and the no-ops), with a lane created at snapshot 3: the plan, the trimmed
    table, and an append after the trim."""
    seen_c = set()
    for before in cuts():
        m, cmds = table()
        c, R, d, noop = m.plan(before, fold)
        seen_c.add(c)
        # a fold keeps any number of each lane's prefix rows, at most R; a lane without a prefix keeps none
        nbase = [(r + 1) // 2 if fold else 0 for r in R]
        cmds += [f"p {before} {fold}", "d", f"t {before} {fold} " + " ".join(map(str, nbase)), "d"]
        want = ["a 0"] * 6 + [f"p {c} {sum(R)} {d} {fold} {int(noop)} " + " ".join(map(str, R)), m.dump(), f"t {int(noop)}"]
        m.trim(before, fold, nbase)
        want.append(m.dump())
        if noop:
            assert want[-1] == want[-3]
        # the lanes stay, also one that lost every row; both take an append, and a new type gets its lane
        cmds += [m.append(TS[-1] + 5, [(9, 3), (0, 2), (200, 1)]), "d"]
        want += ["a 0", m.dump()]
        got = driver(cmds)
        assert got == want, (before, fold, got, want)
        if c >= 4 and not noop:  # type 9's lane existed at the base: its prefix is its own
            assert R[1] == sum(COUNTS[9][:c])
        if c <= 3:
            assert R[1] == 0
    assert seen_c == set(range(7))


def test_trim_twice_and_an_empty_table(driver):
    m, cmds = table()
    want = ["a 0"] * 6
    for before, fold, nbase in ((0, 1, [3, 0]), (11, 0, [0, 0]), (11, 1, [0, 0]), (1 << 41, 1, [2, 1]), (1 << 42, 0, [0, 0]),
                                (5, 0, [0, 0])):
        noop = m.plan(before, fold)[3]
        cmds += [f"t {before} {fold} " + " ".join(map(str, nbase)), "d"]
        m.trim(before, fold, nbase)
        want += [f"t {int(noop)}", m.dump()]
    assert m.ts == [] and [l[0] for l in m.lanes] == [0, 9]
    cmds += [m.append(-99, [(9, 1)]), "d"]  # timestamps start anew in an emptied table
    want += ["a 0", m.dump()]
    assert driver(cmds) == want


# --- the header and the binding ---
def test_header_declares_both_calls_and_lib_binds_them():
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load()
    for name, nargs in (("gns_hh_hist_trim", 4), ("gns_hh_hist_query", 8)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, f"{name} is not declared"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        assert name in _lib.EXPORTED and len(getattr(L, name).argtypes) == nargs
    assert "Not offered: roll-ups. */" in raw and "Not offered: retention" not in raw
    assert "writer_clickhouse.go:25-27" in raw and "one row per" in raw and "no tombstones" in raw
    go = open(os.path.join(HERE, "..", "integration", "go", "sketchgpu", "sketchgpu.go")).read()
    assert "func (y *HeavyHistory) Trim(before int64, fold bool)" in go
    assert "func (y *HeavyHistory) Query(end *int64, typ uint32, flows []byte)" in go


# --- Python argument errors, before any C call ---
def bare_history(K=4):
    h = HeavyHistory.__new__(HeavyHistory)  # no handle and no library: the checks below come first
    h._h, h._L, h.key_bytes, h.device, h._hint = None, None, K, 0, {}
    return h


def bare_task(name="s"):
    task = SketchTask.__new__(SketchTask)
    task.name_, task.flow_fields, task.flow_size, task.sketch = name, ["SrcPort", "DstPort"], 4, None
    return task


def test_python_argument_errors_come_first():
    h = bare_history(4)
    for bad in (2, -1, None, "yes", 0.5):
        with pytest.raises(ValueError, match="fold"):
            h.trim(5, fold=bad)
    with pytest.raises(ValueError, match="before_ns .* int64"):
        h.trim(1 << 63)
    for flows in (np.zeros((3, 5), np.uint8), np.zeros((3, 3), np.uint8), np.zeros(8, np.uint8), [b"12345"], [b"1234", b"123"]):
        with pytest.raises(ValueError, match="flows must be"):
            h.query(0, flows)
    for bad in (256, -1, 1.5, True):
        with pytest.raises(ValueError, match="UInt8"):
            h.query(bad, np.zeros((1, 4), np.uint8))
        with pytest.raises(ValueError, match="UInt8"):
            h.query_device(bad, None)
    with pytest.raises(ValueError, match="end_time .* int64"):
        h.query(0, np.zeros((1, 4), np.uint8), end_time=-(1 << 63) - 1)
    with pytest.raises(TypeError, match="device tensor"):
        h.query_device(0, np.zeros((1, 4), np.uint8))
    # an empty batch is answered without any call
    v, f = h.query(0, np.zeros((0, 4), np.uint8))
    assert v.dtype == np.uint64 and f.dtype == bool and len(v) == len(f) == 0
    v, f = h.query(3, [])
    assert len(v) == len(f) == 0

    task = bare_task()
    for bad in (0, True, -3, 1.5):
        with pytest.raises(ValueError, match="retain"):
            task.keep_heavy_history(retain=bad)
    for bad in (1, None, "no"):
        with pytest.raises(ValueError, match="drop"):
            task.keep_heavy_history(retain=2, drop=bad)
    assert getattr(task, "heavy_history", None) is None
    with pytest.raises(ValueError, match="keep_heavy_history"):
        task.query_heavy([b"1234"], 0)

    class Hist:  # a history stands in: the flow checks still come before it is asked
        def query(self, *a, **k):
            raise AssertionError("not reached")
    task.heavy_history = Hist()
    with pytest.raises(ValueError, match="4 bytes each"):
        task.query_heavy([b"12345"], 0)
    with pytest.raises(ValueError, match="2 fields expected"):
        task.query_heavy("1 2 3", 0)

    calls = []

    class T:
        def name(self):
            return "t"

        def keep_heavy_history(self, **kw):
            calls.append(kw)
            return "h"
    mgr = Manager.__new__(Manager)

    class Group:
        Tasks = [T()]
    mgr.groups = [Group()]
    assert mgr.keep_heavy_history(retain=3, drop=True, max_rows=64) == {"t": "h"}
    assert mgr.keep_heavy_history() == {"t": "h"}
    assert calls == [dict(retain=3, drop=True, max_rows=64), dict(retain=None, drop=False)]


def test_encode_flow_inverts_decode_flow():
    from go2netspectra_amd.task import decode_flow, encode_flow
    fields = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
    rng = np.random.default_rng(3)
    for i in range(50):
        b = bytearray(rng.integers(0, 256, 37, dtype=np.uint8).tobytes())
        if i % 3 == 0:
            b[:12] = bytes(10) + b"\xff\xff"  # IPv4-mapped: printed as a dotted quad
        if i % 5 == 0:
            b[20:32] = bytes(12)  # the reference's IPv4 slot: 4 bytes + 12 zero bytes
        assert encode_flow(decode_flow(bytes(b), fields), fields) == bytes(b)


# --- the truth helpers on hand-written rows ---
def key(a, b):
    return a.to_bytes(2, "big") + b.to_bytes(2, "big")


def test_truth_helpers_on_hand_written_rows():
    tr = HeavyTruth(["SrcPort", "DstPort"])
    a, b, c, d, e = key(1, 80), key(2, 80), key(3, 443), key(4, 53), key(0, 9)
    tr.record(10, {0: [(a, 100), (b, 70), (c, 90)], 1: [(a, 5000)]})
    tr.record(20, {0: [(a, 150), (d, 40)], 1: [(b, 7), (d, 0)]})
    tr.record(30, {0: [(a, 20), (c, 40), (e, 40)], 1: [(a, 1)]})
    # drop below 20 or 15: the four rows of 10 are gone; b is forgotten in type 0 (c comes back at 30), a in no type
    for before in (20, 15, 11):
        dr = dropped(tr, before)
        assert dr.times == [20, 30] and len(dr.rows) == 8
        assert dr.query(0, end_time=20) == [("1 80", 150), ("4 53", 40)]
        assert dr.query(0) == [("0 9", 40), ("3 443", 40), ("4 53", 40), ("1 80", 20)]
        assert dr.query(1, end_time=25) == [("2 80", 7), ("4 53", 0)] and dr.query(0, end_time=19) == []
        assert trim_out(tr, before, False) == [1, 4, 1, 8]
        assert trim_out(tr, before, True) == [0, 0, 0, 12]  # a fold of one snapshot is the snapshot itself
    assert trim_out(tr, 10, False) == [0, 0, 0, 12] and dropped(tr, 10).rows == tr.rows
    # drop below 30: type 0 forgets b and d, type 1 forgets b and d
    assert trim_out(tr, 30, False) == [2, 8, 4, 4]
    assert point(dropped(tr, 30), 0, b) is None and point(tr, 0, b) == 70 and point(tr, 0, b, 9) is None
    assert trim_out(tr, 31, False) == [3, 12, 8, 0] and dropped(tr, 31).times == []
    # fold below 30: a's row of 10 is superseded at 20 and goes; the base holds, in log order, b, c, a, d | a, b, d
    fo = folded(tr, 30)
    assert fo.times == [20, 30] and trim_out(tr, 30, True) == [1, 1, 0, 11]
    assert log_of(fo, 0) == [(0, b, 70), (0, c, 90), (0, a, 150), (0, d, 40), (1, a, 20), (1, c, 40), (1, e, 40)]
    assert log_of(fo, 1) == [(0, a, 5000), (0, b, 7), (0, d, 0), (1, a, 1)]
    assert fo.query(0, end_time=19) == [] and fo.query(0, end_time=20) == tr.query(0, end_time=20)
    assert_fold_keeps_answers(tr, fo, (0, 1, 2))
    fa = folded(tr, 1000)  # fold everything: one snapshot under 30, one row per pair
    assert fa.times == [30] and len(fa.rows) == 8 and trim_out(tr, 1000, True) == [2, 4, 0, 8]
    assert_fold_keeps_answers(tr, fa, (0, 1))
    assert point(fa, 1, d) == 0 and point(fa, 1, c) is None and point(fa, 0, a, 29) is None
    with pytest.raises(AssertionError):  # the statement has teeth: a drop does change answers after the cut
        assert_fold_keeps_answers(tr, dropped(tr, 30), (0,))
