"""The history delta on the GPU (gns_ex_hist_rollup_between, gns_ex_movers): what changed between
two times, re-keyed on the device, equals history_delta_truth.py -- every group, keys sorted, all
five columns bit for bit, and the rows-selected / slots-claimed pair.  The base is the history of
test_exact_history_rollup_gpu.py (1,500 flows in 6 snapshots: two whole, a delta, a reset, a
delta, an empty one, a delta) recorded into a StoredTruth, which stores what the task stores;
GNS_EX_ROLLUP_PIECE=512 cuts the log into pieces, and the first piece holds no selected row for
late windows."""
import ctypes as ct
import ipaddress

import numpy as np
import pytest

from exact_query_truth import FIVE, batch_of, key_bytes_of
from history_delta_truth import (M64, StoredTruth, delta_truth, movers_truth, rowlog_delta, rowlog_sets, signed,
                                 window_sets)
from history_rollup_truth import RowLog, combine
from prefix_truth import prefix_stream
from test_exact_history_gpu import feed_oracle, rows_of
from test_exact_history_rollup_gpu import (CUTS, FULL, NFLOWS, RESET, TS, check, history_of, ip4, new_agg, new_task,
                                           query_times, record_base, sorted_rows)

pytestmark = pytest.mark.gpu

PERMUTED = ["Protocol", "DstPort", "DstIP", "SrcPort", "SrcIP"]
LAYOUTS = [["SrcIP"], ["DstIP", "DstPort"], ["Protocol"], FIVE, PERMUTED]
IDS = lambda f: "-".join(f) if isinstance(f, list) else str(f)
I64 = np.iinfo(np.int64)


@pytest.fixture(autouse=True)
def piece(monkeypatch):
    monkeypatch.setenv("GNS_EX_ROLLUP_PIECE", "512")


def s_of(T, ts=TS):
    """s(T): the newest snapshot at or before T; -1 before the first; None is the newest."""
    return len(ts) - 1 if T is None else sum(1 for t in ts if t <= T) - 1


def windows(times=None):
    """Every ordered pair (T0, T1), T0 <= T1; None stands before everything as T0, after as T1."""
    times = query_times() if times is None else times
    return [(a, b) for a in times for b in times if a is None or b is None or a <= b]


def claimed(tr, T0, T1, fields, prefix=None):
    return len(delta_truth(tr, T0, T1, fields, prefix, keep_zero=True)[0])


def record_stream(task, tr, oracle, full):
    """record_base with the stored form of every snapshot given: the same stream, cuts, times and reset."""
    t, ipver, ts = prefix_stream(NFLOWS)
    for i in range(6):
        if CUTS[i] is not None:
            sel = slice(*CUTS[i])
            task.process_packets(batch_of(t, ipver, ts, sel))
            feed_oracle(tr.oracle, t, ipver, ts, sel)
        task.record(TS[i], full=full[i])
        tr.record(TS[i], tr.oracle.export())
        if i + 1 == RESET:
            task.reset()
            tr.oracle = oracle.Exact(FIVE)


def build_base(oracle, full=FULL):
    task = new_task()
    hist = task.keep_history(max_rows=256, max_flows=32)
    tr = StoredTruth(FIVE, full)
    tr.oracle = oracle.Exact(FIVE)
    if full == FULL:
        record_base(task, tr, oracle)
    else:
        record_stream(task, tr, oracle, full)
    assert hist.stats()["rows"] == len(tr.ts), "StoredTruth does not store what the task stores"
    return task, hist, tr


@pytest.fixture(scope="module")
def base(gpu, oracle):
    task, hist, tr = build_base(oracle)
    assert 3_000 <= len(tr.ts) <= 6_000
    # late windows select nothing in the first piece of 512 log rows: snapshot 1 superseded all of snapshot 0
    plus, minus = window_sets(tr, TS[2], None)
    assert plus and minus and min(plus + minus) >= 512
    yield task, hist, tr
    task.agg.close()
    hist.close()


def roll(hist, fields, T0, T1, prefix=None, dst=None):
    dst = new_agg(fields) if dst is None else dst
    return dst, dst.rollup_from_history(hist, end_time=T1, prefix=prefix, start_time=T0)


# --- 1. every window at every layout ---
@pytest.mark.parametrize("fields", LAYOUTS, ids=IDS)
def test_every_window_equals_the_truth(base, fields):
    _, hist, tr = base
    negative = empty = 0
    most = 0
    for T0, T1 in windows():
        want, n = delta_truth(tr, T0, T1, fields)
        dst = new_agg(fields)
        view = dst.view()
        out = dst.rollup_from_history(hist, end_time=T1, start_time=T0)
        assert out == (n, claimed(tr, T0, T1, fields)), (fields, T0, T1, out)
        check(dst, want, (fields, T0, T1))
        s0, s1 = (-1 if T0 is None else s_of(T0)), s_of(T1)
        if s1 < 0 or s0 == s1:
            assert out == (0, 0) and want == [] and view.refresh() == 0, (T0, T1)  # no position was spent
            empty += 1
        else:
            assert view.refresh() == len(tr.seen(T1)), (T0, T1)  # dst advanced by the rows as of s1
        if 0 <= s0 <= 2 < s1:  # the window spans the reset after snapshot 2
            negative += any(signed(r[3]) < 0 for r in want)
        most = max(most, len(want))
        view.close()
        dst.close()
    assert negative, "no window across the reset holds a negative change"
    assert empty, "no window with s0 == s1"
    if fields == ["Protocol"]:
        assert 0 < most < 8  # few groups: every wave reduces, the rest meets in the LDS table


# --- 2. no start time: the as-of roll-up, bit for bit ---
def test_no_start_time_is_the_rollup_as_of_the_end(base):
    from go2netspectra_amd import _lib, make_prefix
    _, hist, tr = base
    L = _lib.load()
    for fields, prefix in ((["SrcIP"], None), (FIVE, None), (["DstIP", "DstPort"], {"DstIP": (24, 64)})):
        for T1 in query_times():
            ref = new_agg(fields)
            out = ref.rollup_from_history(hist, end_time=T1, prefix=prefix)
            rows = sorted_rows(ref)
            a, out_a = roll(hist, fields, None, T1, prefix)
            b, out_b = roll(hist, fields, TS[0] - 10, T1, prefix)  # (every query time lies at or after it)
            # the C call with a NULL start: the window kernels with s0 = -1
            c = new_agg(fields)
            o = (ct.c_uint64 * 2)()
            end = None if T1 is None else ct.byref(ct.c_int64(T1))
            px = None if prefix is None else ct.byref(make_prefix(prefix))
            assert L.gns_ex_hist_rollup_between(c._h, hist._h, None, end, px, o) == 0
            assert out_a == out_b == (int(o[0]), int(o[1])) == out, (fields, T1)
            assert sorted_rows(a) == sorted_rows(b) == sorted_rows(c) == rows, (fields, T1)
            assert rows == delta_truth(tr, None, T1, fields, prefix)[0]
            for h in (ref, a, b, c):
                h.close()


# --- 3. prefixes ---
PREFIXES = [(["SrcIP"], {"SrcIP": (24, 64)}), (["SrcIP"], {"SrcIP": (8, 32)}), (["Protocol", "SrcIP"], {"SrcIP": (17, 65)}),
            (["SrcIP", "DstIP"], {"SrcIP": (24, 64), "DstIP": (16, 48)})]


@pytest.mark.parametrize("fields,prefix", PREFIXES, ids=IDS)
def test_prefix_windows(base, fields, prefix):
    _, hist, tr = base
    for T0, T1 in ((TS[1], TS[3]), (TS[2], None), (TS[0], TS[2])):
        want, n = delta_truth(tr, T0, T1, fields, prefix)
        plain = delta_truth(tr, T0, T1, fields)[0]
        assert 0 < len(want) < len(plain)
        dst, out = roll(hist, fields, T0, T1, prefix)
        assert out == (n, claimed(tr, T0, T1, fields, prefix))
        check(dst, want, (fields, prefix, T0, T1))
        dst.close()


# --- 4. telescoping: two windows into one destination ---
@pytest.mark.parametrize("fields", [["SrcIP"], FIVE], ids=IDS)
def test_two_windows_add_up_to_their_union(base, fields):
    _, hist, tr = base
    # (None as T0 is the as-of call: in the second place its table growth forgets the groups the first call
    # left without packets -- the documented limit -- so that triple runs in stream order only)
    for T0, T1, T2 in ((TS[0], TS[2], TS[5]), (TS[1], TS[3], None), (TS[0] - 10, TS[1], TS[3]), (None, TS[1], TS[3])):
        whole = {r[0]: r[3:] for r in delta_truth(tr, T0, T2, fields)[0]}
        # keep_zero: a group whose packets did not change in one window claimed its slot there all the same, and
        # the other window's rows add to what it holds ("a key already in dst")
        a, b = delta_truth(tr, T0, T1, fields, keep_zero=True)[0], delta_truth(tr, T1, T2, fields, keep_zero=True)[0]
        want = combine(a, b)
        assert {r[0]: r[3:] for r in want} == whole, "the truth's counts do not telescope"
        assert any(r[3] == 0 for r in a + b)
        for first in (0, 1) if T0 is not None else (0,):
            dst = new_agg(fields)
            for w in ((T0, T1), (T1, T2))[::1 if first == 0 else -1]:
                dst.rollup_from_history(hist, end_time=w[1], start_time=w[0])
            check(dst, want, (fields, T0, T1, T2, first))
            dst.close()


# --- 5. whole views and deltas of one stream ---
def test_whole_views_and_deltas_give_the_same_changes(gpu, oracle):
    wtask, whole, wtr = build_base(oracle, full=[True] * 6)
    dtask, delta, dtr = build_base(oracle, full=[True] + [False] * 5)
    assert whole.stats()["rows"] > delta.stats()["rows"]
    wider = 0
    for T0, T1 in windows([TS[0] - 10, TS[0], TS[1], TS[2], TS[3], TS[5], None]):
        a, _ = roll(whole, FIVE, T0, T1)
        b, _ = roll(delta, FIVE, T0, T1)
        rows = sorted_rows(a)
        assert rows == sorted_rows(b) == delta_truth(dtr, T0, T1, FIVE)[0], (T0, T1)
        a.close()
        b.close()
        a, _ = roll(whole, ["SrcIP"], T0, T1)
        b, _ = roll(delta, ["SrcIP"], T0, T1)
        ra, rb = sorted_rows(a), sorted_rows(b)
        assert [(r[0], r[3], r[4]) for r in ra] == [(r[0], r[3], r[4]) for r in rb], (T0, T1)
        assert ra == delta_truth(wtr, T0, T1, ["SrcIP"])[0] and rb == delta_truth(dtr, T0, T1, ["SrcIP"])[0], (T0, T1)
        wider += ra != rb  # the whole views' plus rows of unchanged flows widen a group's times
        a.close()
        b.close()
    assert wider
    for h in (wtask.agg, whole, dtask.agg, delta):
        h.close()


# --- 6. a destination that is not empty ---
def test_a_destination_that_ingested_packets(base, oracle):
    _, hist, tr = base
    fields = ["SrcIP"]
    t, ipver, ts = prefix_stream(NFLOWS)
    before, after = slice(40_000, 43_000), slice(43_000, 46_000)
    dst = new_agg(fields)  # max_flows=64: grows during the call
    view = dst.view()
    dst.insert_tuples(batch_of(t, ipver, ts, before))
    dst.flush()
    o = oracle.Exact(fields)
    feed_oracle(o, t, ipver, ts, before)
    as_rows = lambda exp: sorted((key_bytes_of(k, fields),) + tuple(v) for k, v in exp.items())
    rows0 = as_rows(o.export())
    assert sorted_rows(dst) == rows0
    cursor = view.refresh()
    T0, T1 = TS[1], TS[5]
    rolled, n = delta_truth(tr, T0, T1, fields, keep_zero=True)
    grown = dst.dict_stats()["growths"]
    out = dst.rollup_from_history(hist, end_time=T1, start_time=T0)
    want = combine(rows0, rolled)
    assert out == (n, len({r[0] for r in rolled} - {r[0] for r in rows0})) and 0 < out[1] < len(rolled)
    assert any(signed(r[3]) < 0 for r in rolled)
    check(dst, want, "counts add the changes, times widen")
    assert dst.dict_stats()["growths"] > grown
    c2 = view.refresh(cursor)
    assert c2 == cursor + len(tr.seen(T1))
    touched = {r[0] for r in rolled}
    assert sorted(rows_of(view.snapshot_arrays())) == [r for r in want if r[0] in touched]
    # packets inserted afterwards add to the changed counts
    dst.insert_tuples(batch_of(t, ipver, ts, after))
    dst.flush()
    o2 = oracle.Exact(fields)
    feed_oracle(o2, t, ipver, ts, after)
    # (from the flows the table holds now: a group whose packets did not change is none, and what its slot
    # still holds is gone with the next growth of the table -- the documented limit)
    every = {r[0]: (r[3], r[4]) for r in want}
    for k, _, _, pk, by in as_rows(o2.export()):
        p0, b0 = every.get(k, (0, 0))
        every[k] = ((p0 + pk) & M64, (b0 + by) & M64)
    every = {k: v for k, v in every.items() if k in {r[0] for r in want} or k not in {r[0] for r in rolled}}
    keys = sorted(every) + [bytes(15) + b"\x01"]
    got = dst.query_many(np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 16))
    assert [int(g) for g in got] == [((pk << 32) | by) & M64 for pk, by in map(every.get, keys[:-1])] + [0]  # task.go:323
    live = {r[0]: (r[3], r[4]) for r in sorted_rows(dst) if r[0] in every}
    assert live == {k: v for k, v in every.items() if v[0] != 0}
    view.close()
    dst.close()


# --- 7. crafted rows through append_rows ---
def crafted_log():
    """(SrcIP, SrcPort) rows in three snapshots.  Snapshot 10: 600 filler rows of group 9 and the
    old rows of the crafted keys among its first rows; snapshot 20 (behind piece 1): their new
    rows; snapshot 30: a few more."""
    fields = ["SrcIP", "SrcPort"]
    log = RowLog(fields)
    key = lambda rows: np.frombuffer(b"".join(ip4(10, 0, 0, g) + p.to_bytes(2, "big") for g, p in rows), np.uint8).reshape(-1, 18)
    u = lambda xs: np.array(xs, np.uint64)
    # group 1: bytes 1 -> 2^63 + 5; group 2: packets equal, bytes 10 -> 20; group 3: packets 2^63 + 1 -> 1
    # group 4: ten rows in a row (one wave reduces them); group 5: two rows
    old = [(1, 1), (2, 1), (3, 1)] + [(4, p) for p in range(10)] + [(5, 1), (5, 2)]
    filler = [(9, 100 + i) for i in range(600)]
    n = len(old)
    log.append(10, key(old + filler), list(range(-n, 0)) + [5] * 600, list(range(n)) + [6] * 600,
               u([7, 5, (1 << 63) + 1] + [3] * 10 + [2, 2] + [1] * 600), u([1, 10, 9] + [100] * 10 + [50, 60] + [4] * 600))
    log.append(20, key(old), [I64.min] + [-3] * (n - 1), [I64.max] + [9] * (n - 1),
               u([8, 5, 1] + [4] * 10 + [1, 5]), u([(1 << 63) + 5, 20, 9] + [90] * 10 + [50, 600]))
    log.append(30, key([(4, 0), (5, 1), (6, 1), (9, 100)]), [1, 2, 3, 4], [1, 2, 3, 4], u([9, 9, 9, 9]), u([1, 2, 3, 4]))
    return log


def test_crafted_rows(gpu):
    log = crafted_log()
    hist = history_of(log)
    plus, minus = rowlog_sets(log, 10, 20)
    assert {s for s, _ in minus} == {0} and max(i for _, i in minus) < 512 and {s for s, _ in plus} == {1}
    assert len(log.snaps[0][1]) > 512  # log rows of snapshot 1 start behind piece 0: a key's minus and plus rows in different pieces
    want, n = rowlog_delta(log, 10, 20, ["SrcIP"])
    by_ip = {r[0]: r for r in want}
    assert signed(by_ip[ip4(10, 0, 0, 1)][4]) == -(1 << 63) + 4 and by_ip[ip4(10, 0, 0, 1)][3] == 1  # 2^63 + 4 wraps
    assert by_ip[ip4(10, 0, 0, 1)][1:3] == (I64.min, I64.max)
    assert ip4(10, 0, 0, 2) not in by_ip  # packets 5 -> 5: no flow, its byte change of 10 is not reported
    assert signed(by_ip[ip4(10, 0, 0, 3)][3]) == -(1 << 63)
    assert by_ip[ip4(10, 0, 0, 4)][3:] == (10, (-100) & M64) and by_ip[ip4(10, 0, 0, 5)][3:] == (2, 540)
    assert ip4(10, 0, 0, 9) not in by_ip and n == 30
    for T0, T1 in ((10, 20), (None, 20), (10, None), (20, 30), (5, 10), (20, 25)):
        for fields in (["SrcIP"], ["SrcIP", "SrcPort"], ["SrcPort", "SrcIP"]):
            want, n = rowlog_delta(log, T0, T1, fields)
            dst, out = roll(hist, fields, T0, T1)
            assert out == (n, len(rowlog_delta(log, T0, T1, fields, keep_zero=True)[0])), (T0, T1, fields)
            check(dst, want, (T0, T1, fields))
            if fields == ["SrcIP"] and (T0, T1) == (10, 20):
                keys, vals = dst.movers(0)
                assert (bytes(keys[0]), int(vals[0])) == (ip4(10, 0, 0, 3), -(1 << 63))  # magnitude 2^63 leads
                assert [(bytes(k), int(v)) for k, v in zip(keys, vals)] == movers_truth(want, 0)
                keys, vals = dst.movers(1, direction=-1)
                assert [(bytes(k), int(v)) for k, v in zip(keys, vals)] == movers_truth(want, 1, -1)
            dst.close()
    hist.close()


# --- 8. movers ---
def listed(pair):
    return [(bytes(k), int(v)) for k, v in zip(*pair)]


def test_movers_across_the_reset(base):
    from go2netspectra_amd import HeavyHitter, _lib
    task, hist, tr = base
    T0, T1 = TS[1], None
    L = _lib.load()
    cut_inside_a_tie = 0
    for fields in (FIVE, ["SrcIP"]):
        rows = delta_truth(tr, T0, T1, fields)[0]
        tab = hist.delta(fields, start_time=T0, end_time=T1)
        check(tab, rows, fields)
        for metric in (0, 1):
            every = movers_truth(rows, metric)
            assert any(v < 0 for _, v in every) and any(v > 0 for _, v in every)
            mid = sorted(abs(v) for _, v in every)[len(every) // 2]
            tie = next(i for i in range(1, len(every)) if abs(every[i][1]) == abs(every[i - 1][1]))
            for direction in (1, -1, 0):
                for thr in (0, 1, mid):
                    full = movers_truth(rows, metric, direction, thr)
                    for limit in (0, 1, 10, tie, len(full) + 7):
                        want = movers_truth(rows, metric, direction, thr, limit)
                        assert listed(tab.movers(metric, direction, thr, limit)) == want, (fields, metric, direction, thr, limit)
                        if limit and limit < len(full) and abs(full[limit][1]) == abs(full[limit - 1][1]):
                            cut_inside_a_tie += 1
                assert movers_truth(rows, metric, direction, 0) == movers_truth(rows, metric, direction, 1)
            # a capacity that is too small: the length is reported, nothing is written
            n = ct.c_uint64(len(every) - 1)
            keys, vals = np.full((len(every), tab.key_bytes), 0xAB, np.uint8), np.full(len(every), 7, np.int64)
            assert L.gns_ex_movers(tab._h, metric, 0, 1, 0, keys.ctypes.data, vals.ctypes.data, ct.byref(n)) == 0
            assert n.value == len(every) and (keys == 0xAB).all() and (vals == 7).all()
            n = ct.c_uint64(0)
            assert L.gns_ex_movers(tab._h, metric, 2, 1, 0, None, None, ct.byref(n)) == _lib.GNS_E_ARG
            assert L.gns_ex_movers(tab._h, 2, 0, 1, 0, None, None, ct.byref(n)) == _lib.GNS_E_ARG
            if fields == FIVE:
                assert listed(hist.movers(fields, metric, -1, 1, 5, start_time=T0, end_time=T1)) == movers_truth(rows, metric, -1, 1, 5)
                names = {key_bytes_of(k, FIVE): k for k in tr.key}
                for direction in (0, 1, -1):
                    got = task.movers(metric, 9, start_time=T0, end_time=T1, direction=direction)
                    assert got == [HeavyHitter(names[k], v) for k, v in movers_truth(rows, metric, direction, 1, 9)]
                assert task.movers(metric, 0, start_time=T0) == [] and task.movers(2, 5, start_time=T0) == []
        tab.close()
    assert cut_inside_a_tie, "no limit cut inside a run of equal magnitudes"


# --- 9. window totals ---
def test_window_totals(base):
    from go2netspectra_amd import Change, TaskSummary, make_filter
    task, hist, tr = base
    v4 = next(p["SrcIP"] for p in tr.parts if "." in p["SrcIP"])
    net = str(ipaddress.ip_network(v4 + "/16", strict=False))
    truth = [{}, {"Protocol": 6}, {"SrcIP": net}]
    engine = [make_filter(), make_filter(protocol=6), make_filter(src_ip=net)]
    moved = 0
    for T0, T1 in ((TS[1], TS[3]), (TS[0], TS[1]), (TS[2], None), (TS[0] - 10, TS[5]), (TS[3], TS[4])):
        want = []
        for f in truth:
            a, b = tr.summary(f, T1), tr.summary(f, T0)
            want.append(Change(a.flows - b.flows, signed(a.packets - b.packets), signed(a.bytes - b.bytes)))
        assert hist.aggregate(engine, start_time=T0, end_time=T1) == want, (T0, T1)
        moved += want[0].packets != 0 and want[2] != Change()
        c = want[1]
        assert task.aggregate_flows(protocol=6, start_time=T0, end_time=T1) == TaskSummary("h", c.bytes, c.packets, c.flows)
    assert moved >= 3
    assert hist.aggregate(engine, start_time=TS[3], end_time=TS[4]) == [Change()] * 3  # the empty snapshot


# --- 10. after a trim ---
def test_windows_after_fold_and_drop(base, oracle):
    from go2netspectra_amd import ExactHistory
    _, hist0, tr = base
    task, hist, _ = build_base(oracle)
    layouts = (["SrcIP"], FIVE)
    answer = lambda h, T0, T1: [sorted_rows(roll(h, f, T0, T1)[0]) for f in layouts]
    pairs = windows([TS[0] - 10, TS[1], TS[2], TS[3], TS[5], None])
    pre = {w: answer(hist0, *w) for w in pairs}
    hist.trim(TS[2], fold=True)  # snapshots 0..1 fold into one base under TS[1]; answers hold from TS[1] on
    base_ts = hist.times()[0]
    assert base_ts == TS[1]
    for T0, T1 in pairs:
        if T0 is not None and T0 >= TS[2]:
            assert answer(hist, T0, T1) == pre[T0, T1], (T0, T1)
        elif T0 is not None and T0 < base_ts:  # a start before the base answers as no start at all
            assert answer(hist, T0, T1) == answer(hist, None, T1), (T0, T1)
    # drop: equal to a history of the kept snapshots, and to its truth
    keys, st, en, pk, by, written, times = hist0.export_log()
    _, dropped, _ = build_base(oracle)
    dropped.trim(TS[3], fold=False)
    later, log = ExactHistory(FIVE, max_rows=256, max_flows=32), RowLog(FIVE)
    for s in range(3, 6):
        m = written == s
        later.append_rows(keys[m], st[m], en[m], pk[m], by[m], TS[s])
        log.append(TS[s], keys[m], st[m], en[m], pk[m], by[m])
    for T0, T1 in pairs:
        got = answer(dropped, T0, T1)
        assert got == answer(later, T0, T1) == [rowlog_delta(log, T0, T1, f)[0] for f in layouts], (T0, T1)
    for h in (task.agg, hist, dropped, later):
        h.close()


# --- 11. errors ---
def test_errors_come_before_any_device_work(base):
    from go2netspectra_amd import ExactHistory, _lib
    _, hist, _ = base
    L = _lib.load()
    t, ipver, ts = prefix_stream(NFLOWS)
    dst = new_agg(["SrcIP", "DstPort"])
    dst.insert_tuples(batch_of(t, ipver, ts, slice(0, 2_000)))
    dst.flush()
    snap0 = [a.tobytes() for a in dst.snapshot_arrays()]
    view = dst.view()
    out = (ct.c_uint64 * 2)(3, 4)
    call = L.gns_ex_hist_rollup_between
    i64 = lambda v: ct.byref(ct.c_int64(v))
    # the window ends before it starts
    assert call(dst._h, hist._h, i64(5), i64(4), None, out) == _lib.GNS_E_ARG and b"window" in L.gns_last_error()
    assert call(dst._h, hist._h, i64(4), i64(4), None, out) == 0 and (out[0], out[1]) == (0, 0)  # equal times: empty
    out[0], out[1] = 3, 4
    with pytest.raises(ValueError, match="start_time"):
        dst.rollup_from_history(hist, end_time=4, start_time=5)
    with pytest.raises(ValueError, match="start_time"):
        hist.delta(["SrcIP"], start_time=TS[3], end_time=TS[2])
    # a layout the history cannot give
    narrow = ExactHistory(["SrcIP"], max_rows=16, max_flows=16)
    assert call(dst._h, narrow._h, None, None, None, out) == _lib.GNS_E_ARG and b"DstPort" in L.gns_last_error()
    with pytest.raises(ValueError, match="DstPort"):
        dst.rollup_from_history(narrow, start_time=0)
    with pytest.raises(ValueError, match="DstPort"):
        narrow.delta(["SrcIP", "DstPort"], start_time=0)
    # a bad prefix
    px = _lib.Prefix(33, 128, 32, 128)
    assert call(dst._h, hist._h, i64(0), None, ct.byref(px), out) == _lib.GNS_E_ARG and b"prefix" in L.gns_last_error()
    with pytest.raises(ValueError):
        dst.rollup_from_history(hist, start_time=0, prefix={"SrcIP": (8, 129)})
    assert call(None, hist._h, None, None, None, out) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()
    with pytest.raises(ValueError):
        dst.rollup_from_history(hist, start_time=1 << 63)
    assert [a.tobytes() for a in dst.snapshot_arrays()] == snap0 and (out[0], out[1]) == (3, 4)
    assert view.refresh() == 2_000  # no positions were spent
    for h in (view, dst, narrow):
        h.close()
    # another device index, through the argument check alone (one device suffices)
    other = ExactHistory.__new__(ExactHistory)
    other._h, other._L, other.key_fields, other.key_bytes, other.device = hist._h, hist._L, FIVE, 37, hist.device + 1
    probe = new_agg(["SrcIP"])
    with pytest.raises(ValueError, match="device"):
        probe.rollup_from_history(other, start_time=TS[0])
    other._h = None  # (not this object's to destroy)
    assert sorted_rows(probe) == []
    probe.close()


def test_a_destination_on_another_device(base):
    import torch
    from go2netspectra_amd import _lib
    if torch.cuda.device_count() < 2:
        pytest.skip("a destination on another device needs two GPUs")
    _, hist, _ = base
    L = _lib.load()
    out = (ct.c_uint64 * 2)(3, 4)
    call = L.gns_ex_hist_rollup_between
    i64 = lambda v: ct.byref(ct.c_int64(v))
    far = new_agg(["SrcIP"], device=1)
    with pytest.raises(ValueError, match="device"):
        far.rollup_from_history(hist, start_time=TS[0])
    assert call(far._h, hist._h, i64(TS[0]), None, None, out) == _lib.GNS_E_ARG and b"device" in L.gns_last_error()
    far.close()
