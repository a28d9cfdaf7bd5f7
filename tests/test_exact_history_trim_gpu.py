"""Trim, export and restore of the exact history on the GPU (gns_ex_hist_trim / _export /
_append_rows): after a trim every answer as of a time equals the reference's SQL over the
trimmed snapshot rows (history_trim_truth.py), an exported log restored into a fresh history
answers the same, rejected calls change nothing, and ``retain`` keeps a bounded window.  The
stream is that of test_exact_history_gpu.py: 18,000 packets, 2,500 flows, six snapshots, a reset
of the source after the third."""
import threading

import numpy as np
import pytest

from exact_query_truth import FIVE, batch_of, got_heavy, to_filter
from history_truth import HistoryTruth
from history_trim_truth import counts, delta_truth, expired, joined, log_model, subset, trimmed_truth
from test_exact_history_gpu import (LAYOUT_IDS, LAYOUTS, NSNAP, TS, assert_history_equals_truth, e_arg,
                                    feed_oracle, interval, make_filters, new_task, query_times, rows_of, stream,
                                    unique_batch)

pytestmark = pytest.mark.gpu

RESET = 3  # the source is reset after this many intervals
NFILT = 24
LOG = ("keys", "start", "end", "packets", "bytes", "written", "times")
_TRUTH, _FILT = {}, {}


def truth_of(oracle, fields, full):
    """The stored rows of the six snapshots, built once per layout: the whole table at every
    snapshot (full), or only the flows touched in the interval (deltas)."""
    if tuple(fields) not in _TRUTH:
        t, ipver, ts = stream()
        tr, o = HistoryTruth(fields), oracle.Exact(fields)
        for i in range(NSNAP):
            feed_oracle(o, t, ipver, ts, interval(i))
            tr.record(TS[i], o.export())
            if i + 1 == RESET:
                o = oracle.Exact(fields)
        _TRUTH[tuple(fields)] = (tr, delta_truth(tr, TS, reset_after=RESET))
    return _TRUTH[tuple(fields)][0 if full else 1]


def filters_of(fields):
    if tuple(fields) not in _FILT:
        f = make_filters(fields, NFILT)
        _FILT[tuple(fields)] = (f, [to_filter(x) for x in f])
    return _FILT[tuple(fields)]


def build(fields, full, first=0, last=NSNAP, task=None, **kw):
    """A task whose history holds snapshots first..last-1 of the stream."""
    t, ipver, ts = stream()
    if task is None:
        task = new_task(fields)
        task.keep_history(max_rows=256, max_flows=32, **kw)
    for i in range(first, last):
        task.process_packets(batch_of(t, ipver, ts, interval(i)))
        task.record(TS[i], full=full)
        if i + 1 == RESET:
            task.reset()
    return task, task.history


def check(hist, tr, times, fields, what):
    filters, engine_filters = filters_of(fields)
    matches = [tr.matches(f) for f in filters]
    assert hist.times() == list(times), what
    st = hist.stats()
    assert (st["snapshots"], st["rows"], st["keys"]) == (len(times),) + counts(tr), (what, st)
    for T in query_times():
        assert_history_equals_truth(hist, tr, filters, engine_filters, matches, T, what)


def befores():
    return [TS[0] - 10] + [x + d for x in TS for d in (0, 1)] + [TS[-1] + (1 << 40)]


def answers(hist, fields, T):
    """Everything a query as of T returns, bit for bit."""
    _, engine_filters = filters_of(fields)
    return ([(s.flows, s.packets, s.bytes) for s in hist.aggregate(engine_filters, end_time=T)],
            got_heavy(*hist.heavy_hitters(0, end_time=T)), got_heavy(*hist.heavy_hitters(1, 1500, 7, end_time=T)),
            [a.tobytes() for a in hist.snapshot_arrays(end_time=T)])


def whole_answers(hist, fields):
    _, engine_filters = filters_of(fields)
    return [(hist.aggregate(engine_filters, end_time=T), answers(hist, fields, T)) for T in query_times()]


def assert_same_log(got, want, what):
    for name, a, b in zip(LOG, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"{what}: {name} differs"


# --- 1. every trim of the six-snapshot history against the trimmed truth ---
@pytest.mark.parametrize("fold", [False, True], ids=["drop", "fold"])
@pytest.mark.parametrize("full", [False, True], ids=["deltas", "whole"])
@pytest.mark.parametrize("fields", LAYOUTS, ids=LAYOUT_IDS)
def test_trim_against_the_truth(gpu, oracle, fields, full, fold):
    base = truth_of(oracle, fields, full)
    trimmed = {}  # by c: TS[i] + 1 and TS[i + 1] expire the same snapshots, the truth is asked once
    for before in befores():
        c = expired(TS, before)
        if c not in trimmed:
            trimmed[c] = trimmed_truth(base, TS, before, fold)
        task, hist = build(fields, full)
        rows0 = hist.stats()["rows"]
        out = hist.trim(before, fold=fold)
        tr, times = trimmed[c]
        check(hist, tr, times, fields, (fields, full, fold, before))
        noop = c == 0 or (fold and c == 1)
        assert out == {"snapshots_removed": 0 if noop else (c - 1 if fold else c), "rows_released": rows0 - counts(tr)[0],
                       "keys_forgotten": counts(base)[1] - counts(tr)[1], "rows": counts(tr)[0]}, (before, out)
        assert hist.stats()["rows_trimmed"] == rows0 - counts(tr)[0]
        if fold:
            assert out["keys_forgotten"] == 0
        task.agg.close()
        hist.close()


@pytest.mark.parametrize("full", [False, True], ids=["deltas", "whole"])
@pytest.mark.parametrize("fields", [FIVE, ["Protocol"]], ids=LAYOUT_IDS)
def test_trim_record_trim(gpu, oracle, fields, full):
    """A chain on one history: four snapshots, fold the first two, two more snapshots, fold again
    past the reset, then drop up to the last snapshot, then clear and start anew."""
    base = truth_of(oracle, fields, full)
    head = subset(base, [i for i, t in enumerate(base.ts) if t <= TS[3]])
    tail = subset(base, [i for i, t in enumerate(base.ts) if t > TS[3]])
    task, hist = build(fields, full, last=4)
    hist.trim(TS[1] + 1)
    tr, times = trimmed_truth(head, TS[:4], TS[1] + 1, True)
    check(hist, tr, times, fields, "first trim")
    build(fields, full, first=4, task=task)
    tr, times = joined(tr, tail), times + TS[4:]
    check(hist, tr, times, fields, "two more")
    released = hist.stats()["rows_trimmed"]
    out = hist.trim(TS[4])
    tr, times = trimmed_truth(tr, times, TS[4], True)
    check(hist, tr, times, fields, "second trim")
    released += out["rows_released"]
    out = hist.trim(TS[5], fold=False)
    tr, times = trimmed_truth(tr, times, TS[5], False)
    assert times == [TS[5]] and out["snapshots_removed"] == 2
    check(hist, tr, times, fields, "drop")
    released += out["rows_released"]
    assert hist.stats()["rows_trimmed"] == released
    out = hist.clear()
    assert out["rows"] == 0 and out["keys_forgotten"] == counts(tr)[1]
    check(hist, HistoryTruth(fields), [], fields, "cleared")
    assert hist.stats()["row_capacity"] == 0 and hist.stats()["index_slots"] == 64  # the memory is returned
    # timestamps start anew, and every key is new again
    t, ipver, ts = stream()
    task.process_packets(batch_of(t, ipver, ts, interval(0)))
    n, new = task.record(TS[0], full=True)
    assert n == new == hist.stats()["keys"] > 0 and hist.times() == [TS[0]]
    task.agg.close()
    hist.close()


# --- 2. fold keeps the present; drop forgets ---
def test_fold_keeps_the_present_and_drop_forgets(gpu, oracle):
    fields = ["Protocol", "SrcIP"]
    base = truth_of(oracle, fields, False)
    for before in (TS[1], TS[3] + 1, TS[5] + 1):  # c = 1 (a no-op), past the reset, down to one snapshot
        task, hist = build(fields, False)
        c = expired(TS, before)
        keep = [T for T in query_times() if T is None or T >= TS[c - 1]]
        pre = {T: answers(hist, fields, T) for T in keep}
        out = hist.trim(before, fold=True)
        assert out["snapshots_removed"] == c - 1 and out["keys_forgotten"] == 0
        assert (out["rows_released"] > 0) == (c > 1)
        for T in keep:
            assert answers(hist, fields, T) == pre[T], (before, T)
        for T in query_times():
            if T is not None and T < TS[c - 1] and c > 1:
                assert [len(a) for a in hist.snapshot_arrays(end_time=T)] == [0] * 5, (before, T)
        task.agg.close()
        hist.close()
    # drop of snapshot 0: the protocol-47 flows, seen only there, are forgotten ...
    task, hist = build(fields, False)
    p47 = {k for k in base.key if k.split("-")[0] == "47"}
    assert p47 and all(t == TS[0] for t, k in zip(base.ts, base.key) if k in p47)
    f47 = [to_filter({"Protocol": 47})]
    assert hist.aggregate(f47)[0].flows == len(p47)
    keys0 = hist.stats()["keys"]
    out = hist.trim(TS[1], fold=False)
    only0 = counts(base)[1] - counts(trimmed_truth(base, TS, TS[1], False)[0])[1]
    assert out["keys_forgotten"] == only0 >= len(p47) and hist.stats()["keys"] == keys0 - only0
    s = hist.aggregate(f47)[0]
    assert (s.flows, s.packets, s.max_packets, s.first_ns) == (0, 0, 0, 0)
    # ... and recorded again they are new keys
    t, ipver, ts = stream()
    task.process_packets(batch_of(t, ipver, ts, [5, 900]))
    assert task.record(TS[5] + 10) == (len(p47), len(p47))
    assert hist.aggregate(f47)[0].flows == len(p47) and hist.stats()["keys"] == keys0 - only0 + len(p47)
    task.agg.close()
    hist.close()


# --- 3. edges of the move ---
def check_log_trim(hist, c, fold, before, what):
    """A trim against the kept set computed with numpy on the exported log: the trimmed log is
    the kept rows in order, renumbered."""
    log = hist.export_log()
    kept, written = log_model(log[5], log[0], c, fold)
    keys_before = len(np.unique(log[0], axis=0)) if len(log[0]) else 0
    out = hist.trim(before, fold=fold)
    got = hist.export_log()
    for name, a, b in zip(LOG[:5], got, log):
        assert np.array_equal(a, b[kept]), (what, name)
    assert np.array_equal(got[5].astype(np.int64), written), what
    noop = c == 0 or (fold and c == 1)
    times = list(log[6]) if noop else ([log[6][c - 1]] if fold else []) + list(log[6][c:])
    assert list(got[6]) == times and hist.times() == [int(x) for x in times], what
    keys_after = len(np.unique(got[0], axis=0)) if len(got[0]) else 0
    assert out == {"snapshots_removed": len(log[6]) - len(times), "rows_released": int((~kept).sum()),
                   "keys_forgotten": keys_before - keys_after, "rows": int(kept.sum())}, (what, out)
    st = hist.stats()
    assert (st["snapshots"], st["rows"], st["keys"]) == (len(times), int(kept.sum()), keys_after), (what, st)
    return got


def small_history(rng):
    """Snapshots of 0, 1, 63, 64, 65, 257 and 0 new one-packet flows at times 0, 10, ..., then one
    that writes 65 known flows again (rows of snapshots 2 and 3 are superseded)."""
    task = new_task(["SrcIP"])
    hist = task.keep_history(max_rows=64, max_flows=32)
    total = 0
    for i, n in enumerate([0, 1, 63, 64, 65, 257, 0]):
        if n:
            task.process_packets(unique_batch(rng, total, n)[0])
        assert task.record(10 * i) == (n, n)
        total += n
    task.process_packets(unique_batch(rng, 60, 65)[0])
    assert task.record(70) == (65, 0)
    return task, hist


@pytest.mark.parametrize("fold", [False, True], ids=["drop", "fold"])
def test_trim_at_every_boundary_of_small_snapshots(gpu, fold):
    open_ = to_filter({})
    for c in range(9):
        task, hist = small_history(np.random.default_rng(4))
        before = 10 * c if c < 8 else 71
        want = hist.aggregate([open_])[0]
        check_log_trim(hist, c, fold, before, (fold, c))
        s = hist.aggregate([open_])[0]
        if fold or c == 0:  # the present is kept
            assert (s.flows, s.packets, s.bytes) == (want.flows, want.packets, want.bytes), c
        live = hist.snapshot_arrays()
        assert len(live[3]) == s.flows == len(set(map(bytes, live[0])))
        # the trimmed history goes on: a known flow supersedes, a new one is new
        task.process_packets(unique_batch(np.random.default_rng(5), 449, 2)[0])
        n, new = task.record(100)
        assert n == 2 and new == (1 if fold or c < 6 else 2), (c, n, new)
        assert hist.aggregate([open_])[0].flows == s.flows + new
        task.agg.close()
        hist.close()


def big_history(sizes, max_flows):
    """Three snapshots of sizes[i] new one-packet flows at times 0, 10, 20."""
    from go2netspectra_amd import ExactTask
    task = ExactTask("big", ["SrcIP"], batch_packets=1 << 18, max_flows=max_flows)
    hist = task.keep_history(max_rows=1024, max_flows=1024)
    rng = np.random.default_rng(9)
    by = first = 0
    for i, n in enumerate(sizes):
        b, nbytes = unique_batch(rng, first, n)
        task.process_packets(b)
        by += nbytes
        first += n
        assert task.record(10 * i) == (n, n)
    return task, hist, by


def fold_middle(hist, sizes, nbytes):
    """Fold at the middle snapshot: the base holds two snapshots' rows, nothing is superseded, so
    the log is what it was, renumbered.  Counts and sums with numpy."""
    open_ = to_filter({})
    total, two = sum(sizes), sizes[0] + sizes[1]
    s = hist.aggregate([open_])[0]
    assert (s.flows, s.packets, s.bytes, s.max_packets) == (total, total, nbytes, 1)
    log = hist.export_log()
    assert np.array_equal(log[5], np.repeat(np.array([0, 1, 2], np.uint32), sizes))
    out = hist.trim(11)
    assert out == {"snapshots_removed": 1, "rows_released": 0, "keys_forgotten": 0, "rows": total}
    assert hist.times() == [10, 20]
    assert hist.aggregate([open_], end_time=10)[0].flows == two and hist.aggregate([open_], end_time=9)[0].flows == 0
    got = hist.export_log()
    k, st, en, pk, by, wr, ts = got
    assert len(pk) == total and int(pk.sum()) == total and int(by.sum(dtype=np.uint64)) == nbytes
    assert np.array_equal(wr, np.repeat(np.array([0, 1], np.uint32), [two, sizes[2]]))
    for name, a, b in zip(LOG[:5], got, log):
        assert np.array_equal(a, b), name  # stably moved
    src = np.sort(k[:, 12:16].copy().view(">u4").ravel())
    assert np.array_equal(src, 0x0A000000 + np.arange(total, dtype=np.uint32))  # every flow once
    assert hist.aggregate([open_])[0] == s
    return got


def fold_all(hist, log, total, nbytes):
    """Fold everything into the base: the ranked prefix is the whole log."""
    out = hist.trim(21)
    assert out == {"snapshots_removed": 1, "rows_released": 0, "keys_forgotten": 0, "rows": total}
    k, st, en, pk, by, wr, ts = hist.export_log()
    assert list(ts) == [20] and not wr.any() and np.array_equal(k, log[0]) and np.array_equal(by, log[4])
    s = hist.aggregate([to_filter({})])[0]
    assert (s.flows, s.packets, s.bytes) == (total, total, nbytes)
    assert hist.stats()["keys"] == total and hist.stats()["rows"] == total


def test_trim_past_one_scan_bin(gpu):
    sizes = [23_334] * 3  # 70,002 rows: past the 65,536 rows of one scan bin
    total = sum(sizes)
    task, hist, nbytes = big_history(sizes, 1 << 17)
    log = fold_middle(hist, sizes, nbytes)
    fold_all(hist, log, total, nbytes)
    task.process_packets(unique_batch(np.random.default_rng(1), total, 5)[0])
    assert task.record(30) == (5, 5)
    out = hist.trim(30, fold=False)  # then drop the base
    assert out == {"snapshots_removed": 1, "rows_released": total, "keys_forgotten": total, "rows": 5}
    assert hist.stats()["keys"] == 5 and hist.aggregate([to_filter({})])[0].flows == 5
    task.agg.close()
    hist.close()


def test_trim_and_restore_past_one_scan_group(gpu):
    from go2netspectra_amd import ExactHistory
    sizes = [699_052, 699_052, 699_051]  # 2^21 + 3 rows: past the 256 * 256 * 32 rows of one scan group
    total, two = sum(sizes), sizes[0] + sizes[1]
    assert total == (1 << 21) + 3
    task, hist, nbytes = big_history(sizes, 1 << 22)
    log = fold_middle(hist, sizes, nbytes)
    # restored: the base snapshot's rows pass append_rows' resolve piece of 2^20
    other = ExactHistory(["SrcIP"], max_rows=1024, max_flows=1024)
    assert other.append_rows(*[a[:two] for a in log[:5]], 10) == (two, two)
    assert other.append_rows(*[a[two:] for a in log[:5]], 20) == (sizes[2], sizes[2])
    assert_same_log(other.export_log(), log, "restored")
    open_ = to_filter({})
    for T in (9, 10, 20, None):
        assert other.aggregate([open_], end_time=T) == hist.aggregate([open_], end_time=T), T
    for h in (hist, other):
        fold_all(h, log, total, nbytes)
    task.agg.close()
    hist.close()
    other.close()


# --- 4. export and import ---
def test_export_equals_the_truth_and_restores(gpu, oracle, tmp_path):
    from go2netspectra_amd import ExactHistory
    for fields in (FIVE, ["Protocol"]):
        for full in (True, False):
            base = truth_of(oracle, fields, full)
            task, hist = build(fields, full)
            for step, before in enumerate((None, TS[3] + 1)):
                if before is not None:
                    hist.trim(before)
                    base = trimmed_truth(base, TS, before, True)[0]
                log = hist.export_log()
                k, st, en, pk, by, wr, ts = log
                assert list(ts) == hist.times() and np.all(np.diff(wr.astype(np.int64)) >= 0)
                assert ts.dtype == np.int64 and wr.dtype == np.uint32 and k.shape == (len(pk), hist.key_bytes)
                # the truth's rows, snapshot by snapshot (within one the order is the view's)
                c = base.cols()
                for j, t in enumerate(ts):
                    got = sorted(rows_of([a[wr == j] for a in log[:5]]))
                    idx = np.nonzero(c["ts"] == t)[0]
                    want = sorted((c["kb"][i], base.start[i], base.end[i], base.pkts[i], base.bytes[i]) for i in idx)
                    assert got == want, (fields, full, step, j)
                # a file, restored into a fresh history: the same log, the same answers
                path = str(tmp_path / f"h{step}.npz")
                hist.save(path)
                other = ExactHistory(fields, max_rows=64, max_flows=32)
                other.append_rows(k[:1], st[:1], en[:1], pk[:1], by[:1], -(1 << 62))  # (what it held is cleared)
                other.restore(path)
                assert_same_log(other.export_log(), log, (fields, full, step))
                assert other.stats()["keys"] == hist.stats()["keys"]
                assert whole_answers(other, fields) == whole_answers(hist, fields), (fields, full, step)
                with pytest.raises(ValueError, match="'key_fields' differs"):
                    ExactHistory(["DstIP"], max_rows=64, max_flows=32).restore(path)
                other.close()
            task.agg.close()
            hist.close()


CM_AND_EXACT = """
aggregator:
  types: ["sketch", "exact"]
  sketch:
    tasks:
      - {name: cm_src, skt_type: 0, flow_fields: [SrcIP], element_fields: [DstIP, SrcPort, DstPort, Protocol],
         width: 4096, depth: 2, size_thereshold: 100000, count_thereshold: 50}
  exact:
    tasks:
      - {name: per_five_tuple, key_fields: [SrcIP, DstIP, SrcPort, DstPort, Protocol]}
"""


def test_task_and_manager_checkpoints_carry_the_history(gpu, tmp_path):
    import os
    from go2netspectra_amd import Manager, parse_config
    t, ipver, ts = stream()
    # ExactTask.save_history / restore_history
    task, hist = build(FIVE, False)
    hist.trim(TS[2])
    task.save_history(str(tmp_path / "task.history.npz"))
    fresh = new_task(FIVE, "fresh")
    fresh.keep_history(max_rows=64, max_flows=32)
    fresh.restore_history(str(tmp_path / "task.history.npz"))
    assert_same_log(fresh.history.export_log(), hist.export_log(), "task")
    assert whole_answers(fresh.history, FIVE) == whole_answers(hist, FIVE)
    for x in (task, fresh):
        x.agg.close()
        x.history.close()
    # Manager.checkpoint / restore: the exact task has a history, the sketch task none
    kw = dict(seeds=np.array([11, 22, 33, 44], np.uint32))
    first, second, bare = (Manager(parse_config(CM_AND_EXACT), **kw) for _ in range(3))
    assert list(first.keep_history(retain=None, max_rows=64, max_flows=32)) == ["per_five_tuple"]
    second.keep_history(max_rows=64, max_flows=32)
    for i in range(3):
        first.process(batch_of(t, ipver, ts, interval(i)))
        first.record(TS[i])
    paths = first.checkpoint(tmp_path / "ckpt")
    assert [os.path.basename(p) for p in paths] == ["cm_src.npz", "per_five_tuple.npz", "per_five_tuple.history.npz"]
    second.restore(tmp_path / "ckpt")
    h1, h2 = first.tasks()[1].history, second.tasks()[1].history
    assert_same_log(h2.export_log(), h1.export_log(), "manager")
    assert whole_answers(h2, FIVE) == whole_answers(h1, FIVE)
    # both go on: the restored one stores every restored flow again, and answers the same
    for m in (first, second):
        m.process(batch_of(t, ipver, ts, interval(3)))
        m.record(TS[3])
    assert h2.stats()["rows"] >= h1.stats()["rows"] and h2.stats()["keys"] == h1.stats()["keys"]
    assert [a for a, _ in whole_answers(h2, FIVE)] and \
        [x[1][:3] for x in whole_answers(h2, FIVE)] == [x[1][:3] for x in whole_answers(h1, FIVE)]
    # a manager without histories restores the same directory and ignores the history file
    bare.restore(tmp_path / "ckpt")
    assert getattr(bare.tasks()[1], "history", None) is None
    assert len(bare.checkpoint(tmp_path / "bare")) == 2
    for m in (first, second, bare):
        m.stop()


# --- 5. rejected calls change nothing ---
def test_rejected_calls_change_nothing(gpu):
    from go2netspectra_amd import _lib
    # (a history with room: a call rejected on the device may have grown the capacities, which are
    # part of stats(); nothing else of it may show)
    task = new_task(FIVE)
    task.keep_history(max_rows=1 << 13, max_flows=1 << 12)
    task, hist = build(FIVE, False, last=2, task=task)
    flt = [to_filter(f) for f in make_filters(FIVE, 20)]

    def state():
        return (hist.times(), hist.stats(), hist.aggregate(flt), hist.aggregate(flt, end_time=TS[0]),
                got_heavy(*hist.heavy_hitters(1)), rows_of(hist.snapshot_arrays()), [a.tobytes() for a in hist.export_log()])
    before = state()
    k, st, en, pk, by = (a.copy() for a in hist.snapshot_arrays())
    rows = lambda sel: [a[sel] for a in (k, st, en, pk, by)]
    assert len(pk) > 600
    for dist in (1, 300):  # the same key twice: neighbours, and more than a workgroup apart
        sel = np.arange(400)
        sel[dist] = 0
        e_arg(hist.append_rows, *rows(sel), TS[1] + 1)
        assert state() == before, dist
    zero = rows(np.arange(5))
    zero[3] = zero[3].copy()
    zero[3][4] = 0
    e_arg(hist.append_rows, *zero, TS[1] + 1)  # a row without packets
    for bad in (TS[1], TS[1] - 1, -(1 << 63)):
        e_arg(hist.append_rows, *rows(np.arange(5)), bad)  # a timestamp not after the last
        e_arg(hist.append_rows, *rows(np.arange(0)), bad)
    assert state() == before
    for fold in (2, -1):
        e_arg(hist.trim, TS[1] + 1, fold)
    assert hist._L.gns_ex_hist_trim(None, 0, 1, None) == _lib.GNS_E_ARG
    assert state() == before
    # the rejected rows are accepted once they are legal, the claimed keys are no leak
    assert hist.append_rows(*rows(np.arange(400)), TS[1] + 1) == (400, 0)
    assert hist.times() == [TS[0], TS[1], TS[1] + 1] and hist.stats()["keys"] == before[1]["keys"]
    assert hist.trim(TS[0] - 1) == {"snapshots_removed": 0, "rows_released": 0, "keys_forgotten": 0, "rows": hist.stats()["rows"]}
    task.agg.close()
    hist.close()


# --- 6. retention ---
@pytest.mark.parametrize("retain", [1, 2, 4])
def test_retention_keeps_a_window(gpu, oracle, retain):
    fields = ["Protocol", "SrcIP"]
    base = truth_of(oracle, fields, False)
    filters, engine_filters = filters_of(fields)
    task = new_task(fields)
    hist = task.keep_history(retain=retain, max_rows=256, max_flows=32)
    t, ipver, ts = stream()
    tr, times = HistoryTruth(fields), []
    for i in range(NSNAP):
        task.process_packets(batch_of(t, ipver, ts, interval(i)))
        task.record(TS[i])
        tr = joined(tr, subset(base, [j for j, x in enumerate(base.ts) if x == TS[i]]))
        times = times + [TS[i]]
        if len(times) > retain:
            tr, times = trimmed_truth(tr, times, times[-(retain - 1)] if retain > 1 else times[-1] + 1, True)
        assert hist.times() == times == TS[max(0, i + 1 - retain):i + 1]
        matches = [tr.matches(f) for f in filters]
        for T in (None, TS[i], times[0], times[0] - 1):
            assert_history_equals_truth(hist, tr, filters, engine_filters, matches, T, (retain, i, T))
        if retain == 1:  # exactly the current state
            st = hist.stats()
            assert st["rows"] == st["keys"] == len(tr.latest(None)) == counts(tr)[0]
        if i + 1 == RESET:
            task.reset()
    task.agg.close()
    hist.close()


def test_reader_thread_during_retained_records(gpu, oracle):
    fields = ["Protocol", "SrcIP"]
    base = truth_of(oracle, fields, False)
    filters, engine_filters = filters_of(fields)
    # the newest answer of every state the store passes through, from the truth alone: empty, then
    # per record the appended snapshot and the fold that follows it (min / max range over fewer rows)
    newest = lambda tr: ([tr.summary(f, None) for f in filters], tr.heavy(0, 0, 5, None), tr.rows_at(None))
    tr, times = HistoryTruth(fields), []
    want = [newest(tr)]
    for i in range(NSNAP):
        tr = joined(tr, subset(base, [j for j, x in enumerate(base.ts) if x == TS[i]]))
        times = times + [TS[i]]
        want.append(newest(tr))
        if len(times) > 2:
            tr, times = trimmed_truth(tr, times, times[-1], True)
            want.append(newest(tr))
    task = new_task(fields)
    hist = task.keep_history(retain=2, max_rows=256, max_flows=32)
    stop, errors, seen = threading.Event(), [], set()

    def reader():
        try:
            while True:
                last = stop.is_set()  # one full round after the writer is done
                got = (hist.aggregate(engine_filters), got_heavy(*hist.heavy_hitters(0, 0, 5)), set(rows_of(hist.snapshot_arrays())))
                # (three calls: a record may fall between them, so each is one of the snapshots' answers)
                for part, g in enumerate(got):
                    hit = [i for i, w in enumerate(want) if w[part] == g]
                    assert hit, part
                    seen.add(hit[-1])
                if last:
                    return
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    th = threading.Thread(target=reader, daemon=True)
    th.start()
    try:
        t, ipver, ts = stream()
        for i in range(NSNAP):
            task.process_packets(batch_of(t, ipver, ts, interval(i)))
            task.record(TS[i])
            assert len(hist.times()) <= 2
            if i + 1 == RESET:
                task.reset()
    finally:
        stop.set()
        th.join(timeout=60)
    assert not th.is_alive(), "the reader did not finish"
    assert not errors, errors
    assert len(want) - 1 in seen  # the last round saw the final state
    task.agg.close()
    hist.close()
