"""The history roll-up on the GPU (gns_ex_hist_rollup): the table a history holds as of a time,
re-keyed on the device, equals the reference's GROUP BY over the latest stored rows
(history_rollup_truth.py) -- every group, keys sorted, all five columns bit for bit.  The base
history is ~1,500 five-tuple flows of prefix_truth.prefix_stream (IPv4, IPv6 and IPv4-mapped
addresses, random signed timestamps) in six snapshots: two whole, a delta, a reset of the task, a
delta, an empty one, a delta.  GNS_EX_ROLLUP_PIECE=512 cuts its few thousand log rows into
pieces, so groups cross pieces and snapshots and some piece holds no live row."""
import numpy as np
import pytest

from exact_query_truth import FIVE, batch_of
from history_rollup_truth import RowLog, combine, latest_arrays, rollup_truth
from history_truth import HistoryTruth
from prefix_truth import prefix_stream
from test_exact_history_gpu import feed_oracle, rows_of

pytestmark = pytest.mark.gpu

NFLOWS = 1500
TS = [-5_000_000_000, -7, -5, 0, 3, 1 << 50]
CUTS = [(0, 9_000), (9_000, 14_000), (14_000, 19_000), (19_000, 24_000), None, (24_000, 30_000)]
FULL = [True, True, False, False, False, False]
RESET = 3  # the task is reset after this many snapshots
I64 = np.iinfo(np.int64)
M64 = (1 << 64) - 1
LAYOUTS = [["SrcIP"], ["DstIP", "DstPort"], ["SrcPort", "Protocol"], ["Protocol"], FIVE,
           ["Protocol", "DstPort", "DstIP", "SrcPort", "SrcIP"]]
IDS = lambda f: "-".join(f) if isinstance(f, list) else str(f)


@pytest.fixture(autouse=True)
def piece(monkeypatch):
    monkeypatch.setenv("GNS_EX_ROLLUP_PIECE", "512")


def new_task(fields=FIVE, name="h"):
    from go2netspectra_amd import ExactTask
    return ExactTask(name, fields, batch_packets=4096, max_flows=1 << 12)


def new_agg(fields, **kw):
    from go2netspectra_amd import ExactAggregator
    kw.setdefault("max_flows", 64)  # grows under the roll-up
    return ExactAggregator(fields, batch_packets=4096, **kw)


def sorted_rows(agg):
    rows = rows_of(agg.snapshot_arrays())
    assert len({r[0] for r in rows}) == len(rows), "a key is listed twice"
    return sorted(rows)


def query_times():
    return [TS[0] - 10] + TS + [TS[1] + 1, None]  # before the first, every snapshot, between -7 and -5, the newest


def record_base(task, tr, oracle, snaps=range(6)):
    """Snapshots ``snaps`` of the base stream into the task's history and into the truth."""
    t, ipver, ts = prefix_stream(NFLOWS)
    for i in snaps:
        if CUTS[i] is not None:
            sel = slice(*CUTS[i])
            task.process_packets(batch_of(t, ipver, ts, sel))
            feed_oracle(tr.oracle, t, ipver, ts, sel)
        out = task.record(TS[i], full=FULL[i])
        if CUTS[i] is None:
            assert out == (0, 0)
        tr.record(TS[i], tr.oracle.export())
        if i + 1 == RESET:
            task.reset()
            tr.oracle = oracle.Exact(FIVE)


@pytest.fixture(scope="module")
def base(gpu, oracle):
    task = new_task()
    hist = task.keep_history(max_rows=256, max_flows=32)
    tr = HistoryTruth(FIVE)
    tr.oracle = oracle.Exact(FIVE)
    record_base(task, tr, oracle)
    # the shape the cases below rely on
    st = hist.stats()
    assert st["snapshots"] == 6 and 3_000 <= st["rows"] <= 6_000, st
    old, new = tr.export_at(TS[2]), tr.export_at(None)
    assert any(new[k][2] < old[k][2] for k in old if new[k] != old[k]), "no flow returned with a smaller count"
    assert any(new[k] == old[k] for k in old) and len(new) >= len(old)
    # every row of snapshot 0 is superseded by the whole snapshot 1: the first piece of 512 log rows holds no live row
    written = hist.export_log()[5]
    assert (written[:512] == 0).all() and len(tr.latest(TS[0])) >= 512
    yield task, hist, tr
    task.agg.close()
    hist.close()


def check(got_agg, want, what):
    got = sorted_rows(got_agg)
    assert len(got) == len(want), (what, len(got), len(want))
    for g, w in zip(got, want):
        assert g == w, (what, g, w)


# --- 1. the base case: every layout at every time ---
@pytest.mark.parametrize("fields", LAYOUTS, ids=IDS)
def test_rollup_equals_the_group_by_at_every_time(base, fields):
    _, hist, tr = base
    groups = set()
    for T in query_times():
        want = rollup_truth(tr, T, fields)
        dst = new_agg(fields)
        out = dst.rollup_from_history(hist, end_time=T)
        assert out == (len(tr.latest(T)), len(want)), (fields, T, out)
        check(dst, want, (fields, T))
        dst.close()
        groups.add(len(want))
    assert 0 in groups and len(groups) >= 2
    if fields == ["Protocol"]:
        assert max(groups) < 8  # few groups: every wave reduces, the rest meets in the LDS table
    if len(fields) == 5:
        assert max(groups) == len(tr.latest(None))  # every row its own group


def test_empty_before_the_first_snapshot_and_the_empty_snapshot(base):
    _, hist, tr = base
    dst = new_agg(["SrcIP"])
    v = dst.view()
    assert dst.rollup_from_history(hist, end_time=TS[0] - 1) == (0, 0)
    assert sorted_rows(dst) == [] and v.refresh() == 0  # no position was spent
    a, b = hist.rollup(["SrcIP"], end_time=TS[3]), hist.rollup(["SrcIP"], end_time=TS[4])  # TS[4]: the empty snapshot
    assert sorted_rows(a) == sorted_rows(b) == rollup_truth(tr, TS[3], ["SrcIP"])
    for h in (v, dst, a, b):
        h.close()


# --- 2. prefixes ---
PREFIXES = [(["SrcIP"], {"SrcIP": p}) for p in ((24, 64), (16, 48), (8, 32), (0, 0), (32, 128))] + [
    (["SrcIP", "DstIP"], {"SrcIP": (24, 64), "DstIP": (16, 48)}),
    (["Protocol", "SrcIP"], {"SrcIP": (17, 65), "DstIP": (3, 3)}),  # unaligned; the prefix of an absent field is ignored
]


@pytest.mark.parametrize("fields,prefix", PREFIXES, ids=IDS)
def test_prefix_rollup(base, fields, prefix):
    _, hist, tr = base
    for T in (TS[2], TS[3], None):
        want = rollup_truth(tr, T, fields, prefix)
        plain = rollup_truth(tr, T, fields)
        dst = hist.rollup(fields, prefix=prefix, end_time=T)
        check(dst, want, (fields, prefix, T))
        if prefix == {"SrcIP": (32, 128)}:  # the full prefix is the unmasked call, bit for bit
            assert want == plain
            other = hist.rollup(fields, end_time=T)
            for x, y in zip(dst.snapshot_arrays(), other.snapshot_arrays()):
                assert x.tobytes() == y.tobytes()
            other.close()
        elif prefix["SrcIP"] == (0, 0):
            assert len(want) == 2  # one group per address class
        else:
            assert 1 < len(want) < len(plain)
        dst.close()


# --- 3. signed times, wraps: rows given to append_rows ---
def ip4(a, b, c, d):
    return bytes(10) + b"\xff\xff" + bytes([a, b, c, d])


def signed_log():
    """(SrcIP, SrcPort) rows in three snapshots of 700 / 500 / 300 rows: 8 large groups by SrcIP
    spread over all pieces, 40 small ones; group 0 has only positive starts, group 1 only
    negative ends, group 2 both int64 extremes, the others random times of both signs."""
    fields = ["SrcIP", "SrcPort"]
    rng = np.random.default_rng(23)
    log, port, log_groups = RowLog(fields), 0, {}
    for si, n in enumerate((700, 500, 300)):
        keys, st, en = [], [], []
        for i in range(n):
            g = int(rng.integers(0, 8)) if rng.random() < 0.85 else 8 + int(rng.integers(0, 40))
            if si and rng.random() < 0.3:  # supersede a row of an earlier snapshot
                p = int(rng.integers(0, port))
                g = log_groups[p]
            else:
                p = port
                port += 1
            if any(k[1] == p for k in keys):
                continue
            keys.append((g, p))
            log_groups[p] = g
            s, e = int(rng.integers(-(1 << 62), 1 << 62)), int(rng.integers(-(1 << 62), 1 << 62))
            if g == 0:
                s = abs(s) + 5
            if g == 1:
                e = -abs(e) - 5
            if g == 2 and i % 7 == 0:
                s, e = (I64.max, I64.min) if i % 2 else (I64.min, I64.max)
            st.append(s)
            en.append(e)
        kb = np.frombuffer(b"".join(ip4(10, 0, g >> 4, g & 15) + p.to_bytes(2, "big") for g, p in keys), np.uint8)
        m = len(keys)
        log.append(10 * (si + 1), kb.reshape(m, 18), st, en, rng.integers(1, 1 << 40, m).astype(np.uint64),
                   rng.integers(1 << 62, 1 << 64, m, dtype=np.uint64))
    return log



def history_of(log):
    from go2netspectra_amd import ExactHistory
    hist = ExactHistory(log.fields, max_rows=256, max_flows=32)
    for ts, keys, st, en, pk, by in log.snaps:
        assert hist.append_rows(keys, st, en, pk, by, ts)[0] == len(keys)
    return hist


def test_signed_times_are_min_and_max(gpu):
    log = signed_log()
    hist = history_of(log)
    assert hist.stats()["rows"] > 1024  # three pieces and more
    for T in (10, 20, None):
        want = log.rollup(T, ["SrcIP"])
        by_ip = {r[0]: r for r in want}
        assert by_ip[ip4(10, 0, 0, 0)][1] > 0, "group 0: the true min start is positive"
        assert by_ip[ip4(10, 0, 0, 1)][2] < 0, "group 1: the true max end is negative"
        if T is None:
            assert by_ip[ip4(10, 0, 0, 2)][1:3] == (I64.min, I64.max)
        assert any(r[1] < 0 < r[2] for r in want) and any(r[4] < (1 << 62) for r in want)  # mixed signs; bytes wrapped
        for fields in (["SrcIP"], ["SrcPort", "SrcIP"], ["SrcIP", "SrcPort"]):
            dst = hist.rollup(fields, end_time=T)
            check(dst, log.rollup(T, fields), (fields, T))
            dst.close()
        masked = hist.rollup(["SrcIP"], prefix={"SrcIP": 28}, end_time=T)
        check(masked, log.rollup(T, ["SrcIP"], {"SrcIP": 28}), ("/28", T))
        masked.close()
    hist.close()


def test_groups_that_wrap(gpu):
    fields = ["SrcIP", "SrcPort"]
    log = RowLog(fields)
    keys = lambda rows: np.frombuffer(b"".join(ip4(10, 0, 0, g) + p.to_bytes(2, "big") for g, p in rows), np.uint8).reshape(-1, 18)
    # group 1: 2^63 + 2^63 packets, it vanishes; group 2: bytes wrap to 5; group 3: 2^63 + 2^63 + 1 packets over two snapshots
    log.append(1, keys([(1, 1), (2, 1), (3, 1), (3, 2)]), [4, -4, 1, 2], [5, -5, 1, 2],
               np.array([1 << 63, 7, 1 << 63, 1 << 63], np.uint64), np.array([1, M64, 1, 1], np.uint64))
    log.append(2, keys([(1, 2), (2, 2), (3, 3)]), [-9, 8, 3], [9, -8, 3], np.array([1 << 63, 1, 1], np.uint64),
               np.array([1, 6, 1], np.uint64))
    hist = history_of(log)
    want = log.rollup(None, ["SrcIP"])
    assert want == [(ip4(10, 0, 0, 2), -4, -5, 8, 5), (ip4(10, 0, 0, 3), 1, 3, 1, 3)]
    dst = new_agg(["SrcIP"])
    assert dst.rollup_from_history(hist) == (7, 3)  # the vanished group claimed a slot and holds no flow
    check(dst, want, "wrap")
    at1 = hist.rollup(["SrcIP"], end_time=1)
    check(at1, log.rollup(1, ["SrcIP"]), "wrap at 1")
    assert len(sorted_rows(at1)) == 2  # 10.0.0.1 with 2^63 packets, 10.0.0.2; 10.0.0.3 sums to 0
    for h in (dst, at1, hist):
        h.close()


# --- 4. a destination that is not empty ---
def test_two_histories_into_one_handle_in_both_orders(base, oracle):
    _, hist, tr = base
    # a second history of the same layout: other packets of the stream, overlapping keys
    t, ipver, ts = prefix_stream(NFLOWS)
    task2, tr2 = new_task(name="h2"), HistoryTruth(FIVE)
    h2 = task2.keep_history(max_rows=256, max_flows=32)
    o2 = oracle.Exact(FIVE)
    for i, sel in enumerate((slice(30_000, 36_000), slice(36_000, 40_000))):
        task2.process_packets(batch_of(t, ipver, ts, sel))
        feed_oracle(o2, t, ipver, ts, sel)
        task2.record(100 + i)
        tr2.record(100 + i, o2.export())
    for fields, prefix in ((["SrcIP"], None), (["DstIP", "DstPort"], {"DstIP": (24, 64)}), (FIVE, None)):
        a, b = rollup_truth(tr, TS[3], fields, prefix), rollup_truth(tr2, None, fields, prefix)
        want = combine(a, b)
        assert len(want) < len(a) + len(b), "no key in both"
        for first in (0, 1):
            dst = new_agg(fields)
            pairs = [(hist, TS[3]), (h2, None)]
            n1 = dst.rollup_from_history(*pairs[first], prefix=prefix)
            n2 = dst.rollup_from_history(*pairs[1 - first], prefix=prefix)
            assert n1[1] == len((a, b)[first]) and n1[1] + n2[1] == len(want) and n2[1] < len((a, b)[1 - first])
            check(dst, want, (fields, prefix, first))
            dst.close()
    task2.agg.close()
    h2.close()


def test_a_destination_that_ingested_packets(base, oracle):
    _, hist, tr = base
    fields = ["SrcIP"]
    t, ipver, ts = prefix_stream(NFLOWS)
    before, after = slice(40_000, 43_000), slice(43_000, 46_000)
    dst = new_agg(fields)
    view = dst.view()
    dst.insert_tuples(batch_of(t, ipver, ts, before))
    dst.flush()
    o = oracle.Exact(fields)
    feed_oracle(o, t, ipver, ts, before)
    from exact_query_truth import key_bytes_of
    as_rows = lambda exp: sorted((key_bytes_of(k, fields),) + tuple(v) for k, v in exp.items())
    rows0 = as_rows(o.export())
    assert sorted_rows(dst) == rows0
    cursor = view.refresh()
    assert cursor == 3_000
    rolled = rollup_truth(tr, None, fields)
    n, new = dst.rollup_from_history(hist)
    want = combine(rows0, rolled)
    assert n == len(tr.latest(None)) and new == len(want) - len(rows0) and 0 < new < len(rolled)
    check(dst, want, "counts add, times are min / max")
    # a view cursor taken before the call selects exactly the groups
    c2 = view.refresh(cursor)
    assert c2 == cursor + hist.stats()["rows"]
    assert sorted(rows_of(view.snapshot_arrays())) == [r for r in want if r[0] in {x[0] for x in rolled}]
    # packets inserted afterwards land after the rolled-up rows: the ingest's stream-order rule gives a
    # flow the end of its last packet whatever the roll-up stored, keeps the start of a flow that existed
    dst.insert_tuples(batch_of(t, ipver, ts, after))
    dst.flush()
    o2 = oracle.Exact(fields)
    feed_oracle(o2, t, ipver, ts, after)
    late = {r[0]: r[1:] for r in as_rows(o2.export())}
    final = {r[0]: r[1:] for r in want}
    for k, (st, en, pk, by) in late.items():
        if k in final:
            s0, _, p0, b0 = final[k]
            final[k] = (s0, en, (p0 + pk) & M64, (b0 + by) & M64)
        else:
            final[k] = (st, en, pk, by)
    check(dst, sorted((k,) + v for k, v in final.items()), "packets after the roll-up")
    assert view.refresh(c2) == c2 + 3_000
    assert {r[0] for r in rows_of(view.snapshot_arrays())} == set(late)
    view.close()
    dst.close()


# --- 5. the destination is a full handle ---
def test_table_as_of_a_time_is_the_snapshot(base):
    _, hist, tr = base
    for T in (TS[0], TS[2], TS[3], None):
        tab = hist.table(end_time=T, max_flows=64)
        rows = sorted(rows_of(hist.snapshot_arrays(end_time=T)))
        assert sorted_rows(tab) == rows and len(rows) == len(tr.latest(T))
        for fields, prefix in ((["SrcIP"], None), (["DstIP", "Protocol"], {"DstIP": (16, 48)})):
            chained = tab.rollup(fields, prefix=prefix, max_flows=64)
            direct = hist.rollup(fields, prefix=prefix, end_time=T, max_flows=64)
            counts = lambda a: [(r[0], r[3], r[4]) for r in sorted_rows(a)]
            assert counts(chained) == counts(direct) == [(r[0], r[3], r[4]) for r in rollup_truth(tr, T, fields, prefix)]
            chained.close()
            direct.close()
        tab.close()


def test_spread_as_of_a_time(base):
    from test_prefix_rollup_gpu import snap, spread_truth
    task, hist, tr = base
    for T in (TS[2], None):
        keys = latest_arrays(tr, T)[0]
        for flow, elem, fpx in ((["SrcIP"], ["DstIP"], None), (["SrcIP"], ["SrcIP"], {"SrcIP": (24, 48)})):
            want, _ = spread_truth(keys, FIVE, flow, elem, fpx, None)
            assert 1 < len(want) and max(want.values()) > 1
            # (a task's end_time=None is its live table: the newest snapshot is asked for by its time)
            for src, at in ((hist, T), (task, TS[5] if T is None else T)):
                sp = src.spread(flow, elem, flow_prefix=fpx, end_time=at, max_flows=1 << 12, max_pairs=1 << 13)
                assert snap(sp) == want, (flow, elem, fpx, T)
                sp.close()


@pytest.mark.parametrize("metric", [0, 1], ids=["packets", "bytes"])
def test_hierarchical_heavy_hitters_as_of_a_time(base, metric):
    from go2netspectra_amd import discount_heavy_prefixes
    from test_prefix_rollup_gpu import brute_hhh
    task, hist, tr = base
    levels = [(32, 128), (24, 64), (16, 48), (8, 32)]
    for T in (TS[2], None):
        per_level = [rollup_truth(tr, T, ["SrcIP"], {"SrcIP": lv}) for lv in levels]
        value = lambda r: r[4] if metric else r[3]
        leaves = {r[0]: value(r) for r in per_level[0]}
        assert sum(leaves.values()) < 1 << 64
        threshold = sum(leaves.values()) // 40
        lists = []
        for rows in per_level:
            heavy = sorted(((r[0], value(r)) for r in rows if value(r) >= threshold), key=lambda r: (-r[1], r[0]))
            lists.append((np.frombuffer(b"".join(k for k, _ in heavy), np.uint8).reshape(-1, 16), [v for _, v in heavy]))
        want = discount_heavy_prefixes(lists, levels, threshold)
        assert want == brute_hhh(leaves, levels, threshold)
        assert want[0] and any(want[li] for li in (1, 2, 3))
        assert hist.hierarchical_heavy_hitters("SrcIP", levels, metric, threshold, end_time=T) == want
        if T is not None:
            assert task.hierarchical_heavy_hitters("SrcIP", levels, metric, threshold, end_time=T) == want


# --- 6. lifecycle: trim, save / restore ---
LIFE = [(["SrcIP"], None), (["DstIP", "DstPort"], None), (["SrcIP", "DstIP"], {"SrcIP": (24, 64), "DstIP": (16, 48)})]


def answers(hist, T):
    out = []
    for fields, prefix in LIFE:
        a = hist.rollup(fields, prefix=prefix, end_time=T, max_flows=64)
        out.append(sorted_rows(a))
        a.close()
    return out


def rebuilt(oracle, snaps=range(6)):
    task = new_task()
    hist = task.keep_history(max_rows=256, max_flows=32)
    tr = HistoryTruth(FIVE)
    tr.oracle = oracle.Exact(FIVE)
    record_base(task, tr, oracle, snaps)
    return task, hist


def test_fold_keeps_every_answer_from_the_base_time_on(base, oracle):
    _, hist0, tr = base
    task, hist = rebuilt(oracle)
    pre = {T: answers(hist0, T) for T in query_times()}
    assert pre[None] == [rollup_truth(tr, None, f, p) for f, p in LIFE]
    out = hist.trim(TS[3], fold=True)  # snapshots 0..2 fold into one base under TS[2]
    assert out["snapshots_removed"] == 2 and out["rows_released"] > 0
    for T in query_times():
        if T is None or T >= TS[2]:
            assert answers(hist, T) == pre[T], T
        else:
            assert answers(hist, T) == [[], [], []], T
    task.agg.close()
    hist.close()


def test_drop_equals_a_history_of_the_later_snapshots(base, oracle):
    from go2netspectra_amd import ExactHistory
    _, hist0, _ = base
    task, hist = rebuilt(oracle)
    log = hist0.export_log()
    keys, st, en, pk, by, written, times = log
    assert list(times) == TS
    hist.trim(TS[3], fold=False)
    later = ExactHistory(FIVE, max_rows=256, max_flows=32)
    for s in range(3, 6):
        m = written == s
        later.append_rows(keys[m], st[m], en[m], pk[m], by[m], TS[s])
    for T in query_times():
        got = answers(hist, T)
        assert got == answers(later, T), T
        if T is not None and T < TS[3]:
            assert got == [[], [], []]
    assert answers(hist, None) != answers(hist0, None)  # the flows seen only before the reset are gone
    for h in (task.agg, hist, later):
        h.close()


def test_save_and_restore_answer_the_same(base, tmp_path):
    from go2netspectra_amd import ExactHistory
    _, hist, _ = base
    hist.save(tmp_path / "h.ckpt")
    back = ExactHistory(FIVE, max_rows=16, max_flows=16)
    back.restore(tmp_path / "h.ckpt")
    for T in query_times():
        assert answers(back, T) == answers(hist, T), T
    back.close()


# --- 7. the task surface ---
def test_task_rollup_and_spread_as_of_a_time(base, oracle):
    from go2netspectra_amd import ExactTask
    from test_prefix_rollup_gpu import snap
    task, hist, tr = base
    for T in (TS[1], TS[4]):
        sub = task.rollup("nets", ["SrcIP"], prefix={"SrcIP": (24, 64)}, end_time=T, max_flows=64)
        assert isinstance(sub, ExactTask) and sub.name() == "nets"
        check(sub.agg, rollup_truth(tr, T, ["SrcIP"], {"SrcIP": (24, 64)}), ("task", T))
        sub.agg.close()
        a = task.spread(["SrcIP"], ["DstPort"], end_time=T, max_flows=1 << 12, max_pairs=1 << 13)
        b = hist.spread(["SrcIP"], ["DstPort"], end_time=T, max_flows=1 << 12, max_pairs=1 << 13)
        assert snap(a) == snap(b) and len(snap(a)) > 1
        a.close()
        b.close()
    # end_time=None is the live table, as before
    live = task.rollup("live", ["SrcIP"], max_flows=64)
    direct = task.agg.rollup(["SrcIP"], max_flows=64)
    assert sorted_rows(live.agg) == sorted_rows(direct)
    assert sorted_rows(live.agg) != sorted_rows(hist.rollup(["SrcIP"]))  # (the history also holds the flows before the reset)
    live.agg.close()
    direct.close()
    bare = new_task(["SrcIP"], name="bare")
    for call in (lambda: bare.rollup("r", ["SrcIP"], end_time=5), lambda: bare.spread(["SrcIP"], ["SrcIP"], end_time=5),
                 lambda: bare.hierarchical_heavy_hitters("SrcIP", [(32, 128)], 0, 1, end_time=5)):
        with pytest.raises(ValueError, match="end_time"):
            call()
    bare.agg.close()


# --- 8. errors ---
def test_errors_come_before_any_device_work(base):
    import ctypes as ct
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
    call = L.gns_ex_hist_rollup
    # a field the history lacks, named
    narrow = ExactHistory(["SrcIP"], max_rows=16, max_flows=16)
    assert call(dst._h, narrow._h, None, None, out) == _lib.GNS_E_ARG and b"DstPort" in L.gns_last_error()
    with pytest.raises(ValueError, match="DstPort"):
        dst.rollup_from_history(narrow)
    with pytest.raises(ValueError, match="DstPort"):
        narrow.rollup(["SrcIP", "DstPort"])
    # a prefix out of range
    for bad in ((33, 128, 32, 128), (32, 129, 32, 128), (32, 128, 33, 128), (32, 128, 32, 129)):
        px = _lib.Prefix(*bad)
        assert call(dst._h, hist._h, None, ct.byref(px), out) == _lib.GNS_E_ARG and b"prefix" in L.gns_last_error()
    for bad in ({"SrcIP": 33}, {"SrcIP": (8, 129)}):
        with pytest.raises(ValueError):
            dst.rollup_from_history(hist, prefix=bad)
    # null handles
    assert call(None, hist._h, None, None, out) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()
    assert call(dst._h, None, None, None, out) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()
    # another device index, through the argument check alone (one device suffices)
    other = ExactHistory.__new__(ExactHistory)
    other._h, other._L, other.key_fields, other.key_bytes, other.device = hist._h, hist._L, FIVE, 37, hist.device + 1
    with pytest.raises(ValueError, match="device"):
        dst.rollup_from_history(other)
    other._h = None  # (not this object's to destroy)
    with pytest.raises(ValueError):
        dst.rollup_from_history(hist, end_time=1 << 63)
    assert [a.tobytes() for a in dst.snapshot_arrays()] == snap0 and (out[0], out[1]) == (3, 4)
    assert view.refresh() == 2_000  # no positions were spent
    # ... and the handle still takes the roll-up
    n, new = dst.rollup_from_history(hist, end_time=TS[0])
    assert n == hist.stats()["rows"] - sum(1 for w in hist.export_log()[5] if w > 0) and new > 0
    for h in (view, dst, narrow):
        h.close()
