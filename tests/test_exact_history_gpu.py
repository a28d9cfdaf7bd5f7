"""The exact history on the GPU (gns_ex_hist_*): every answer as of a time equals the
reference's SQL over the stored snapshot rows (history_truth.py), bit for bit.  Streams are
tricky_stream's: v4, v6, mapped and aliased addresses, wire lengths near 2^32, random signed
timestamps; at most 20K packets over at most 3K flows."""
import ipaddress
import threading

import numpy as np
import pytest

from exact_query_truth import FIVE, batch_of, got_heavy, packet_value, to_filter, tricky_stream
from history_truth import HistoryTruth

pytestmark = pytest.mark.gpu

LAYOUTS = [FIVE, ["SrcIP"], ["Protocol", "SrcIP"], ["Protocol"]]  # (unaligned IP; K = 1: every snapshot supersedes every row)
LAYOUT_IDS = lambda f: "-".join(f)
NPKT, NFLOWS, NSNAP = 18_000, 2_500, 6
TS = [-5_000_000_000, -7, -5, 0, 3, 1 << 50]  # snapshot times: negative, adjacent to each other's +-1, large
NAMES = ("keys", "start", "end", "packets", "bytes")
_CACHE = {}


def stream():
    """The stream of every test below, cut into NSNAP intervals.  Two packets of interval 0 carry
    protocol 47, which no other packet has: a flow seen only in snapshot 0 under every layout."""
    if "s" not in _CACHE:
        t, ipver, ts = tricky_stream(11, NPKT, NFLOWS)
        t["proto"][[5, 900]] = 47
        _CACHE["s"] = (t, ipver, ts)
    return _CACHE["s"]


def interval(i):
    n = NPKT // NSNAP
    return slice(i * n, (i + 1) * n)


def new_task(fields, name="h"):
    from go2netspectra_amd import ExactTask
    return ExactTask(name, fields, batch_packets=4096, max_flows=1 << 12)


def feed_oracle(o, t, ipver, ts, sel):
    o.insert_tuples(t["src16"][sel], t["dst16"][sel], t["sport"][sel], t["dport"][sel], t["proto"][sel],
                    ipver[sel], t["length"][sel], ts[sel])


def ip_text(t, ipver, i, field):
    """The address of packet i as text, and whether it is a 4-byte net.IP."""
    slot = bytes(t["src16" if field == "SrcIP" else "dst16"][i])
    if ipver[i] == 4:
        return str(ipaddress.IPv4Address(slot[:4])), True
    return str(ipaddress.IPv6Address(slot)), False


def make_filters(fields, n=70):
    """n filters {field: value}: the open filter, equality on subsets of the layout's fields with
    values packets carry, IPs also as prefixes (/0, /8, /24 of an IPv4 address; /0, /64, /120 of an
    IPv6 one; the /120 of ::ffff:a.b.c.d, which is the IPv4 /24), and a field outside the layout."""
    t, ipver, _ = stream()
    rng = np.random.default_rng(len(fields) * 1000 + sum(map(len, fields)))
    out = [{}, {"Protocol": 99} if "Protocol" in fields else {"SrcIP": "255.255.255.254"}]  # everything, nothing
    absent = [f for f in FIVE if f not in fields]
    if absent:
        out.append({absent[0]: packet_value(t, ipver, 3, absent[0])})
        out.append({absent[0]: packet_value(t, ipver, 4, absent[0]), fields[0]: packet_value(t, ipver, 4, fields[0])})
    while len(out) < n:
        i = int(rng.integers(0, NPKT))
        k = int(rng.integers(1, len(fields) + 1))
        flt = {}
        for f in rng.choice(fields, k, replace=False):
            f = str(f)
            v = packet_value(t, ipver, i, f)
            if f in ("SrcIP", "DstIP") and rng.random() < 0.6:
                text, v4 = ip_text(t, ipver, i, f)
                c = int(rng.integers(0, 4))
                if v4:
                    v = [f"{text}/0", f"{text}/8", f"{text}/24", f"::ffff:{text}/120"][c]
                else:
                    v = [f"{text}/0", f"{text}/64", f"{text}/120", f"{text}/8"][c]
            flt[f] = v
        out.append(flt)
    return out


def query_times():
    out = [TS[0] - 10]
    for x in TS:
        out += [x - 1, x, x + 1]
    return sorted(set(out)) + [TS[-1] + (1 << 40), None]


def heavy_cases():
    return [(m, thr, lim) for m, mid in ((0, 3), (1, 1500)) for thr in (0, mid) for lim in (0, 1, 7)]


def cut(rows, thr, lim):
    rows = [r for r in rows if r[1] >= thr]
    return rows[:lim] if lim else rows


def rows_of(arrays):
    keys, st, en, pk, by = arrays
    return [(bytes(keys[i]), int(st[i]), int(en[i]), int(pk[i]), int(by[i])) for i in range(len(pk))]


def assert_same_arrays(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape, f"{what}: {name} {a.shape} vs {b.shape}"
        assert np.array_equal(a, b), f"{what}: {name} differs"


def e_arg(fn, *a):
    from go2netspectra_amd import GnsError, _lib
    with pytest.raises(GnsError) as e:
        fn(*a)
    assert e.value.code == _lib.GNS_E_ARG, e.value


def assert_history_equals_truth(hist, tr, filters, engine_filters, matches, T, what):
    got = hist.aggregate(engine_filters, end_time=T)
    for flt, m, g in zip(filters, matches, got):
        assert g == tr.summary(flt, T, match=m), (what, T, flt)
    for metric in (0, 1):
        full = tr.heavy(metric, 0, 0, T)
        for m2, thr, lim in heavy_cases():
            if m2 == metric:
                assert got_heavy(*hist.heavy_hitters(metric, thr, lim, end_time=T)) == cut(full, thr, lim), (what, T, metric, thr, lim)
    rows = rows_of(hist.snapshot_arrays(end_time=T))
    assert len(rows) == len(set(rows)) and set(rows) == tr.rows_at(T), (what, T)


def run_intervals(task, oracle, fields, tr, reset_after=3, full=False, first=0, last=NSNAP):
    """Feed intervals first..last-1 to the task and to the truth, recording each; the task is
    reset (and the oracle replaced) after interval ``reset_after``."""
    t, ipver, ts = stream()
    if not hasattr(tr, "oracle"):
        tr.oracle = oracle.Exact(fields)  # the period's table; replaced at a reset
    for i in range(first, last):
        task.process_packets(batch_of(t, ipver, ts, interval(i)))
        feed_oracle(tr.oracle, t, ipver, ts, interval(i))
        task.record(TS[i], full=full)
        tr.record(TS[i], tr.oracle.export())
        if i + 1 == reset_after:
            task.reset()
            tr.oracle = oracle.Exact(fields)


# --- 1. a history holding one whole view answers as that view ---
@pytest.mark.parametrize("fields", LAYOUTS, ids=LAYOUT_IDS)
def test_one_whole_view(gpu, fields):
    from go2netspectra_amd import ExactHistory, Summary
    t, ipver, ts = stream()
    task = new_task(fields)
    task.process_packets(batch_of(t, ipver, ts))
    view = task.view()
    view.refresh()
    hist = ExactHistory(fields, max_rows=256, max_flows=32)
    nrows = len(view.snapshot_arrays()[3])
    assert hist.append(view, 100) == (nrows, nrows)
    flt = [to_filter(f) for f in make_filters(fields)]
    want = view.aggregate(flt)
    assert any(s.flows > 1 for s in want) and any(s.flows == 0 for s in want) and want[0].flows == nrows
    for T in (None, 100, 101, 1 << 62):
        assert hist.aggregate(flt, end_time=T) == want, T
        for metric, thr, lim in heavy_cases():
            a, b = hist.heavy_hitters(metric, thr, lim, end_time=T), view.heavy_hitters(metric, thr, lim)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (T, metric, thr, lim)
        assert_same_arrays(hist.snapshot_arrays(end_time=T), view.snapshot_arrays(), f"snapshot at {T}")
    assert hist.aggregate(flt, end_time=99) == [Summary()] * len(flt)
    assert len(hist.heavy_hitters(0, end_time=99)[1]) == 0 and len(hist.snapshot_arrays(end_time=99)[3]) == 0
    assert hist.times() == [100]
    hist.close()
    view.close()
    task.agg.close()


# --- 2. six delta snapshots, a reset of the source after the third ---
@pytest.mark.parametrize("fields", LAYOUTS, ids=LAYOUT_IDS)
def test_delta_snapshots_across_a_reset(gpu, oracle, fields):
    task = new_task(fields)
    hist = task.keep_history(max_rows=256, max_flows=32)
    tr = HistoryTruth(fields)
    run_intervals(task, oracle, fields, tr)
    # the input, checked on the truth side: the three classes of flows are there
    by_key = {}
    for ts_, k, pk in zip(tr.ts, tr.key, tr.pkts):
        by_key.setdefault(k, {})[ts_] = pk
    only_first = [k for k, v in by_key.items() if set(v) == {TS[0], TS[1], TS[2]} and v[TS[0]] == v[TS[1]] == v[TS[2]]]
    assert only_first, "a flow seen only in snapshot 0 (its row never changes before the reset, none after)"
    every = [k for k, v in by_key.items() if len(v) == NSNAP and all(v[TS[i]] > v[TS[i - 1]] for i in (1, 2, 4, 5))]
    assert every, "a flow touched in every snapshot"
    back = [k for k, v in by_key.items() if TS[2] in v and TS[3] in v and v[TS[3]] < v[TS[2]]]
    assert back, "a flow that comes back after the reset with a smaller packet count"
    st = hist.stats()
    assert st["snapshots"] == NSNAP and st["keys"] == len(by_key) and hist.times() == TS
    if len(by_key) > 256:  # (the Protocol layout holds three keys: nothing there needs to grow)
        assert st["index_growths"] >= 2 and st["log_growths"] >= 2, st
    # (the index grows before a piece once half its slots are claimed, and no piece may claim beyond 3/4)
    assert st["rows"] <= st["row_capacity"] and 4 * st["keys"] <= 3 * st["index_slots"]
    filters = make_filters(fields)
    engine_filters = [to_filter(f) for f in filters]
    matches = [tr.matches(f) for f in filters]
    for T in query_times():
        assert_history_equals_truth(hist, tr, filters, engine_filters, matches, T, fields)
    # TraceFlow of a flow that came back: max_packets is the old, larger count
    k = back[0]
    flt = dict(zip(fields, k.split("-")))
    s = hist.aggregate([to_filter(flt)], end_time=TS[3])[0]
    assert s.flows == 1 and s.max_packets == by_key[k][TS[2]] > s.packets == by_key[k][TS[3]]
    task.agg.close()
    hist.close()


# --- 3. storing whole views or deltas answers the same ---
@pytest.mark.parametrize("fields", [FIVE, ["Protocol"]], ids=LAYOUT_IDS)
def test_whole_views_against_deltas(gpu, oracle, fields):
    tasks = [new_task(fields, "full"), new_task(fields, "delta")]
    hists = [t.keep_history(max_rows=256, max_flows=32) for t in tasks]
    trs = [HistoryTruth(fields), HistoryTruth(fields)]
    run_intervals(tasks[0], oracle, fields, trs[0], full=True)
    run_intervals(tasks[1], oracle, fields, trs[1], full=False)
    assert hists[0].stats()["rows"] > hists[1].stats()["rows"] and hists[0].stats()["keys"] == hists[1].stats()["keys"]
    flt = [to_filter(f) for f in make_filters(fields)]
    for T in query_times():
        a, b = (h.aggregate(flt, end_time=T) for h in hists)
        assert a == b, T
        for metric in (0, 1):
            x, y = (h.heavy_hitters(metric, end_time=T) for h in hists)
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), (T, metric)
        assert set(rows_of(hists[0].snapshot_arrays(end_time=T))) == set(rows_of(hists[1].snapshot_arrays(end_time=T))), T
    for t, h in zip(tasks, hists):
        t.agg.close()
        h.close()


# --- 4. edges of the link and the scans ---
def unique_batch(rng, first, n):
    """n one-packet flows with IPv4 sources 10.0.0.0 + first .. + first + n - 1."""
    from go2netspectra_amd import PacketBatch
    src = np.zeros((n, 16), np.uint8)
    src[:, :4] = (0x0A000000 + first + np.arange(n)).astype(">u4").view(np.uint8).reshape(n, 4)
    dst = np.zeros((n, 16), np.uint8)
    dst[:, :4] = [192, 0, 2, 1]
    length = rng.integers(64, 1500, n).astype(np.uint32)
    return PacketBatch(src, dst, np.full(n, 1234, np.uint16), np.full(n, 443, np.uint16), np.full(n, 6, np.uint8),
                       length, np.full(n, 4, np.uint8), rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)), int(length.sum())


def test_empty_history_and_append_sizes(gpu):
    from go2netspectra_amd import ExactHistory, Summary
    task = new_task(["SrcIP"])
    hist = task.keep_history(max_rows=64, max_flows=32)
    open_ = to_filter({})
    for T in (None, 0, -(1 << 63), (1 << 63) - 1):
        assert hist.aggregate([open_], end_time=T) == [Summary()]
        assert len(hist.heavy_hitters(0, end_time=T)[1]) == 0 and len(hist.heavy_hitters(1, 5, 3, end_time=T)[1]) == 0
        assert [len(a) for a in hist.snapshot_arrays(end_time=T)] == [0] * 5
    assert hist.times() == [] and hist.stats()["snapshots"] == 0 and hist.stats()["rows"] == 0
    rng = np.random.default_rng(4)
    total, pk, by, rows = 0, 0, 0, {}
    for i, n in enumerate([0, 1, 63, 64, 65, 257, 0]):
        if n:
            b, nbytes = unique_batch(rng, total, n)
            task.process_packets(b)
            pk += n
            by += nbytes
        assert task.record(10 * i) == (n, n), n
        total += n
        s = hist.aggregate([open_])[0]
        assert (s.flows, s.packets, s.bytes, s.max_packets) == (total, pk, by, 1 if total else 0), n
        got = hist.snapshot_arrays()
        assert len(got[3]) == total and len(set(map(bytes, got[0]))) == total
        rows[10 * i] = total
        assert hist.stats()["rows"] == total and hist.stats()["keys"] == total
    for T, want in rows.items():  # every earlier time still answers with its own rows, in log order
        assert hist.aggregate([open_], end_time=T)[0].flows == want and len(hist.snapshot_arrays(end_time=T + 9)[3]) == want
        assert len(hist.heavy_hitters(0, 1, 0, end_time=T)[1]) == want
    first = hist.snapshot_arrays(end_time=20)
    assert np.array_equal(hist.snapshot_arrays()[0][:64], first[0])  # log order: the earlier rows lead
    # a second write of known keys: 65 rows supersede, nothing is new
    task.process_packets(unique_batch(rng, 60, 65)[0])
    assert task.record(100) == (65, 0)
    s = hist.aggregate([open_])[0]
    assert (s.flows, s.packets, s.max_packets) == (total, pk + 65, 2) and hist.stats()["rows"] == total + 65
    assert hist.aggregate([open_], end_time=99)[0].packets == pk
    task.agg.close()
    hist.close()


def test_rejected_appends_change_nothing(gpu):
    from go2netspectra_amd import ExactHistory
    t, ipver, ts = stream()
    task, other = new_task(FIVE), new_task(["SrcIP", "DstIP"])
    hist = task.keep_history(max_rows=256, max_flows=32)
    task.process_packets(batch_of(t, ipver, ts, interval(0)))
    other.process_packets(batch_of(t, ipver, ts, interval(0)))
    task.record(50)
    task.process_packets(batch_of(t, ipver, ts, interval(1)))
    flt = [to_filter(f) for f in make_filters(FIVE, 20)]

    def state():
        return (hist.times(), hist.stats(), hist.aggregate(flt), hist.aggregate(flt, end_time=50), got_heavy(*hist.heavy_hitters(1)),
                rows_of(hist.snapshot_arrays()))
    before = state()
    for bad in (50, 49, -(1 << 63)):
        e_arg(task.record, bad)
    assert state() == before
    wrong = other.view()
    wrong.refresh()
    e_arg(hist.append, wrong, 60)       # another layout
    e_arg(hist.append, task.view(), 60)  # never refreshed
    assert state() == before
    # the interval the rejected records did not store is still stored by the next one
    n1 = task.record(51)[0]
    v = task.view()
    v.refresh()
    assert n1 > 0 and hist.times() == [50, 51] and hist.stats()["rows"] == before[1]["rows"] + n1
    assert hist.aggregate([to_filter({})])[0] == v.aggregate([to_filter({})])[0]
    assert hist.aggregate(flt, end_time=50) == before[3]
    for a in (task.agg, other.agg):
        a.close()
    hist.close()


# --- 5. a reader asks about earlier times while the writer records ---
def test_reader_thread_while_recording(gpu, oracle):
    fields = ["Protocol", "SrcIP"]
    task = new_task(fields)
    hist = task.keep_history(max_rows=256, max_flows=32)
    tr = HistoryTruth(fields)
    run_intervals(task, oracle, fields, tr, reset_after=99, last=2)
    filters = make_filters(fields, 12)
    engine_filters = [to_filter(f) for f in filters]
    times = [TS[0] - 1, TS[0], TS[0] + 1, TS[1]]  # (TS[1] + 1 is TS[2] - 1: still snapshot 1 once 2 exists)
    want = {T: ([tr.summary(f, T) for f in filters], tr.heavy(0, 0, 5, T), tr.rows_at(T)) for T in times}
    stop, errors, rounds = threading.Event(), [], [0]

    def reader():
        try:
            while True:
                last = stop.is_set()  # one full round after the writer is done
                for T in times:
                    got = (hist.aggregate(engine_filters, end_time=T), got_heavy(*hist.heavy_hitters(0, 0, 5, end_time=T)),
                           set(rows_of(hist.snapshot_arrays(end_time=T))))
                    assert got == want[T], T
                rounds[0] += 1
                if last:
                    return
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    th = threading.Thread(target=reader)
    th.start()
    try:
        run_intervals(task, oracle, fields, tr, reset_after=4, first=2)
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    assert rounds[0] >= 1 and hist.stats()["snapshots"] == NSNAP
    matches = [tr.matches(f) for f in filters]
    for T in (TS[1] + 1, TS[3], TS[5], None):
        assert_history_equals_truth(hist, tr, filters, engine_filters, matches, T, "after the writer")
    task.agg.close()
    hist.close()


# --- 6. the task surface: end_time answers from the history, None from the live table ---
def test_task_surface(gpu, oracle):
    from go2netspectra_amd import FlowLifecycle, HeavyHitter, TaskSummary
    task = new_task(FIVE, "five")
    tr = HistoryTruth(FIVE)
    assert task.keep_history(max_rows=256, max_flows=32) is task.keep_history()
    run_intervals(task, oracle, FIVE, tr)
    t, ipver, ts = stream()
    live = HistoryTruth(FIVE)  # the live table: the period since the reset
    live.record(0, tr.oracle.export())
    names = dict(zip(tr.cols()["kb"], tr.key))  # key bytes -> the oracle's Go key string
    flows = [k for k in dict.fromkeys(tr.key)][:40]
    arg = {"SrcIP": "src_ip", "DstIP": "dst_ip", "SrcPort": "src_port", "DstPort": "dst_port", "Protocol": "protocol"}
    for T in (TS[0] - 1, TS[1], TS[2] + 1, TS[4], None):
        truth = live if T is None else tr
        reqs, want = [], []
        for k in flows[:8]:
            parts = dict(zip(FIVE, k.split("-")))
            flt = {"SrcIP": parts["SrcIP"], "Protocol": int(parts["Protocol"])}
            s = truth.summary(flt, T)
            reqs.append(dict({arg[f]: v for f, v in flt.items()}, end_time=T))
            want.append(TaskSummary("five", s.bytes, s.packets, s.flows))
            assert task.aggregate_flows(end_time=T, **{arg[f]: v for f, v in flt.items()}) == want[-1], (T, k)
            full = {f: (int(v) if f not in ("SrcIP", "DstIP") else v) for f, v in parts.items()}
            s = truth.summary(full, T)
            assert task.trace_flow({f: str(v) for f, v in full.items()}, end_time=T) == \
                FlowLifecycle(s.first_ns, s.last_ns, s.max_packets, s.max_bytes), (T, k)
        assert task.aggregate_flows_many(reqs) == want, T
        for typ in (0, 1):
            got = task.heavy_hitters(typ, 9, end_time=T)
            assert got == [HeavyHitter(names[k], v) for k, v in truth.heavy(typ, 0, 9, T)], (T, typ)
    # one batch mixing times: one device call per distinct end_time, answers in request order
    mixed = [dict(protocol=6, end_time=TS[1]), dict(protocol=6), dict(protocol=17, end_time=TS[4]), dict(protocol=6, end_time=TS[1])]
    got = task.aggregate_flows_many(mixed)
    want = [tr.summary({"Protocol": 6}, TS[1]), live.summary({"Protocol": 6}, None), tr.summary({"Protocol": 17}, TS[4]),
            tr.summary({"Protocol": 6}, TS[1])]
    assert got == [TaskSummary("five", s.bytes, s.packets, s.flows) for s in want]
    assert got[0] != got[1]
    task.agg.close()
    task.history.close()
