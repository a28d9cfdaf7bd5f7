"""Snapshot views of the exact engine on the GPU (gns_ex_view_*): a full view is the
snapshot and the oracle, a delta view is exactly the flows touched since its cursor, a
view stays what it was at its refresh whatever the handle does afterwards, the query plane
answers on a view as on the table, and a reader thread reads a view while the handle
ingests.  Truth: oracle.Exact, and the ClickHouse comparison of exact_query_truth.py.
Device batches are 16K packets, so every stream below spans several and flows become
designated."""
import threading

import numpy as np
import pytest

from exact_query_truth import (FIVE, batch_of, got_heavy, key_bytes_of, oracle_export, packet_value, to_filter,
                               tricky_stream, truth_heavy, truth_rows, truth_summary)
from helpers import assert_same_flows, assert_same_list, random_tuples

pytestmark = pytest.mark.gpu

NAMES = ("keys", "start", "end", "packets", "bytes")
_CACHE = {}


def stream():
    """60k packets over 2500 flows: v4, v6 and v4-mapped arrivals of the same flows."""
    if "s" not in _CACHE:
        _CACHE["s"] = tricky_stream(7, 60_000, 2500)
    return _CACHE["s"]


def new_task(fields, max_flows=1 << 12, name="v"):
    from go2netspectra_amd import ExactTask
    return ExactTask(name, fields, batch_packets=4096, max_flows=max_flows)


def as_dict(arrays):
    from go2netspectra_amd import apply_delta
    return apply_delta({}, arrays)


def want_dict(export, fields):
    return {key_bytes_of(k, fields): v for k, v in export.items()}


def assert_same_arrays(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape, f"{what}: {name} {a.shape} vs {b.shape}"
        assert np.array_equal(a, b), f"{what}: {name} differs first at row {int(np.argmax((a != b).reshape(len(a), -1).any(1)))}"


def e_arg(fn, *a):
    from go2netspectra_amd import GnsError, _lib
    with pytest.raises(GnsError) as e:
        fn(*a)
    assert e.value.code == _lib.GNS_E_ARG, e.value


# --- 1. a full view is the snapshot and the oracle, at every record width ---
@pytest.mark.parametrize("fields", [FIVE, ["SrcIP"], ["DstPort", "Protocol"]], ids=lambda f: "-".join(f))
def test_full_view_equals_snapshot_and_oracle(gpu, oracle, fields):
    t, ipver, ts = stream()
    task = new_task(fields)
    task.process_packets(batch_of(t, ipver, ts))
    view = task.view()
    cur = view.refresh()
    assert cur == 60_000 == task.agg.counters()["records"]
    got, snap = view.snapshot_arrays(), task.agg.snapshot_arrays()
    assert_same_arrays(got, snap, f"{fields}: view vs snapshot_arrays")
    assert got[0].shape[1] == task.agg.key_bytes
    assert_same_flows(as_dict(got), want_dict(oracle_export(oracle, fields, t, ipver, ts), fields), "view vs oracle")
    snapd = task.snapshot_from(view)
    assert sum(len(s.Flows) for s in snapd.Shards) == len(got[3])
    assert task.snapshot_from(view) == task.snapshot()
    view.close()
    task.agg.close()


# --- 2. compaction edges: rows and order = the snapshot filtered on the host ---
def unique_stream(rng, n, base=0x0A000000):
    """n packets of n flows (distinct IPv4 sources base + 7 i)."""
    ids = (base + 7 * np.arange(n)).astype(">u4")
    src = np.zeros((n, 16), np.uint8)
    src[:, :4] = ids.view(np.uint8).reshape(n, 4)
    dst = np.zeros((n, 16), np.uint8)
    dst[:, :4] = [192, 0, 2, 1]
    t = dict(src16=src, dst16=dst, sport=np.full(n, 1234, np.uint16), dport=np.full(n, 443, np.uint16),
             proto=np.full(n, 6, np.uint8), length=rng.integers(64, 1500, n).astype(np.uint32))
    return t, np.full(n, 4, np.uint8), rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64), ids.astype(np.uint32)


def host_filter(snap, ids):
    """The rows of a SrcIP-keyed snapshot whose source is one of ``ids``, in snapshot order."""
    src = snap[0][:, 12:16].copy().view(">u4").reshape(-1).astype(np.uint32)
    keep = np.isin(src, ids)
    return tuple(a[keep] for a in snap)


@pytest.mark.parametrize("nflows,max_flows", [(150_000, 1 << 18), (5_000, 1 << 21)], ids=["dense-150k", "sparse-4M-slots"])
def test_compaction_edges(gpu, nflows, max_flows):
    """150k one-packet flows: more than 65,536 rows over 2048 slot blocks (8 per scan bin).  5k
    flows in 2^22 slots: 16384 slot blocks, most of them empty, two groups of the scan."""
    rng = np.random.default_rng(nflows)
    t, ipver, ts, ids = unique_stream(rng, nflows)
    task = new_task(["SrcIP"], max_flows=max_flows)
    view = task.view()
    task.process_packets(batch_of(t, ipver, ts))
    c1 = view.refresh()
    snap = task.agg.snapshot_arrays()
    assert len(snap[3]) == nflows and (snap[3] == 1).all()
    assert_same_arrays(view.snapshot_arrays(), snap, "full view")
    assert task.agg.dict_stats()["growths"] == 0
    # a delta selecting nothing
    assert view.refresh(c1) == c1
    got = view.snapshot_arrays()
    assert [len(a) for a in got] == [0] * 5 and got[0].shape == (0, 16)
    assert view.aggregate([to_filter({})])[0].flows == 0 and len(view.heavy_hitters(0)[1]) == 0
    # a delta whose touched flows leave whole slot blocks and whole waves empty
    some = rng.choice(nflows, 300, replace=False)
    task.process_packets(batch_of(t, ipver, ts + 1, some))
    c2 = view.refresh(c1)
    assert c2 == c1 + 300
    snap = task.agg.snapshot_arrays()
    want = host_filter(snap, ids[some])
    assert len(want[3]) == 300 and (want[3] == 2).all()
    assert_same_arrays(view.snapshot_arrays(), want, "sparse delta")
    # a delta selecting every flow
    task.process_packets(batch_of(t, ipver, ts + 2))
    c3 = view.refresh(c2)
    assert c3 == c2 + nflows
    snap = task.agg.snapshot_arrays()
    assert_same_arrays(view.snapshot_arrays(), snap, "delta of every flow")
    assert view.refresh(c2 + 1) == c3  # a cursor inside the last window: all but the flow of its first packet
    got = view.snapshot_arrays()
    assert_same_arrays(got, host_filter(snap, np.delete(ids, 0)), "all but one")
    view.close()
    task.agg.close()


# --- 3. a view stays what it was at its refresh ---
def test_view_is_frozen_at_its_refresh(gpu, oracle):
    from go2netspectra_amd import Summary
    t, ipver, ts = stream()
    fields = FIVE
    task = new_task(fields, max_flows=1024)
    view = task.view()
    e_arg(view.snapshot_arrays)  # never refreshed
    e_arg(view.aggregate, [to_filter({})])
    e_arg(view.heavy_hitters, 0)
    task.process_packets(batch_of(t, ipver, ts, slice(0, 20_000)))
    e_arg(view.refresh, 20_001)  # beyond the stream position: the view stays unrefreshed
    e_arg(view.snapshot_arrays)
    cur = view.refresh()
    assert cur == 20_000
    want = oracle_export(oracle, fields, t, ipver, ts, slice(0, 20_000))
    rows = truth_rows(want, fields)
    filters = [{}, {"SrcIP": packet_value(t, ipver, 3, "SrcIP")}, {f: packet_value(t, ipver, 9, f) for f in FIVE},
               {"Protocol": 6}, {"Protocol": 200}]
    exp_sum = [truth_summary(rows, fields, f) for f in filters]
    assert exp_sum[0].flows == len(want) and exp_sum[2].flows == 1 and exp_sum[4] == Summary()
    snap0 = task.agg.snapshot_arrays()

    def check(what):
        got = view.snapshot_arrays()
        assert_same_arrays(got, snap0, what)
        assert_same_flows(as_dict(got), want_dict(want, fields), what)
        assert view.aggregate([to_filter(f) for f in filters]) == exp_sum, what
        for metric in (0, 1):
            assert_same_list(got_heavy(*view.heavy_hitters(metric)), truth_heavy(want, fields, metric), what)
            assert_same_list(got_heavy(*view.heavy_hitters(metric, 0, 10)), truth_heavy(want, fields, metric, 0, 10), what)

    check("at the refresh")
    task.process_packets(batch_of(t, ipver, ts, slice(20_000, 60_000)))  # 40k more packets
    check("after more ingest")
    t2, ipver2, ts2 = tricky_stream(11, 40_000, 20_000)  # many new flows: a table of 1024 grows
    task.process_packets(batch_of(t2, ipver2, ts2))
    assert task.agg.dict_stats()["growths"] >= 2
    check("after table growth")
    task.agg.merge(*snap0)
    check("after a merge")
    e_arg(view.refresh, task.agg.counters()["records"] + len(snap0[3]) + 1)  # since beyond the position ...
    check("after a refused refresh")                                         # ... leaves the view untouched
    task.reset()
    assert task.agg.aggregate([to_filter({})]) == [Summary()]
    check("after a reset")
    view.refresh()
    assert [len(a) for a in view.snapshot_arrays()] == [0] * 5
    assert view.aggregate([to_filter({})]) == [Summary()]
    view.close()
    task.agg.close()


# --- 4. deltas ---
def merge_truth(state, rows):
    """gns_ex_merge restated on a key -> (start, end, packets, bytes) map."""
    out = dict(state)
    keys, st, en, pk, by = rows
    for i in range(len(pk)):
        if int(pk[i]) == 0:
            continue
        k = bytes(keys[i])
        if k in out:
            s, _, p, b = out[k]
            out[k] = (s, int(en[i]), (p + int(pk[i])) & (2**64 - 1), (b + int(by[i])) & (2**64 - 1))
        else:
            out[k] = (int(st[i]), int(en[i]), int(pk[i]), int(by[i]))
    return out


@pytest.mark.parametrize("touched_list", [False, True], ids=["scan", "GNS_EX_LIST"])
def test_deltas_are_the_flows_touched_since_the_cursor(gpu, oracle, monkeypatch, touched_list):
    from go2netspectra_amd import apply_delta
    if touched_list:
        monkeypatch.setenv("GNS_EX_LIST", "1")
    fields = FIVE
    rng = np.random.default_rng(31)
    t = random_tuples(rng, 80_000, 3000, v6_frac=0.3)
    ipver = np.where(t["v6"], 6, 4).astype(np.uint8)
    ts = rng.integers(-(1 << 40), 1 << 40, 80_000).astype(np.int64)
    task = new_task(fields, max_flows=1024)  # grows under the first windows
    view, full = task.view(), task.view()
    orc = oracle.Exact(fields)
    state, before, cur = {}, {}, 0
    for w in range(4):  # four windows with chained cursors
        sel = slice(20_000 * w, 20_000 * (w + 1))
        task.process_packets(batch_of(t, ipver, ts, sel))
        orc.insert_tuples(t["src16"][sel], t["dst16"][sel], t["sport"][sel], t["dport"][sel], t["proto"][sel],
                          ipver[sel], t["length"][sel], ts[sel])
        after = want_dict(orc.export(), fields)
        nxt = view.refresh(cur)
        assert nxt == 20_000 * (w + 1)
        delta = view.snapshot_arrays()
        changed = {k for k, v in after.items() if before.get(k, (0, 0, 0, 0))[2] != v[2]}
        assert len(set(map(bytes, delta[0]))) == len(delta[3]), "a flow appears once"
        assert set(map(bytes, delta[0])) == changed, f"window {w}"
        assert 0 < len(changed) < len(after) or w == 0
        state = apply_delta(state, delta)
        assert_same_flows(state, after, f"fold after window {w}")
        before, cur = after, nxt
    assert task.agg.dict_stats()["growths"] >= 1
    full.refresh()
    assert_same_flows(as_dict(full.snapshot_arrays()), before, "full view vs oracle")
    assert_same_flows(state, as_dict(full.snapshot_arrays()), "fold vs full view")
    # two refreshes with no packets between them
    assert view.refresh(cur) == cur
    assert len(view.snapshot_arrays()[3]) == 0
    # a window containing a merge: existing keys, new keys, rows without packets
    snap = full.snapshot_arrays()
    pick = rng.choice(len(snap[3]), 200, replace=False)
    mk = np.concatenate([snap[0][pick], rng.integers(0, 256, (100, 37), dtype=np.uint8)])
    mpk = rng.integers(1, 50, 300).astype(np.uint64)
    mpk[::7] = 0  # rows without packets: ignored, old key or new
    rows = (mk, rng.integers(-1000, 1000, 300).astype(np.int64), rng.integers(2000, 3000, 300).astype(np.int64), mpk,
            rng.integers(1, 1 << 34, 300).astype(np.uint64))
    task.agg.merge(*rows)
    truth = merge_truth(before, rows)
    nxt = view.refresh(cur)
    assert nxt == cur + 300  # merged rows take stream positions
    delta = view.snapshot_arrays()
    assert set(map(bytes, delta[0])) == {bytes(mk[i]) for i in range(300) if mpk[i]}
    assert (delta[3] != 0).all()
    state = apply_delta(state, delta)
    assert_same_flows(state, truth, "fold after the merge")
    full.refresh()
    assert_same_flows(as_dict(full.snapshot_arrays()), truth, "full view after the merge")
    cur = nxt
    # a table growth between the cursor and the refresh: the renumbering carries `last`
    growths = task.agg.dict_stats()["growths"]
    t2 = random_tuples(rng, 30_000, 12_000, s=0.3)
    ipver2 = np.full(30_000, 4, np.uint8)
    ts2 = rng.integers(-(1 << 40), 1 << 40, 30_000).astype(np.int64)
    old = slice(100, 400)  # a few packets of the first stream ahead of the new flows, in the same window
    task.process_packets(batch_of(t, ipver, ts, old))
    task.process_packets(batch_of(t2, ipver2, ts2))
    assert task.agg.dict_stats()["growths"] > growths
    touched = set(want_dict(oracle_export(oracle, fields, t, ipver, ts, old), fields))
    touched |= set(want_dict(oracle_export(oracle, fields, t2, ipver2, ts2), fields))
    nxt = view.refresh(cur)
    assert nxt == cur + 300 + 30_000
    delta = view.snapshot_arrays()
    assert set(map(bytes, delta[0])) == touched
    state = apply_delta(state, delta)
    full.refresh()
    assert_same_flows(state, as_dict(full.snapshot_arrays()), "fold after the growth")
    assert_same_arrays(full.snapshot_arrays(), task.agg.snapshot_arrays(), "full view after the growth")
    # a cursor from before a reset selects every flow of the new period
    task.reset()
    sel = slice(60_000, 65_000)
    task.process_packets(batch_of(t, ipver, ts, sel))
    assert view.refresh(nxt) == nxt + 5_000  # positions never restart
    got = view.snapshot_arrays()
    assert_same_arrays(got, task.agg.snapshot_arrays(), "a cursor from before the reset")
    assert_same_flows(as_dict(got), want_dict(oracle_export(oracle, fields, t, ipver, ts, sel), fields), "new period")
    view.close()
    full.close()
    task.agg.close()


# --- 5. the query plane on a view ---
def tie_stream(rng):
    """400 flows keyed without the protocol: 50 heavy ones with distinct counts, 50 with 9
    packets of lengths near 2^32, 150 with 5 packets and 150 with 1 packet of 100 bytes each:
    runs of equal values under both metrics."""
    nfl = 400
    src, dst = np.zeros((nfl, 16), np.uint8), np.zeros((nfl, 16), np.uint8)
    src[:, :4] = rng.integers(0, 256, (nfl, 4))
    src[200:, :4] = src[200, :4]  # one source address shared by 200 flows
    dst[:, :4] = rng.integers(0, 256, (nfl, 4))
    sport = np.arange(nfl).astype(np.uint16)
    counts = np.concatenate([100 + 3 * np.arange(50), np.full(50, 9), np.full(150, 5), np.full(150, 1)])
    idx = rng.permutation(np.repeat(np.arange(nfl), counts))
    n = len(idx)
    length = rng.integers(64, 1500, n).astype(np.uint32)
    length[(idx >= 50) & (idx < 100)] = rng.integers(1 << 31, 1 << 32, int(((idx >= 50) & (idx < 100)).sum()),
                                                      dtype=np.uint64).astype(np.uint32)
    length[idx >= 100] = 100
    tt = dict(src16=src[idx], dst16=dst[idx], sport=sport[idx], dport=np.full(n, 443, np.uint16),
              proto=np.full(n, 6, np.uint8), length=length)
    return tt, np.full(n, 4, np.uint8), rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64), idx


def test_queries_on_a_view(gpu, oracle):
    fields = ["SrcIP", "DstIP", "SrcPort", "DstPort"]  # Protocol is a field outside the key
    t, ipver, ts, idx = tie_stream(np.random.default_rng(5))
    n = len(ipver)
    first = np.flatnonzero(idx < 300)  # the first period leaves 100 one-packet flows out
    task = new_task(fields, max_flows=1 << 10)
    task.process_packets(batch_of(t, ipver, ts, first))
    view = task.view()
    cur = view.refresh()
    base = [{}, {"SrcIP": packet_value(t, ipver, int(np.flatnonzero(idx == 200)[0]), "SrcIP")},
            {f: packet_value(t, ipver, int(first[0]), f) for f in fields}, {"Protocol": 6}]
    want = oracle_export(oracle, fields, t, ipver, ts, first)
    rows = truth_rows(want, fields)
    asked = {}
    for nf in (1, 5, 70):  # narrow, wide, two passes
        flt = [to_filter(base[(i + nf) % 4]) for i in range(nf)]
        asked[nf] = (flt, task.agg.aggregate(flt))  # the handle's answers at the refresh point
        assert asked[nf][1] == [truth_summary(rows, fields, base[(i + nf) % 4]) for i in range(nf)]
        assert view.aggregate(flt) == asked[nf][1], nf
    s = {i: truth_summary(rows, fields, base[i]) for i in range(4)}
    assert s[0].flows == 300 and s[1].flows == 100 and s[2].flows == 1 and s[3].flows == 0
    heavy = {}
    for metric in (0, 1):
        for limit in (0, 180, 75):  # 180 cuts inside the run of 5-packet / 500-byte flows
            heavy[metric, limit] = got_heavy(*task.agg.heavy_hitters(metric, 0, limit))
            assert_same_list(heavy[metric, limit], truth_heavy(want, fields, metric, 0, limit), "handle")
            assert_same_list(got_heavy(*view.heavy_hitters(metric, 0, limit)), heavy[metric, limit], "view")
        vals = [v for _, v in heavy[metric, 0]]
        assert vals[179] == vals[180] == (500 if metric else 5)
        thr = vals[120]
        assert_same_list(got_heavy(*view.heavy_hitters(metric, thr, 60)), truth_heavy(want, fields, metric, thr, 60),
                         "threshold and limit")
    # more ingest changes the handle's answers, not the view's
    rest = np.flatnonzero((idx >= 300) | (idx % 3 == 0))
    task.process_packets(batch_of(t, ipver, ts + 5, rest))
    assert task.agg.aggregate(asked[5][0]) != asked[5][1]
    for nf, (flt, exp) in asked.items():
        assert view.aggregate(flt) == exp, nf
    for (metric, limit), exp in heavy.items():
        assert_same_list(got_heavy(*view.heavy_hitters(metric, 0, limit)), exp, "view after more ingest")
    # a delta view answers over the touched subset
    assert view.refresh(cur) == cur + len(rest)
    o = oracle.Exact(fields)
    for sel, d in ((first, 0), (rest, 5)):
        o.insert_tuples(t["src16"][sel], t["dst16"][sel], t["sport"][sel], t["dport"][sel], t["proto"][sel],
                        ipver[sel], t["length"][sel], ts[sel] + d)
    now = o.export()
    touched = set(oracle_export(oracle, fields, t, ipver, ts, rest))
    sub = {k: v for k, v in now.items() if k in touched}
    assert 0 < len(sub) < len(now)
    srows = truth_rows(sub, fields)
    for nf in (1, 5, 70):
        assert view.aggregate(asked[nf][0]) == [truth_summary(srows, fields, base[(i + nf) % 4]) for i in range(nf)], nf
    for metric in (0, 1):
        assert_same_list(got_heavy(*view.heavy_hitters(metric, 0, 50)), truth_heavy(sub, fields, metric, 0, 50), "delta top 50")
    assert n == len(first) + int((idx >= 300).sum())
    view.close()
    task.agg.close()


# --- 6. a reader thread on a view while the handle ingests ---
def test_view_answers_the_state_at_refresh_while_ingesting(gpu, oracle):
    fields = FIVE
    rng = np.random.default_rng(21)
    n, a = 600_000, 200_000
    t = random_tuples(rng, n, 30_000)
    ipver = np.full(n, 4, np.uint8)
    ts = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    task = new_task(fields, max_flows=1 << 16)
    task.process_packets(batch_of(t, ipver, ts, slice(0, a)))
    view = task.view()
    view.refresh()  # the state after packets [0, a)
    want = oracle_export(oracle, fields, t, ipver, ts, slice(0, a))
    rows = truth_rows(want, fields)
    filters = [{}, {"Protocol": 17}, {f: packet_value(t, ipver, 5, f) for f in FIVE}]
    exp_sum = [truth_summary(rows, fields, f) for f in filters]
    exp_top = [truth_heavy(want, fields, m, 0, 100) for m in (0, 1)]
    snap0 = task.agg.snapshot_arrays()
    assert_same_flows(as_dict(snap0), want_dict(want, fields), "snapshot at the refresh point")
    results, errors = [], []

    def reader():
        try:
            for _ in range(6):
                results.append((view.snapshot_arrays(), view.aggregate([to_filter(f) for f in filters]),
                                [got_heavy(*view.heavy_hitters(m, 0, 100)) for m in (0, 1)]))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=reader)
    th.start()
    for lo in range(a, n, 50_000):  # ingest continues while the reader runs
        task.process_packets(batch_of(t, ipver, ts, slice(lo, lo + 50_000)))
    th.join()
    assert not errors, errors
    assert len(results) == 6
    for snap, summ, top in results:
        assert_same_arrays(snap, snap0, "reader snapshot")
        assert summ == exp_sum
        assert top == exp_top
    cur = view.refresh()  # now the whole stream
    assert cur == n
    want = oracle_export(oracle, fields, t, ipver, ts)
    assert_same_flows(as_dict(view.snapshot_arrays()), want_dict(want, fields), "after the next refresh")
    assert view.aggregate([to_filter({})])[0] == truth_summary(truth_rows(want, fields), fields, {})
    view.close()
    task.agg.close()
