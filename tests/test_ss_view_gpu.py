"""SuperSpread snapshot views on the GPU (gns_ss_view_*): every answer of a view -- the
list, queries from host and device keys, the exported state and the checkpoint made of it
-- is the sequential oracle's at the refresh point, whatever the handle does afterwards
(more inserts, reclaim, reset, import), from another thread while the handle ingests."""
import ctypes as ct
import threading

import numpy as np
import pytest

from helpers import assert_same_list, frames_from_tuples, random_tuples
from test_ss_gpu import HLL_MASTER, RNG_SEED, assert_same_ss, make_pair, spread_stream

pytestmark = pytest.mark.gpu


def recorded(orc, flows, absent):
    """What the oracle answers now: (list, queries of flows then absent keys, state)."""
    q = np.array([orc.query(bytes(f)) for f in flows] + [orc.query(bytes(f)) for f in absent], np.uint64)
    return orc.heavy(), q, [a.copy() for a in orc.export()]


def view_list(view):
    return [(h.Flow, h.Count) for h in view.heavy_hitters().Count]


def assert_view_is(view, want, flows, absent, what="view", state=True):
    want_hh, want_q, want_state = want
    assert_same_list(view_list(view), want_hh, what + " list")
    keys = np.ascontiguousarray(np.concatenate([flows, absent]))
    assert np.array_equal(view.query_many(keys), want_q), what + " queries"
    got = view.export_state(state=state)
    for name, a, b in zip(("values", "keys", "regs", "pbits"), got, want_state):
        if name == "pbits":
            a, b = a.view(np.uint64), b.view(np.uint64)  # bit patterns
        assert np.array_equal(a, b), f"{what} {name}: {int((a != b).sum())} entries differ"


@pytest.mark.parametrize("w,d,m,size,Kf,Ke,thr,nflows,n", [
    (64, 2, 32, 5, 16, 16, 20, 40, 50_000),        # takeovers all the time
    (1, 1, 16, 8, 4, 4, 1, 30, 30_000),            # one cell
    (1000, 3, 64, 3, 13, 7, 5, 2000, 100_000),     # non-power-of-two w, key no multiple of 4 bytes
    (512, 4, 32, 4, 37, 2, 1, 800, 60_000),        # Kw = 10; flows own several cells: the emit rule and its ties
    (4096, 3, 128, 5, 16, 16, 50, 3000, 200_000),  # the reference's m and size
])
def test_refresh_point_parity(gpu, oracle, w, d, m, size, Kf, Ke, thr, nflows, n):
    import torch
    rng = np.random.default_rng(w + 17 * d + Kf)
    ss, orc = make_pair(oracle, w, d, m, size, Kf, Ke, thr=thr)
    fl, el, flows = spread_stream(rng, n, nflows, Kf, Ke)
    absent = rng.integers(0, 256, (50, Kf), dtype=np.uint8)
    a = (3 * n) // 5
    ss.insert_keys(fl[:a], el[:a])
    view = ss.view()
    view.refresh(state=True)
    orc.insert(fl[:a], el[:a])
    want = recorded(orc, flows, absent)
    ss.insert_keys(fl[a:], el[a:])  # the handle moves on; the view does not
    assert_view_is(view, want, flows, absent)
    qd = view.query_many(torch.from_numpy(np.ascontiguousarray(np.concatenate([flows, absent]))).cuda())
    assert qd.is_cuda and np.array_equal(qd.cpu().numpy().view(np.uint64), want[1])
    rows = view.heavy_hitters_rows_device()
    assert rows.is_cuda and tuple(rows.shape) == (len(want[0]), Kf + 4)
    rows = rows.cpu().numpy()
    got_rows = [(bytes(r[:Kf]), int(np.frombuffer(bytes(r[Kf:]), "<u4")[0])) for r in rows]
    assert_same_list(got_rows, want[0], "device rows")
    assert view.counters() == {"inserted": a, "dropped": 0, "unsupported": 0, "records": a}
    if d > 1 and thr == 1:  # the case meant to exercise the emit rule did: some listed flow owns several cells
        values, keys = want[2][0], want[2][1]
        owned = [bytes(k) for k, v in zip(keys, values) if v > 0]
        assert len(owned) > len(set(owned))
    ss.flush()
    orc.insert(fl[a:], el[a:])
    assert_same_ss(ss, orc)
    assert_same_list([(h.Flow, h.Count) for h in ss.heavy_hitters().Count], orc.heavy(), "handle list")
    view.close()
    ss.close()


def test_view_is_self_contained(gpu, oracle):
    """A 64-flow dictionary that part B grows and reclaims; then reclaim, reset and an import:
    after each the view still answers part A's state, without an error."""
    rng = np.random.default_rng(5)
    Kf = Ke = 16
    ss, orc = make_pair(oracle, 512, 2, 32, 5, Kf, Ke, thr=5, max_flows=64)
    fl, el, flows = spread_stream(rng, 20_000, 300, Kf, Ke)
    absent = rng.integers(0, 256, (50, Kf), dtype=np.uint8)
    ss.insert_keys(fl, el)
    view = ss.view()
    view.refresh(state=True)
    orc.insert(fl, el)
    want = recorded(orc, flows, absent)
    assert len(want[0]) > 0
    fl2, el2, _ = spread_stream(rng, 40_000, 4000, Kf, Ke, s=0.5)
    d0 = ss.dict_stats()
    ss.insert_keys(fl2, el2)
    ss.flush()
    d1 = ss.dict_stats()
    assert d1["growths"] + d1["reclaims"] > d0["growths"] + d0["reclaims"]  # the records the refresh read were moved
    assert_view_is(view, want, flows, absent, "after more inserts")
    other = ss.export_state()
    records = ss.counters()["records"]
    ss.reclaim()
    assert_view_is(view, want, flows, absent, "after reclaim")
    ss.reset()
    assert_view_is(view, want, flows, absent, "after reset")
    assert ss.heavy_hitters().Count == []
    ss.import_state(*other, records)
    assert_view_is(view, want, flows, absent, "after import")
    orc.insert(fl2, el2)
    assert_same_ss(ss, orc)  # (and the handle is where the import put it)
    view.close()
    ss.close()


def test_reader_thread_during_ingest(gpu, oracle):
    rng = np.random.default_rng(21)
    Kf = Ke = 16
    ss, orc = make_pair(oracle, 1 << 14, 3, 128, 5, Kf, Ke, thr=50)
    n, a = 600_000, 200_000
    fl, el, flows = spread_stream(rng, n, 20_000, Kf, Ke, s=1.3, elem_pool=n)
    q = np.ascontiguousarray(flows[:3000])
    ss.insert_keys(fl[:a], el[:a])
    view = ss.view()
    view.refresh()  # the state after packets [0, a)
    orc.insert(fl[:a], el[:a])
    want_hh = orc.heavy()
    want_q = np.array([orc.query(bytes(f)) for f in q], np.uint64)
    assert len(want_hh) > 0
    results, errors = [], []

    def reader():
        try:
            for _ in range(6):
                results.append((view_list(view), view.query_many(q)))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=reader)
    th.start()
    for lo in range(a, n, 50_000):  # ingest continues while the reader runs
        ss.insert_keys(fl[lo:lo + 50_000], el[lo:lo + 50_000])
    th.join()
    assert not errors, errors
    assert len(results) == 6
    for hh, got_q in results:
        assert_same_list(hh, want_hh, "reader list")
        assert np.array_equal(got_q, want_q)
    later = ss.view()
    later.refresh()  # the whole stream
    orc.insert(fl[a:], el[a:])
    assert_same_list(view_list(later), orc.heavy(), "later view")
    assert np.array_equal(later.query_many(q), np.array([orc.query(bytes(f)) for f in q], np.uint64))
    assert_same_list(view_list(view), want_hh, "first view")  # independent of the second
    assert np.array_equal(view.query_many(q), want_q)
    ss.flush()
    assert_same_ss(ss, orc)
    ss.close()  # closes both views first
    assert view._h is None and later._h is None


def test_checkpoint_during_ingest(gpu, oracle, tmp_path):
    from go2netspectra_amd import GnsError, checkpoint
    rng = np.random.default_rng(8)
    Kf, Ke = 13, 7
    ss, orc = make_pair(oracle, 1000, 3, 64, 5, Kf, Ke, thr=5)
    twin, _ = make_pair(oracle, 1000, 3, 64, 5, Kf, Ke, thr=5)  # fed part A only: what a serial save writes
    fl, el, _ = spread_stream(rng, 90_000, 2000, Kf, Ke)
    a = 50_001
    ss.insert_keys(fl[:a], el[:a])
    twin.insert_keys(fl[:a], el[:a])
    view = ss.view()
    view.refresh(state=True)
    ss.insert_keys(fl[a:70_000], el[a:70_000])  # keeps inserting
    checkpoint.save(view, tmp_path / "view.npz")
    ss.insert_keys(fl[70_000:], el[70_000:])
    checkpoint.save(twin, tmp_path / "twin.npz")
    (m1, a1), (m2, a2) = checkpoint.read(tmp_path / "view.npz"), checkpoint.read(tmp_path / "twin.npz")
    assert m1 == m2 and m1["class"] == "SuperSpread" and m1["records"] == a
    assert sorted(a1) == sorted(a2) and all(np.array_equal(a1[k], a2[k]) and a1[k].dtype == a2[k].dtype for k in a1)
    fresh, _ = make_pair(oracle, 1000, 3, 64, 5, Kf, Ke, thr=5)
    checkpoint.restore(fresh, tmp_path / "view.npz")
    fresh.insert_keys(fl[a:], el[a:])
    fresh.flush()
    orc.insert(fl, el)
    assert_same_ss(fresh, orc)  # so the generator position travelled
    ss.flush()
    assert_same_ss(ss, orc)
    view.refresh()  # without state
    view.export_state(state=False)
    with pytest.raises(GnsError):
        view.export_state()
    with pytest.raises(GnsError):
        view.counters()
    with pytest.raises(GnsError):
        checkpoint.save(view, tmp_path / "nostate.npz")
    for x in (view, ss, twin, fresh):
        x.close()


def test_export_spans_more_than_two_pinned_chunks(gpu):
    """The view's export goes out through two 4 MiB pinned chunks.  Nine-byte flows are three
    key words a cell (12-byte rows of which 9 go out; 4 MiB is no multiple of 12), and
    4 * 2^18 cells make 12 MiB of them: four pieces, so both chunks are used twice and every
    piece but the first starts inside the destination at an offset that is no multiple of the
    chunk.  The handle's own export takes another route (ids -> bytes on the device), so the
    two agree only if every piece landed where it belongs."""
    from go2netspectra_amd import SuperSpread
    rng = np.random.default_rng(99)
    w, d, m, Kf, Ke = 1 << 18, 4, 32, 9, 4
    seeds = rng.integers(0, 2**32, d, dtype=np.uint64).astype(np.uint32)
    ss = SuperSpread(w, d, 1, m, 5, 0.5, 1.08, flow_bytes=Kf, elem_bytes=Ke, seeds=seeds, hll_master=HLL_MASTER,
                     rng_seed=RNG_SEED)
    fl, el, _ = spread_stream(rng, 6000, 3000, Kf, Ke)
    ss.insert_keys(fl, el)
    view = ss.view()
    view.refresh(state=True)
    want = ss.export_state()  # the same point: nothing is inserted after the refresh
    got = view.export_state()
    assert int((want[0] != 0).sum()) > 1000  # cells all over the rows hold flows
    owned = np.flatnonzero(want[0])
    assert owned.min() < (1 << 18) and owned.max() > 3 * (1 << 18)  # in the first and in the last piece
    for name, a, b in zip(("values", "keys", "regs", "pbits"), got, want):
        if name == "pbits":
            a, b = a.view(np.uint64), b.view(np.uint64)  # bit patterns
        assert a.shape == b.shape and np.array_equal(a, b), f"{name}: {int((a != b).sum())} entries differ"
    view.close()
    ss.close()


def test_edges(gpu, oracle):
    from go2netspectra_amd import GnsError, _lib
    rng = np.random.default_rng(13)
    Kf = Ke = 8
    ss, orc = make_pair(oracle, 256, 2, 32, 5, Kf, Ke, thr=3)
    fl, el, flows = spread_stream(rng, 40_000, 400, Kf, Ke)
    ss.insert_keys(fl[:20_000], el[:20_000])
    orc.insert(fl[:20_000], el[:20_000])
    view = ss.view()
    for call in (view.heavy_hitters, lambda: view.query_many(flows[:4]), lambda: view.export_state(state=False),
                 view.heavy_hitters_rows_device):
        with pytest.raises(GnsError, match="never refreshed"):
            call()
    ss.set_timing(True)
    view.refresh()
    ss.flush()
    assert ss.stage_times()["view"][1] == 1  # one timed refresh in slot 6
    ss.set_timing(False)
    want = orc.heavy()
    assert len(want) > 8
    assert_same_list(view_list(view), want)
    # capacity: *n smaller than the list -> the full length comes back, nothing at or past the capacity is written
    L, cap = _lib.load(), 5
    f = np.full((len(want) + 4, Kf), 0xEE, np.uint8)
    v = np.full(len(want) + 4, 0xEEEEEEEE, np.uint32)
    n = ct.c_uint64(cap)
    assert L.gns_ss_view_heavy_hitters(view._h, f.ctypes.data, v.ctypes.data, ct.byref(n)) == 0
    assert n.value == len(want)
    assert [(bytes(f[i]), int(v[i])) for i in range(cap)] == want[:cap]
    assert (f[cap:] == 0xEE).all() and (v[cap:] == 0xEEEEEEEE).all()
    import torch
    rows = torch.full((len(want), Kf + 4), 0xEE, dtype=torch.uint8, device="cuda")
    n = ct.c_uint64(cap)
    assert L.gns_ss_view_heavy_rows(view._h, rows.data_ptr(), ct.byref(n)) == 0 and n.value == len(want)
    assert bool((rows == 0xEE).all())  # a list longer than its buffer is reported, not written
    # stride < flow_bytes and a null out are argument errors
    out = np.zeros(4, np.uint64)
    k = np.ascontiguousarray(flows[:4])
    assert L.gns_ss_view_query(view._h, k.ctypes.data, Kf - 1, 4, out.ctypes.data) == _lib.GNS_E_ARG
    assert L.gns_ss_view_query(view._h, k.ctypes.data, Kf, 4, None) == _lib.GNS_E_ARG
    assert L.gns_ss_view_heavy_hitters(view._h, None, None, None) == _lib.GNS_E_ARG
    # a second refresh replaces the first
    ss.insert_keys(fl[20_000:], el[20_000:])
    orc.insert(fl[20_000:], el[20_000:])
    view.refresh(state=True)
    assert_view_is(view, recorded(orc, flows, flows[:0]), flows, flows[:0], "second refresh")
    # an empty list at a high threshold
    hi, orc_hi = make_pair(oracle, 256, 2, 32, 5, Kf, Ke, thr=10**9)
    hi.insert_keys(fl, el)
    orc_hi.insert(fl, el)
    vh = hi.view()
    vh.refresh()
    assert view_list(vh) == [] == orc_hi.heavy()
    assert tuple(vh.heavy_hitters_rows_device().shape) == (0, Kf + 4)
    assert np.array_equal(vh.query_many(flows), np.array([orc_hi.query(bytes(x)) for x in flows], np.uint64))
    for x in (view, ss, vh, hi):
        x.close()


THREE_TASKS = """
aggregator:
  types: ["sketch", "exact"]
  sketch:
    tasks:
      - {name: cm_src, skt_type: 0, flow_fields: [SrcIP], element_fields: [DstIP, SrcPort, DstPort, Protocol],
         width: 4096, depth: 2, size_thereshold: 100000, count_thereshold: 50}
      - {name: ss_src_dst, skt_type: 1, flow_fields: [SrcIP], element_fields: [DstIP], width: 4096, depth: 2,
         count_thereshold: 1, m: 128, size: 5, b: 1.08, base: 0.5}
  exact:
    tasks:
      - {name: per_five_tuple, key_fields: [SrcIP, DstIP, SrcPort, DstPort, Protocol]}
"""


def test_task_and_manager_views(gpu, tmp_path):
    from go2netspectra_amd import CountMinView, ExactView, HeaderBatch, Manager, SuperSpreadView, parse_config
    rng = np.random.default_rng(55)
    n, cut = 40_000, 23_001
    t = random_tuples(rng, n, 3000, v6_frac=0.2)
    hdr = frames_from_tuples(t, rng, vlan_frac=0.2)
    ts = np.cumsum(rng.integers(0, 5000, n)).astype(np.int64)
    batch = lambda lo, hi: HeaderBatch(hdr[lo:hi], t["length"][lo:hi], ts[lo:hi])
    mgr = Manager(parse_config(THREE_TASKS), seeds=np.array([11, 22, 33, 44], np.uint32), hll_master=HLL_MASTER,
                  rng_seed=RNG_SEED)
    assert [x.name() for x in mgr.tasks()] == ["cm_src", "ss_src_dst", "per_five_tuple"]
    views = mgr.views()
    assert [type(v) for v in views] == [CountMinView, SuperSpreadView, ExactView]
    mgr.process(batch(0, cut))
    mgr.refresh_views(views)
    want = mgr.snapshot()  # the same point: nothing was inserted in between
    rules = [{"name": "spread", "task_name": "ss_src_dst", "metric": "super_spreader_spread", "operator": ">=",
              "threshold": 2},
             {"name": "count", "task_name": "cm_src", "metric": "heavy_hitter_count", "operator": ">", "threshold": 60}]
    want_msg = [task.alerter_msg(rules) for task in mgr.tasks()[:2]]
    assert all("<table" in m for m in want_msg)
    mgr.process(batch(cut, n))
    got = mgr.snapshot_from_views(views)
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
    assert len(want["ss_src_dst"].Count) > 0 and want["ss_src_dst"].Size is None
    assert [task.alerter_msg(rules, view=v) for task, v in zip(mgr.tasks()[:2], views[:2])] == want_msg
    assert mgr.snapshot()["ss_src_dst"] != want["ss_src_dst"]  # the live tasks moved on
    # a task's checkpoint from its view
    from go2netspectra_amd import checkpoint
    ss_task, ss_view = mgr.tasks()[1], views[1]
    mgr.refresh_views(views, state=True)
    assert ss_view.counters()["records"] == n
    ss_task.save_from(ss_view, tmp_path / "from_view.npz")
    ss_task.save(tmp_path / "serial.npz")
    (m1, a1), (m2, a2) = checkpoint.read(tmp_path / "from_view.npz"), checkpoint.read(tmp_path / "serial.npz")
    assert m1 == m2 and all(np.array_equal(a1[k], a2[k]) for k in a2)
    for v in views:
        v.close()
    for task in mgr.tasks():
        (task.sketch if hasattr(task, "sketch") else task.agg).close()
