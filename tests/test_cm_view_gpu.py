"""Detached Count-Min snapshot views on the GPU (gns_cm_view_refresh_at with
GNS_CM_VIEW_DETACH): every answer of a view -- both lists, queries from host and device
keys, the packed device rows, the exported state, the counters and the checkpoint made of
them -- is the sequential oracle's at the refresh point, whatever the handle does afterwards
(more inserts, reclaim, dictionary growth, reset, import), from another thread while the
handle ingests.  Every comparison is bit-exact."""
import ctypes as ct
import threading

import numpy as np
import pytest

from helpers import assert_same_list, frames_from_tuples, random_tuples, sizes_u32, zipf_keys
from test_cm_gpu import assert_same_state, make_pair

pytestmark = pytest.mark.gpu

STATE = ("C", "S", "FPc", "FPs")


def recorded(orc, flows, absent):
    """What the oracle answers now: (count list, size list, queries of flows then absent keys, state)."""
    q = np.array([orc.query(bytes(f)) for f in flows] + [orc.query(bytes(f)) for f in absent], np.uint64)
    return orc.heavy("count"), orc.heavy("size"), q, [a.copy() for a in orc.export()]


def lists_of(x):
    hh = x.heavy_hitters()
    return [(h.Flow, h.Count) for h in hh.Count], [(h.Flow, h.Size) for h in hh.Size]


def rows_list(rows, K):
    rows = rows.cpu().numpy()
    return [(bytes(r[:K]), int(np.frombuffer(bytes(r[K:]), "<u4")[0])) for r in rows]


def assert_same_arrays(got, want, what):
    for name, a, b in zip(STATE, got, want):
        assert a.shape == b.shape, f"{what} {name}: shape {a.shape} against {b.shape}"
        assert np.array_equal(a, b), f"{what} {name}: {int((a != b).sum())} entries differ"


def assert_view_is(view, want, flows, absent, what="view", state=True):
    want_c, want_s, want_q, want_state = want
    got_c, got_s = lists_of(view)
    assert_same_list(got_c, want_c, what + " count list")
    assert_same_list(got_s, want_s, what + " size list")
    keys = np.ascontiguousarray(np.concatenate([flows, absent]))
    assert np.array_equal(view.query_many(keys), want_q), what + " queries"
    if state:
        assert_same_arrays(view.export_state(), want_state, what)


def distinct_owners(state):
    """The flows a state's fingerprint arrays name (no all-zero key among them)."""
    fp = np.concatenate([state[2], state[3]])
    return np.unique(fp[fp.any(axis=1)], axis=0)


@pytest.mark.parametrize("w,d,K,nflows,n,s,kw", [
    (1, 1, 4, 30, 30_000, 1.1, {}),                             # one cell, constant take-overs
    (16, 2, 13, 200, 50_000, 1.1, {}),                          # C == 0 under a live FPc; key no multiple of 4; the zero key
    (1000, 3, 8, 2000, 100_000, 1.1, {}),                       # non-power-of-two w
    (256, 8, 37, 800, 60_000, 1.1, {}),                         # 128-byte dictionary records, 10 key words
    (4096, 4, 16, 20_000, 200_000, 0.5, {"max_flows": 1 << 15}),  # > 8192 marked slots of a 2^16-slot dictionary
])
def test_refresh_point_parity(gpu, oracle, w, d, K, nflows, n, s, kw):
    import torch
    rng = np.random.default_rng(w + 17 * d + K)
    cm, orc = make_pair(oracle, w, d, K, st=3000, ct=8, **kw)
    _, flows, idx = zipf_keys(rng, n, nflows, K, s=s)
    if K == 13:
        flows[2] = 0  # the all-zero key is a flow like any other; an empty cell is not that flow
    keys = np.ascontiguousarray(flows[idx])
    sizes = sizes_u32(rng, n)
    absent = rng.integers(0, 256, (50, K), dtype=np.uint8)
    a = (3 * n) // 5
    cm.insert_keys(keys[:a], sizes[:a])
    view = cm.view()
    view.refresh(detach=True)
    orc.insert_keys(keys[:a], sizes[:a])
    want = recorded(orc, flows, absent)
    cm.insert_keys(keys[a:], sizes[a:])  # the handle moves on; the view does not
    assert_view_is(view, want, flows, absent)
    qd = view.query_many(torch.from_numpy(np.ascontiguousarray(np.concatenate([flows, absent]))).cuda())
    assert qd.is_cuda and np.array_equal(qd.cpu().numpy().view(np.uint64), want[2])
    cr, sr = view.heavy_hitters_rows_device()
    assert cr.is_cuda and sr.is_cuda
    assert tuple(cr.shape) == (len(want[0]), K + 4) and tuple(sr.shape) == (len(want[1]), K + 4)
    assert_same_list(rows_list(cr, K), want[0], "device count rows")
    assert_same_list(rows_list(sr, K), want[1], "device size rows")
    assert view.counters() == {"inserted": a, "dropped": 0, "unsupported": 0}
    C, _, FPc, _ = want[3]
    if K == 13:  # what the case is there for
        assert bool(((C == 0) & FPc.any(axis=1)).any()), "no cell with C == 0 under a live fingerprint"
        assert want[2][2] > 0, "the all-zero key owns no cell"
    if w == 4096:
        assert len(distinct_owners(want[3])) > 8192
        assert cm.dict_stats()["slots"] >= 1 << 16
    cm.flush()
    orc.insert_keys(keys[a:], sizes[a:])
    assert_same_state(cm, orc)
    got_c, got_s = lists_of(cm)
    assert_same_list(got_c, orc.heavy("count"), "handle count list")
    assert_same_list(got_s, orc.heavy("size"), "handle size list")
    view.close()
    cm.close()


def test_view_is_self_contained(gpu, oracle):
    """A 64-flow dictionary that part B grows and reclaims; then reclaim, reset and an import:
    after each the detached view still answers part A's state, without an error.  A reclaim
    neither remaps it nor keeps its flows alive; a plain view of the same handle is remapped
    by the reclaim, and stale after the reset, as ever."""
    from go2netspectra_amd import GnsError
    rng = np.random.default_rng(5)
    K = 16
    cm, orc = make_pair(oracle, 512, 2, K, st=3000, ct=8, max_flows=64)
    keys, flows, _ = zipf_keys(rng, 20_000, 300, K)
    sizes = sizes_u32(rng, 20_000)
    absent = rng.integers(0, 256, (50, K), dtype=np.uint8)
    cm.insert_keys(keys, sizes)
    view = cm.view()
    view.refresh(detach=True)
    orc.insert_keys(keys, sizes)
    want = recorded(orc, flows, absent)
    assert len(want[0]) > 0 and len(want[1]) > 0
    keys2, flows2, _ = zipf_keys(rng, 40_000, 4000, K, s=0.5)
    sizes2 = sizes_u32(rng, 40_000)
    d0 = cm.dict_stats()
    cm.insert_keys(keys2, sizes2)
    cm.flush()
    d1 = cm.dict_stats()
    assert d1["growths"] + d1["reclaims"] > d0["growths"] + d0["reclaims"]  # the records the refresh read were moved
    assert_view_is(view, want, flows, absent, "after more inserts")
    orc.insert_keys(keys2, sizes2)
    want_b = recorded(orc, flows2, absent)
    other = cm.export_state()
    other_counters = [cm.counters()[k] for k in ("inserted", "dropped", "unsupported")]
    plain = cm.view()
    plain.refresh()  # the same period, ids of the live dictionary
    cm.reclaim()
    assert_view_is(view, want, flows, absent, "after reclaim")
    assert_view_is(plain, want_b, flows2, absent, "plain view after reclaim")  # remapped with the buckets
    # the detached view names A's flows, and they are gone from the dictionary all the same
    live_b = len(distinct_owners(want_b[3]))
    assert len(np.unique(np.concatenate([distinct_owners(want[3]), distinct_owners(want_b[3])]), axis=0)) > live_b
    assert cm.dict_stats()["live"] == live_b
    cm.reset()
    assert_view_is(view, want, flows, absent, "after reset")
    with pytest.raises(GnsError, match="stale"):
        plain.heavy_hitters()
    with pytest.raises(GnsError, match="stale"):
        plain.export_state()
    assert lists_of(cm) == ([], [])
    cm.reclaim()
    ds = cm.dict_stats()
    assert ds["live"] == 0 and ds["claimed"] == 0  # none of A's flows is kept alive by the view
    assert_view_is(view, want, flows, absent, "after reset and reclaim")
    cm.import_state(*other, counters=other_counters)
    assert_view_is(view, want, flows, absent, "after import")
    assert view.counters() == {"inserted": 20_000, "dropped": 0, "unsupported": 0}
    assert_same_state(cm, orc)  # (and the handle is where the import put it)
    assert lists_of(cm) == (want_b[0], want_b[1])
    for x in (view, plain):
        x.close()
    cm.close()


def test_reader_thread_across_a_reset(gpu, oracle):
    """The window cycle: refresh detached, reset, insert the next window -- while a reader
    thread lists and queries the window that was just closed."""
    rng = np.random.default_rng(21)
    K, nwin, per = 16, 3, 150_000
    cm, _ = make_pair(oracle, 8192, 4, K, st=20_000, ct=50)
    keys, flows, _ = zipf_keys(rng, nwin * per, 30_000, K)
    sizes = sizes_u32(rng, nwin * per)
    q = np.ascontiguousarray(flows[:3000])
    wants = []
    seeds = np.random.default_rng(1).integers(0, 2**32, 4, dtype=np.uint64).astype(np.uint32)  # make_pair's
    for i in range(nwin):  # every window's oracle, once
        orc = oracle.CountMin(8192, 4, 20_000, 50, K, seeds)
        orc.insert_keys(keys[i * per:(i + 1) * per], sizes[i * per:(i + 1) * per])
        wants.append((orc.heavy("count"), orc.heavy("size"), np.array([orc.query(bytes(f)) for f in q], np.uint64)))
        assert len(wants[-1][0]) > 0
    cm.insert_keys(keys[:per], sizes[:per])
    views, threads, results, errors = [], [], [], []

    def reader(view, i):
        try:
            for _ in range(6):
                c, s = lists_of(view)
                results.append((i, c, s, view.query_many(q)))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    for i in range(2):
        view = cm.view()  # a fresh view per window
        view.refresh(detach=True)
        cm.reset()
        th = threading.Thread(target=reader, args=(view, i))
        th.start()
        lo = (i + 1) * per
        for b in range(lo, lo + per, 50_000):  # the next window, while the reader runs
            cm.insert_keys(keys[b:b + 50_000], sizes[b:b + 50_000])
        views.append(view)
        threads.append(th)
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(results) == 12
    for i, c, s, got_q in results:
        assert_same_list(c, wants[i][0], f"window {i} count list")
        assert_same_list(s, wants[i][1], f"window {i} size list")
        assert np.array_equal(got_q, wants[i][2]), f"window {i} queries"
    cm.flush()
    got_c, got_s = lists_of(cm)  # the handle holds the last window alone
    assert_same_list(got_c, wants[2][0], "handle count list")
    assert_same_list(got_s, wants[2][1], "handle size list")
    for v in views:
        v.close()
    cm.close()


def test_checkpoint_during_ingest(gpu, oracle, tmp_path):
    from go2netspectra_amd import GnsError, checkpoint
    rng = np.random.default_rng(8)
    K = 13
    cm, orc = make_pair(oracle, 1000, 3, K, st=3000, ct=8)
    keys, _, _ = zipf_keys(rng, 90_000, 2000, K)
    sizes = sizes_u32(rng, 90_000)
    a = 50_001
    cm.insert_keys(keys[:a], sizes[:a])
    view = cm.view()
    view.refresh(detach=True)
    errors = []

    def saver():
        try:
            checkpoint.save(view, tmp_path / "view.npz")
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=saver)
    th.start()
    for lo in range(a, 90_000, 10_000):  # keeps inserting
        cm.insert_keys(keys[lo:lo + 10_000], sizes[lo:lo + 10_000])
    th.join()
    assert not errors, errors
    orc.insert_keys(keys[:a], sizes[:a])
    meta, arrays = checkpoint.read(tmp_path / "view.npz")
    assert meta["class"] == "CountMin" and meta["counters"] == [a, 0, 0]
    assert meta == dict(checkpoint.describe(cm), counters=[a, 0, 0])
    assert_same_arrays([arrays[k] for k in STATE], orc.export(), "file")
    fresh, _ = make_pair(oracle, 1000, 3, K, st=3000, ct=8)
    checkpoint.restore(fresh, tmp_path / "view.npz")
    assert_same_state(fresh, orc)
    fresh.insert_keys(keys[a:], sizes[a:])
    fresh.flush()
    orc.insert_keys(keys[a:], sizes[a:])
    assert_same_state(fresh, orc)
    assert fresh.counters()["inserted"] == 90_000
    cm.flush()
    assert_same_state(cm, orc)
    view.refresh()  # plain: no counters, so no checkpoint
    with pytest.raises(GnsError):
        checkpoint.save(view, tmp_path / "plain.npz")
    for x in (view, cm, fresh):
        x.close()


def test_export_spans_more_than_two_pinned_chunks(gpu):
    """The view's export goes out through two 4 MiB pinned chunks; d=4, w=65536, K=37 make
    each fingerprint array 9.7 MB: three pieces, so the first chunk is used twice and the last
    piece is a short one.  The handle's own export takes another route (one copy), so the two
    agree only if every piece landed where it belongs."""
    from go2netspectra_amd import CountMin
    rng = np.random.default_rng(99)
    w, d, K = 65536, 4, 37
    seeds = rng.integers(0, 2**32, d, dtype=np.uint64).astype(np.uint32)
    cm = CountMin(w, d, 1000, 10, key_bytes=K, seeds=seeds)
    keys, _, _ = zipf_keys(rng, 60_000, 30_000, K, s=0.5)
    cm.insert_keys(keys, sizes_u32(rng, 60_000))
    view = cm.view()
    view.refresh(detach=True)
    want = cm.export_state()  # the same point: nothing is inserted after the refresh
    got = view.export_state()
    owned = np.flatnonzero(want[2].any(axis=1))
    assert len(owned) > 10_000 and owned.min() < w and owned.max() > 3 * w  # in the first and in the last piece
    assert_same_arrays(got, want, "detached")
    view.refresh()
    assert_same_arrays(view.export_state(), want, "plain")  # through the live dictionary
    view.close()
    cm.close()


def test_edges(gpu, oracle):
    from go2netspectra_amd import GnsError, _lib
    import torch
    rng = np.random.default_rng(13)
    K = 8
    cm, orc = make_pair(oracle, 256, 2, K, st=3000, ct=8)
    keys, flows, _ = zipf_keys(rng, 40_000, 400, K)
    sizes = sizes_u32(rng, 40_000)
    view = cm.view()
    for call in (view.heavy_hitters, lambda: view.query_many(flows[:4]), view.export_state, view.counters,
                 view.heavy_hitters_rows_device, lambda: view.query_many(torch.from_numpy(flows[:4].copy()).cuda())):
        with pytest.raises(GnsError, match="never refreshed"):
            call()
    # an empty sketch: an empty table, empty lists, zero answers
    view.refresh(detach=True)
    assert lists_of(view) == ([], [])
    cr, sr = view.heavy_hitters_rows_device()
    assert tuple(cr.shape) == (0, K + 4) and tuple(sr.shape) == (0, K + 4)
    assert not view.query_many(flows).any()
    assert not view.query_many(np.zeros((1, K), np.uint8)).any()
    assert all(not a.any() for a in view.export_state())
    assert view.counters() == {"inserted": 0, "dropped": 0, "unsupported": 0}
    cm.insert_keys(keys[:20_000], sizes[:20_000])
    orc.insert_keys(keys[:20_000], sizes[:20_000])
    want = recorded(orc, flows, flows[:0])
    assert len(want[0]) > 8 and len(want[1]) > 8
    assert lists_of(view) == ([], [])  # still the empty sketch
    # detached, then plain, then detached on one view
    view.refresh(detach=True)
    assert_view_is(view, want, flows, flows[:0], "detached")
    view.refresh()
    assert_view_is(view, want, flows, flows[:0], "plain")
    with pytest.raises(GnsError, match="counters"):
        view.counters()
    cr, sr = view.heavy_hitters_rows_device()  # the new readers on a plain snapshot
    assert_same_list(rows_list(cr, K), want[0], "plain device count rows")
    assert_same_list(rows_list(sr, K), want[1], "plain device size rows")
    qd = view.query_many(torch.from_numpy(np.ascontiguousarray(flows)).cuda())
    assert np.array_equal(qd.cpu().numpy().view(np.uint64), want[2])
    view.refresh(detach=True)
    assert_view_is(view, want, flows, flows[:0], "detached again")
    assert view.counters()["inserted"] == 20_000
    # capacity: a list longer than *n is reported and not written
    L, cap = _lib.load(), 5
    nc_full, ns_full = len(want[0]), len(want[1])
    crow = torch.full((nc_full, K + 4), 0xEE, dtype=torch.uint8, device="cuda")
    srow = torch.full((ns_full, K + 4), 0xEE, dtype=torch.uint8, device="cuda")
    nc, ns = ct.c_uint64(cap), ct.c_uint64(ns_full)
    assert L.gns_cm_view_heavy_rows(view._h, crow.data_ptr(), ct.byref(nc), srow.data_ptr(), ct.byref(ns)) == 0
    assert (nc.value, ns.value) == (nc_full, ns_full)
    assert bool((crow == 0xEE).all())
    assert_same_list(rows_list(srow, K), want[1], "size rows beside a short count buffer")
    nc, ns = ct.c_uint64(0), ct.c_uint64(0)
    assert L.gns_cm_view_heavy_rows(view._h, None, ct.byref(nc), None, ct.byref(ns)) == 0
    assert (nc.value, ns.value) == (nc_full, ns_full)
    # argument errors
    out = np.zeros(4, np.uint64)
    k = np.ascontiguousarray(flows[:4])
    kd = torch.from_numpy(k).cuda()
    od = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert L.gns_cm_view_query_device(view._h, kd.data_ptr(), K - 1, 4, od.data_ptr()) == _lib.GNS_E_ARG
    assert L.gns_cm_view_query_device(view._h, kd.data_ptr(), K, 4, None) == _lib.GNS_E_ARG
    assert L.gns_cm_view_query(view._h, k.ctypes.data, K - 1, 4, out.ctypes.data) == _lib.GNS_E_ARG
    assert L.gns_cm_view_heavy_rows(view._h, None, None, None, None) == _lib.GNS_E_ARG
    assert L.gns_cm_view_refresh_at(view._h, 2) == _lib.GNS_E_ARG
    # two detached views of one handle are independent
    cm.insert_keys(keys[20_000:], sizes[20_000:])
    orc.insert_keys(keys[20_000:], sizes[20_000:])
    later = cm.view()
    later.refresh(detach=True)
    want2 = recorded(orc, flows, flows[:0])
    assert want2[0] != want[0]
    assert_view_is(later, want2, flows, flows[:0], "second view")
    assert_view_is(view, want, flows, flows[:0], "first view")
    cm.reset()
    assert_view_is(later, want2, flows, flows[:0], "second view after reset")
    assert_view_is(view, want, flows, flows[:0], "first view after reset")
    for x in (view, later):
        x.close()
    cm.close()


CM_TASK = """
aggregator:
  types: ["sketch"]
  sketch:
    tasks:
      - {name: cm_src, skt_type: 0, flow_fields: [SrcIP], element_fields: [DstIP, SrcPort, DstPort, Protocol],
         width: 4096, depth: 2, size_thereshold: 100000, count_thereshold: 50}
"""


def test_task_and_manager(gpu, tmp_path):
    from go2netspectra_amd import CountMinView, HeaderBatch, Manager, checkpoint, parse_config
    rng = np.random.default_rng(55)
    n, cut = 40_000, 23_001
    t = random_tuples(rng, n, 3000, v6_frac=0.2)
    hdr = frames_from_tuples(t, rng, vlan_frac=0.2)
    ts = np.cumsum(rng.integers(0, 5000, n)).astype(np.int64)
    batch = lambda lo, hi: HeaderBatch(hdr[lo:hi], t["length"][lo:hi], ts[lo:hi])
    mgr = Manager(parse_config(CM_TASK), seeds=np.array([11, 22, 33, 44], np.uint32))
    task = mgr.tasks()[0]
    views = mgr.views()
    assert [type(v) for v in views] == [CountMinView]
    mgr.process(batch(0, cut))
    mgr.refresh_views(views, detach=True)
    want = mgr.snapshot()  # the same point: nothing was inserted in between
    task.save(tmp_path / "serial.npz")
    assert len(want["cm_src"].Count) > 0
    mgr.reset_all()  # the window boundary: the view stays readable
    mgr.process(batch(cut, n))
    got = mgr.snapshot_from_views(views)
    assert list(got) == ["cm_src"] and got["cm_src"] == want["cm_src"]
    assert mgr.snapshot()["cm_src"] != want["cm_src"]  # the live task counts the next window
    task.save_from(views[0], tmp_path / "from_view.npz")
    (m1, a1), (m2, a2) = checkpoint.read(tmp_path / "from_view.npz"), checkpoint.read(tmp_path / "serial.npz")
    assert m1 == m2 and sorted(a1) == sorted(a2)
    assert all(np.array_equal(a1[k], a2[k]) and a1[k].dtype == a2[k].dtype for k in a2)
    mgr.refresh_views(views)  # detach defaults to False: the plain snapshot of the new window
    assert mgr.snapshot_from_views(views) == mgr.snapshot()
    for v in views:
        v.close()
    task.sketch.close()
