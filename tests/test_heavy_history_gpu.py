"""The heavy-hitter history on the GPU (gns_hh_hist_*): every answer -- at every snapshot time,
between two, before the first and with no end time -- equals QueryHeavyHitters' SQL restated
over the rows the reference's sketch writer would have stored (heavy_history_truth.py), for
synthetic lists at every size boundary of the kernels, through Count-Min and SuperSpread
against the sequential oracles, from a snapshotter thread during ingest, after a restore, and
across two flow-disjoint histories.  Every comparison is exact."""
import ctypes as ct
import threading

import numpy as np
import pytest

from go2netspectra_amd import GnsError, HeavyHistory, SketchTask, _lib
from go2netspectra_amd.exact import HeavyHitter
from go2netspectra_amd.heavy_history import pack_rows
from heavy_history_truth import HeavyTruth
from helpers import assert_same_list, frames_from_tuples, random_tuples, sizes_u32, zipf_keys

pytestmark = pytest.mark.gpu

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
HLL_MASTER, RNG_SEED = 0x0123456789ABCDEF, 0x0DDBA11CAFEF00D5


def dev(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda()


def got(hist, type, threshold=0, limit=0, T=None):
    flows, vals = hist.heavy_hitters(type, threshold, limit, end_time=T)
    assert flows.dtype == np.uint8 and vals.dtype == np.uint64 and flows.shape == (len(vals), hist.key_bytes)
    return [(bytes(f), int(v)) for f, v in zip(flows, vals)]


def entries(flows, vals):
    return [(bytes(f), int(v)) for f, v in zip(flows, vals)]


def assert_history_is(hist, tr, types, what, limits=(1, 10), thresholds=()):
    """Every probe time x type: the whole list, each limit, the list length - 1, each threshold."""
    for T in tr.probe_times():
        for type in types:
            full = tr.query_bytes(type, end_time=T)
            assert_same_list(got(hist, type, T=T), full, f"{what} type {type} T {T}")
            for limit in tuple(limits) + ((len(full) - 1,) if len(full) > 1 else ()):
                assert_same_list(got(hist, type, 0, limit, T), tr.query_bytes(type, limit, 0, T),
                                 f"{what} type {type} T {T} limit {limit}")
            for thr in thresholds:
                assert_same_list(got(hist, type, thr, 0, T), tr.query_bytes(type, 0, thr, T),
                                 f"{what} type {type} T {T} threshold {thr}")
                assert_same_list(got(hist, type, thr, 10, T), tr.query_bytes(type, 10, thr, T),
                                 f"{what} type {type} T {T} threshold {thr} limit 10")


# --- 1. synthetic rows, every boundary ---
LENGTHS = {0: [4096, 1, 63, 4097, 65, 256], 3: [0, 64, 257, 0, 4096, 1]}  # per type, over the six snapshots
TS6 = [-(1 << 40), -7, 0, 3, 1 << 33, (1 << 62) + 5]


@pytest.mark.parametrize("K", [1, 4, 13, 16, 37])
def test_synthetic_rows_every_boundary(gpu, K):
    """Strides 5, 8, 17, 20 and 41; list lengths 0, 1, 63, 64, 65, 256, 257, 4096, 4097 over six
    snapshots (K = 1 has only 256 flows: its lists stop at 256 rows); half of each list repeats
    earlier flows; max_rows = max_flows = 64, so the log and the index grow several times."""
    rng = np.random.default_rng(100 + K)
    pool = np.unique(rng.integers(0, 256, (20_000 if K > 1 else 4000, K), dtype=np.uint8), axis=0)
    pool = pool[rng.permutation(len(pool))]
    hist = HeavyHistory(K, max_rows=64, max_flows=64)
    tr = HeavyTruth(decode=bytes.hex)
    fresh_at, used = 0, np.zeros(len(pool), bool)
    assert got(hist, 0) == [] and hist.times() == []
    for s, t in enumerate(TS6):
        lists, want = {}, {}
        for type, lens in LENGTHS.items():
            n = min(lens[s], len(pool))
            old = np.flatnonzero(used)
            n_old = min(n // 2, len(old))
            n_new = min(n - n_old, len(pool) - fresh_at)
            n_old = n - n_new
            idx = np.concatenate([rng.choice(old, n_old, replace=False) if n_old else np.zeros(0, np.int64),
                                  np.arange(fresh_at, fresh_at + n_new)]).astype(np.int64)
            rng.shuffle(idx)
            flows = pool[idx]
            # few distinct values (ties), zeros, the largest u32, and wide values
            vals = np.where(rng.random(n) < 0.5, rng.integers(0, 6, n), rng.integers(0, 1 << 32, n)).astype(np.uint64)
            if n > 2:
                vals[0], vals[1] = 0xFFFFFFFF, 0
            if n or type == 0:
                lists[type] = (flows, vals.astype(np.uint32))
                want[type] = entries(flows, vals)
            used[idx] = True
            fresh_at += n_new
        # device rows and host rows take turns
        arg = {ty: dev(pack_rows(f, v, K)) for ty, (f, v) in lists.items()} if s % 2 == 0 else lists
        rows, new = hist.append(t, arg)
        before = {ty: set(tr.latest(ty)) for ty in lists}
        tr.record(t, want)
        assert rows == sum(len(v) for v in want.values())
        assert new == sum(len(set(tr.latest(ty)) - before[ty]) for ty in lists)
    assert hist.times() == TS6
    st = hist.stats()
    assert st["snapshots"] == 6 and st["rows"] == len(tr.rows) and st["lanes"] == 2
    assert st["keys"] == len(tr.latest(0)) + len(tr.latest(3))
    assert st["index_growths"] >= (2 if K > 1 else 1) and st["log_growths"] >= 2  # (K = 1: 256 flows, one growth)
    assert_history_is(hist, tr, (0, 3, 9), f"K {K}", thresholds=(3, 1 << 31))
    hist.close()


# --- 2. past one resolve piece ---
def test_past_one_resolve_piece(gpu):
    """Two snapshots of 2^20 + 5 rows each, half of the second's flows from the first: each list
    crosses kResolvePiece; one comes as device rows, one as host rows.  Truth by numpy."""
    K, N = 4, (1 << 20) + 5
    rng = np.random.default_rng(2)
    ids1 = rng.permutation(N).astype(np.uint32)
    ids2 = (rng.permutation(N) + N // 2).astype(np.uint32)
    v1 = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    v2 = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    keys = lambda ids: ids.astype(">u4").view(np.uint8).reshape(-1, 4)  # byte order == numeric order
    hist = HeavyHistory(K, max_rows=1 << 20, max_flows=1 << 19)
    assert hist.append(10, {0: dev(pack_rows(keys(ids1), v1, K))}) == (N, N)
    assert hist.append(20, {0: (keys(ids2), v2)}) == (N, N - (N - N // 2))
    latest1 = np.zeros(N + N // 2, np.uint64)
    latest1[ids1] = v1
    latest2 = latest1.copy()
    latest2[ids2] = v2
    for T, latest, nkeys in ((10, latest1, N), (15, latest1, N), (20, latest2, N + N // 2), (None, latest2, N + N // 2)):
        ids = np.arange(nkeys)
        order = np.lexsort((ids, -latest[:nkeys].astype(np.int64)))
        top = order[:100]
        want = list(zip([bytes(k) for k in keys(top.astype(np.uint32))], latest[top].tolist()))
        assert_same_list(got(hist, 0, 0, 100, T), want, f"T {T} limit 100")
        thr = (1 << 32) - (1 << 22)  # about a thousandth of the rows
        sel = order[latest[order] >= thr]
        assert 500 < len(sel) < 3000
        want = list(zip([bytes(k) for k in keys(sel.astype(np.uint32))], latest[sel].tolist()))
        assert_same_list(got(hist, 0, thr, 0, T), want, f"T {T} threshold")
    assert got(hist, 0, 0, 5, 9) == []
    st = hist.stats()
    assert st["rows"] == 2 * N and st["keys"] == N + N // 2 and st["index_growths"] >= 1 and st["log_growths"] >= 1
    hist.close()


# --- 3. ties ---
@pytest.mark.parametrize("K", [13, 37])
def test_ties_in_canonical_order(gpu, K):
    """1,000 rows of 3 distinct values whose keys agree in bytes 0..3: the limit falls inside a run
    of equal values, the cut value is the largest value (the top band of the select), and with
    every value equal the whole list is one run."""
    rng = np.random.default_rng(K)
    flows = np.zeros((1000, K), np.uint8)
    flows[:, :4] = [9, 9, 9, 9]
    tail = np.unique(rng.integers(0, 256, (3000, K - 4), dtype=np.uint8), axis=0)
    flows[:, 4:] = tail[rng.permutation(len(tail))[:1000]]
    vals = rng.choice(np.array([0xFFFFFFFF, 0xFFFFFFFE, 7], np.uint32), 1000)
    hist = HeavyHistory(K, max_rows=64, max_flows=64)
    tr = HeavyTruth(decode=bytes.hex)
    hist.append(1, {2: dev(pack_rows(flows, vals, K))})
    tr.record(1, {2: entries(flows, vals)})
    n_top = int((vals == 0xFFFFFFFF).sum())
    assert 100 < n_top < 900
    for limit in (1, n_top // 2, n_top - 1, n_top, n_top + 1, 999, 1000, 1001, 0):
        assert_same_list(got(hist, 2, 0, limit), tr.query_bytes(2, limit), f"limit {limit}")
    assert_same_list(got(hist, 2, 0xFFFFFFFF, 10), tr.query_bytes(2, 10, 0xFFFFFFFF), "threshold at the top value")
    hist.append(2, {2: dev(pack_rows(flows, np.full(1000, 5, np.uint32), K))})  # every value equal
    tr.record(2, {2: entries(flows, np.full(1000, 5))})
    for limit in (1, 500, 1000, 0):
        assert_same_list(got(hist, 2, 0, limit), tr.query_bytes(2, limit), f"all equal, limit {limit}")
    assert_same_list(got(hist, 2, 0, 300, 1), tr.query_bytes(2, 300, 0, 1), "as of the first snapshot")
    assert got(hist, 2, 6, 0) == []
    hist.close()


# --- 4. types ---
def test_types_are_independent_tables(gpu):
    K = 16
    hist = HeavyHistory(K)
    flow = np.arange(K, dtype=np.uint8).reshape(1, K)
    other = np.full((1, K), 200, np.uint8)
    tr = HeavyTruth(decode=bytes.hex)
    lists = {ty: (np.concatenate([flow, other]), np.array([v, 1000 - v], np.uint32))
             for ty, v in ((0, 10), (1, 20), (2, 30), (255, 40))}
    assert hist.append(5, {ty: dev(pack_rows(f, v, K)) for ty, (f, v) in lists.items()}) == (8, 8)
    tr.record(5, {ty: entries(f, v) for ty, (f, v) in lists.items()})
    assert hist.append(6, {1: (flow, np.array([1], np.uint32))}) == (1, 0)
    tr.record(6, {1: entries(flow, [1])})
    assert_history_is(hist, tr, (0, 1, 2, 255, 3, 254), "types", limits=(1,))
    assert got(hist, 1) == [(bytes(other[0]), 980), (bytes(flow[0]), 1)] and got(hist, 0)[1] == (bytes(flow[0]), 10)
    assert hist.stats()["lanes"] == 4 and hist.stats()["keys"] == 8
    # a type twice in one call: GNS_E_ARG, and nothing changes
    L, rows = _lib.load(), dev(pack_rows(flow, np.array([77], np.uint32), K))
    arr = (_lib.HhList * 2)()
    for i in range(2):
        arr[i].type, arr[i].rows, arr[i].n = 2, rows.data_ptr(), 1
    out = (ct.c_uint64 * 2)()
    assert L.gns_hh_hist_append(hist._h, 7, arr, 2, _lib.MEM_DEVICE, out) == _lib.GNS_E_ARG
    arr[1].type = 256
    assert L.gns_hh_hist_append(hist._h, 7, arr, 2, _lib.MEM_DEVICE, out) == _lib.GNS_E_ARG
    assert L.gns_hh_hist_append(None, 7, arr, 1, _lib.MEM_DEVICE, out) == _lib.GNS_E_ARG
    host = pack_rows(flow, np.array([77], np.uint32), K)  # host memory handed in as device rows
    arr[0].rows = host.ctypes.data
    assert L.gns_hh_hist_append(hist._h, 7, arr, 1, _lib.MEM_DEVICE, out) == _lib.GNS_E_ARG
    assert hist.times() == [5, 6]
    assert_history_is(hist, tr, (0, 1, 2, 255), "types after the rejections", limits=(1,))
    hist.close()


# --- 5. rejections change nothing ---
def test_rejected_appends_change_nothing(gpu):
    K = 13
    rng = np.random.default_rng(5)
    pool = np.unique(rng.integers(0, 256, (12_000, K), dtype=np.uint8), axis=0)
    hist = HeavyHistory(K, max_rows=64, max_flows=64)
    tr = HeavyTruth(decode=bytes.hex)
    f0, v0 = pool[:300], rng.integers(0, 1000, 300).astype(np.uint32)
    hist.append(100, {0: (f0, v0), 1: (f0[:7], v0[:7])})
    tr.record(100, {0: entries(f0, v0), 1: entries(f0[:7], v0[:7])})
    before = (hist.times(), [hist.stats()[k] for k in ("snapshots", "rows", "keys")])
    # a duplicate flow whose twin lies in another 4096-block of the list; most flows are new (the index grows)
    f1 = pool[200:5200].copy()
    f1[4500] = f1[3]
    v1 = rng.integers(0, 1000, 5000).astype(np.uint32)
    for arg in ({0: (f1, v1)}, {0: dev(pack_rows(f1, v1, K))}, {1: (f0[:5], v0[:5]), 0: dev(pack_rows(f1, v1, K)).cpu().numpy()}):
        with pytest.raises(GnsError, match="same flow") as e:
            hist.append(200, arg)
        assert e.value.code == _lib.GNS_E_ARG
    for t in (100, 99, -(1 << 63)):  # a stale timestamp
        with pytest.raises(GnsError, match="not after") as e:
            hist.append(t, {0: (f0[:3], v0[:3])})
        assert e.value.code == _lib.GNS_E_ARG
    with pytest.raises(ValueError, match=r"must be \[n, 17\]"):  # a wrong row width
        hist.append(200, {0: dev(np.zeros((4, K + 3), np.uint8))})
    assert (hist.times(), [hist.stats()[k] for k in ("snapshots", "rows", "keys")]) == before
    assert hist.stats()["index_growths"] >= 1  # (the key index may have grown)
    assert_history_is(hist, tr, (0, 1), "after the rejections")
    f1[4500] = pool[5300]  # the same list without the duplicate
    assert hist.append(200, {0: dev(pack_rows(f1, v1, K))}) == (5000, 4900)
    tr.record(200, {0: entries(f1, v1)})
    assert_history_is(hist, tr, (0, 1), "after a good append")
    hist.close()


# --- 6. / 7. the sketches through the engine ---
TSI = [1_000, 2_000, 2_001, 1 << 40]
FIELDS_OF_K = {4: ["SrcPort", "DstPort"], 37: FIVE}


def bare_task(sketch, K):
    """A SketchTask around a sketch built by key width (13 bytes are no field layout: that case
    is compared at the history, by key bytes)."""
    task = SketchTask.__new__(SketchTask)
    task.name_, task.sketch, task.flow_size, task.flow_fields = "t", sketch, K, FIELDS_OF_K.get(K, [])
    return task


def assert_task_is(task, tr, types, K):
    for T in tr.probe_times():
        for type in types:
            for limit in (1, 5, 1000):
                if K in FIELDS_OF_K:
                    want = [HeavyHitter(s, v) for s, v in tr.query(type, limit, 0, T)]
                    assert_same_list(task.query_heavy_hitters(type, limit, end_time=T), want, f"type {type} T {T} limit {limit}")
                else:
                    assert_same_list(got(task.heavy_history, type, 0, limit, T), tr.query_bytes(type, limit, 0, T),
                                     f"type {type} T {T} limit {limit}")
            assert task.query_heavy_hitters(type, 0, end_time=T) == []


def assert_some_flow_vanished(tr, type, last_list):
    """The no-tombstone rule is exercised: a flow listed before the reset is in no later list and
    is still answered, with its last listed value."""
    gone = set(tr.latest(type)) - {tr.decode(bytes(k)) for k, _ in last_list}
    assert gone, "no flow vanished from the list: choose another seed"
    return gone


@pytest.mark.parametrize("K", [4, 13, 37])
def test_count_min_through_the_engine(gpu, oracle, K):
    from test_cm_gpu import make_pair
    rng = np.random.default_rng(60 + K)
    cm, orc = make_pair(oracle, 64, 2, K, st=1, ct=1)
    task = bare_task(cm, K)
    hist = task.keep_heavy_history(max_rows=64, max_flows=64)
    assert task.keep_heavy_history() is hist
    tr = HeavyTruth(FIELDS_OF_K[K]) if K in FIELDS_OF_K else HeavyTruth(decode=bytes.hex)
    view = cm.view()
    flows = np.unique(rng.integers(0, 256, (400, K), dtype=np.uint8), axis=0)[:300]
    for i, t in enumerate(TSI):
        fl = flows[:150] if i < 2 else flows[150:]  # other flows after the reset: the old ones leave the list
        keys = np.ascontiguousarray(fl[zipf_keys(rng, 3000, len(fl), 1)[2]])
        sizes = sizes_u32(rng, 3000)
        cm.insert_keys(keys, sizes)
        orc.insert_keys(keys, sizes)
        if i % 2 == 0:
            out = task.record_heavy(t)  # the task's own view of the live handle
        else:
            view.refresh()
            out = task.record_heavy(t, view=view)
        tr.record_cm(t, orc)
        assert out[0] == len(orc.heavy("count")) + len(orc.heavy("size"))
        if i == 1:
            cm.reset()
            orc.reset()
    for type, which in ((0, "count"), (1, "size")):
        gone = assert_some_flow_vanished(tr, type, orc.heavy(which))
        assert gone & {s for s, _ in tr.query(type, 1000)}
    assert_task_is(task, tr, (0, 1), K)
    assert task.query_heavy_hitters(2, 10) == []  # a type without rows
    view.close()
    hist.close()
    cm.close()


@pytest.mark.parametrize("K", [4, 13, 37])
def test_superspread_through_the_engine(gpu, oracle, K):
    from test_ss_gpu import make_pair, spread_stream
    rng = np.random.default_rng(70 + K)
    ss, orc = make_pair(oracle, 64, 2, 16, 5, K, 4, thr=1)
    task = bare_task(ss, K)
    hist = task.keep_heavy_history(max_rows=64, max_flows=64)
    tr = HeavyTruth(FIELDS_OF_K[K]) if K in FIELDS_OF_K else HeavyTruth(decode=bytes.hex)
    view = ss.view()
    flows = np.unique(rng.integers(0, 256, (400, K), dtype=np.uint8), axis=0)[:300]
    for i, t in enumerate(TSI):
        fl = flows[:150] if i < 2 else flows[150:]
        idx = zipf_keys(rng, 3000, len(fl), 1)[2]
        f = np.ascontiguousarray(fl[idx])
        e = rng.integers(0, 256, (3000, 4), dtype=np.uint8)
        ss.insert_keys(f, e)
        orc.insert(f, e)
        if i % 2 == 0:
            out = task.record_heavy(t)
        else:
            view.refresh()
            out = task.record_heavy(t, view=view)
        tr.record_ss(t, orc)
        assert out[0] == len(orc.heavy()) > 0
        if i == 1:
            ss.reset()
            orc.reset()
    gone = assert_some_flow_vanished(tr, 2, orc.heavy())
    assert gone & {s for s, _ in tr.query(2, 1000)}
    assert_task_is(task, tr, (2,), K)
    assert task.query_heavy_hitters(0, 10) == [] and task.query_heavy_hitters(1, 10) == []
    view.close()
    hist.close()
    ss.close()


# --- 8. a snapshotter thread appends from views and queries while the main thread inserts ---
def test_snapshotter_thread_while_inserting(gpu, oracle):
    from test_cm_gpu import make_pair
    K, NI = 13, 6
    rng = np.random.default_rng(8)
    cm, orc = make_pair(oracle, 64, 2, K, st=1, ct=1)
    task = bare_task(cm, K)
    hist = task.keep_heavy_history(max_rows=64, max_flows=64)
    tr = HeavyTruth(decode=bytes.hex)
    views = [cm.view(), cm.view()]  # one is read by the snapshotter while the next is refreshed
    keys, _, _ = zipf_keys(rng, NI * 3000, 300, K)
    sizes = sizes_u32(rng, NI * 3000)
    ready, done = [threading.Semaphore(0) for _ in views], [threading.Semaphore(1) for _ in views]
    errors, seen = [], []

    def snapshotter():
        try:
            for i in range(NI):
                ready[i % 2].acquire()
                task.record_heavy(1000 + i, view=views[i % 2])
                done[i % 2].release()
                for T in (999, 1000, 1000 + i, None):  # whatever is appended so far is answered at once
                    seen.append((i, T, got(hist, 0, 0, 5, T), got(hist, 1, 0, 0, T)))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)
            for s in done:
                s.release()

    th = threading.Thread(target=snapshotter)
    th.start()
    try:
        for i in range(NI):
            part = slice(i * 3000, (i + 1) * 3000)
            cm.insert_keys(keys[part], sizes[part])
            orc.insert_keys(keys[part], sizes[part])
            done[i % 2].acquire()  # the snapshotter has read this view's previous refresh
            views[i % 2].refresh()  # on the ingest thread; the handle keeps inserting while it is read
            tr.record_cm(1000 + i, orc)
            ready[i % 2].release()
    finally:
        for s in ready:
            s.release()
        th.join()
    assert not errors, errors
    assert len(seen) == 4 * NI and hist.times() == [1000 + i for i in range(NI)]
    for i, T, count5, size_all in seen:
        # the truth holds later snapshots by now: bound the time by what the thread had appended
        Tq = 1000 + i if T is None else T
        assert_same_list(count5, tr.query_bytes(0, 5, 0, Tq), f"reader after {i} T {T} count")
        assert_same_list(size_all, tr.query_bytes(1, 0, 0, Tq), f"reader after {i} T {T} size")
    assert_history_is(hist, tr, (0, 1), "after the writer")
    for v in views:
        v.close()
    hist.close()
    cm.close()


# --- 9. restore ---
def assert_same_history(a, b, tr_times):
    assert a.times() == b.times() == tr_times
    for x, y in zip(a.export_log(), b.export_log()):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    for T in [tr_times[0] - 1] + tr_times + [None]:
        for type in (0, 1, 2, 9):
            for limit in (0, 3):
                assert got(a, type, 0, limit, T) == got(b, type, 0, limit, T), (T, type, limit)


def test_save_and_restore(gpu, tmp_path):
    K = 16
    rng = np.random.default_rng(9)
    pool = np.unique(rng.integers(0, 256, (3000, K), dtype=np.uint8), axis=0)
    hist = HeavyHistory(K, max_rows=64, max_flows=64)
    tr = HeavyTruth(decode=bytes.hex)
    times = [-50, -3, 0, 10, 11]
    for s, t in enumerate(times):
        lists = {}
        for type, n in ((0, 700), (1, 0 if s == 2 else 90), (2, 5 if s == 3 else 0)):
            if s == 1:
                continue  # an empty snapshot: only its timestamp
            idx = rng.choice(len(pool), n, replace=False)
            lists[type] = (pool[idx], rng.integers(0, 50, n).astype(np.uint32))
        hist.append(t, lists)
        tr.record(t, {ty: entries(f, v) for ty, (f, v) in lists.items()})
    ty, fl, va, wr, ts = hist.export_log()
    assert ts.tolist() == times and len(ty) == len(tr.rows) == hist.stats()["rows"]
    assert np.all(np.diff(ty.astype(int)) >= 0) and all(np.all(np.diff(wr[ty == t].astype(int)) >= 0) for t in (0, 1, 2))
    want = sorted((ty_, s, bytes.fromhex(f), v) for s, (t, ty_, f, v) in
                  ((times.index(r[0]), r) for r in tr.rows))
    assert sorted(zip(ty.tolist(), wr.tolist(), [bytes(f) for f in fl], va.tolist())) == want
    hist.save(tmp_path / "h.npz")
    back = HeavyHistory(K)
    back.restore(tmp_path / "h.npz")
    assert_same_history(hist, back, times)
    assert_history_is(back, tr, (0, 1, 2), "restored", limits=(3,))
    with pytest.raises(ValueError, match="not empty"):
        back.restore(tmp_path / "h.npz")
    with pytest.raises(ValueError, match="16-byte flows"):
        HeavyHistory(4).restore(tmp_path / "h.npz")
    hist.close()
    back.close()


CM_AND_SS = """
aggregator:
  types: ["sketch"]
  sketch:
    tasks:
      - {name: cm_src, skt_type: 0, flow_fields: [SrcIP], element_fields: [DstIP, SrcPort, DstPort, Protocol],
         width: 256, depth: 2, size_thereshold: 2000, count_thereshold: 5}
      - {name: ss_src, skt_type: 1, flow_fields: [SrcIP, Protocol], element_fields: [DstIP], width: 256, depth: 2,
         count_thereshold: 1, m: 16, size: 5, b: 1.08, base: 0.5}
"""


def test_manager_checkpoint_round_trip(gpu, tmp_path):
    import os
    from go2netspectra_amd import HeaderBatch, Manager, parse_config
    rng = np.random.default_rng(91)
    n = 12_000
    t = random_tuples(rng, n, 1500, v6_frac=0.2)
    hdr = frames_from_tuples(t, rng)
    kw = dict(seeds=np.array([11, 22, 33, 44], np.uint32), hll_master=HLL_MASTER, rng_seed=RNG_SEED)
    first, second, bare = (Manager(parse_config(CM_AND_SS), **kw) for _ in range(3))
    hists = first.keep_heavy_history(max_rows=64, max_flows=64)
    assert list(hists) == ["cm_src", "ss_src"] and first.keep_heavy_history() == hists
    truths = {"cm_src": HeavyTruth(["SrcIP"]), "ss_src": HeavyTruth(["SrcIP", "Protocol"])}
    times = [100, 200, 300]
    for i, ts in enumerate(times):
        first.process(HeaderBatch(hdr[i * 4000:(i + 1) * 4000], t["length"][i * 4000:(i + 1) * 4000]))
        snap = first.snapshot()  # the lists at this point (their parity with the oracle: test_cm_gpu, test_ss_gpu)
        out = first.record_heavy(ts)
        cm, ss = snap["cm_src"], snap["ss_src"]
        truths["cm_src"].record(ts, {0: [(h.Flow, h.Count) for h in cm.Count], 1: [(h.Flow, h.Size) for h in cm.Size]})
        truths["ss_src"].record(ts, {2: [(h.Flow, h.Count) for h in ss.Count]})
        assert out == {"cm_src": (len(cm.Count) + len(cm.Size), out["cm_src"][1]), "ss_src": (len(ss.Count), out["ss_src"][1])}
        assert len(cm.Count) > 0 and len(ss.Count) > 0
        if i == 1:
            first.reset_all()

    def check(mgr):
        for task in mgr.tasks():
            tr = truths[task.name()]
            for T in tr.probe_times():
                for type in (0, 1, 2):
                    want = [HeavyHitter(s, v) for s, v in tr.query(type, 7, 0, T)]
                    assert_same_list(task.query_heavy_hitters(type, 7, end_time=T), want, f"{task.name()} type {type} T {T}")
    check(first)
    paths = first.checkpoint(str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ["cm_src.npz", "ss_src.npz", "cm_src.heavy.npz", "ss_src.heavy.npz"]
    second.keep_heavy_history()
    second.restore(str(tmp_path))
    check(second)
    for a, b in zip(first.tasks(), second.tasks()):
        assert_same_history(a.heavy_history, b.heavy_history, times)
    bare.restore(str(tmp_path))  # no heavy history attached: the file is left alone
    assert all(getattr(task, "heavy_history", None) is None for task in bare.tasks())
    with pytest.raises(ValueError, match="keep_heavy_history"):
        bare.tasks()[0].query_heavy_hitters(0, 5)
    for mgr in (first, second, bare):
        for task in mgr.tasks():
            if getattr(task, "heavy_history", None) is not None:
                task.heavy_history.close()
            task.sketch.close()


# --- 10. the multi-GPU hand-off: flow-disjoint histories, merged by gns_hh_order_rows ---
def test_rows_of_disjoint_histories_merge(gpu):
    import torch
    K = 13
    rng = np.random.default_rng(10)
    pool = np.unique(rng.integers(0, 256, (5000, K), dtype=np.uint8), axis=0)
    parts = [pool[:2000], pool[2000:4000]]  # what two GPUs own
    hists = [HeavyHistory(K, max_rows=64, max_flows=64) for _ in parts]
    tr = HeavyTruth(decode=bytes.hex)
    for s, t in enumerate((10, 20, 30)):
        want = []
        for h, part in zip(hists, parts):
            idx = rng.choice(len(part), 600, replace=False)
            vals = rng.integers(0, 40, 600).astype(np.uint32)
            h.append(t, {0: dev(pack_rows(part[idx], vals, K))})
            want += entries(part[idx], vals)
        tr.record(t, {0: want})
    L = _lib.load()
    for T in (9, 10, 25, None):
        for thr, limit in ((0, 0), (30, 0), (0, 50)):
            rows = torch.cat([h.heavy_hitters_rows_device(0, thr, limit, end_time=T) for h in hists])
            assert rows.is_cuda and rows.dtype == torch.uint8 and rows.shape[1] == K + 4
            out = torch.empty_like(rows)
            _lib.device_ready(rows)
            _lib.check(L.gns_hh_order_rows(rows.data_ptr(), K, rows.shape[0], out.data_ptr(), 0))
            merged = [(bytes(r[:K]), int(np.frombuffer(bytes(r[K:]), "<u4")[0])) for r in out.cpu().numpy()]
            if limit:
                merged = merged[:limit]  # each GPU's first `limit` rows hold the union's first `limit`
            assert_same_list(merged, tr.query_bytes(0, limit, thr, T), f"T {T} threshold {thr} limit {limit}")
    for h in hists:
        h.close()
