"""Retention and point queries of the heavy-hitter history on the GPU (gns_hh_hist_trim /
gns_hh_hist_query): after a drop every answer equals QueryHeavyHitters' SQL over the table without
the expired rows, after a fold over the table whose expired rows became one base snapshot
(heavy_history_trim_truth.py), at every cut of a six-snapshot table with lists at every size
boundary, past one block and one scan step, across lanes, chained with appends, through save /
restore and the Manager's checkpoint, through Count-Min and SuperSpread with ``retain``, and from
a reader thread during retained records.  Every comparison is exact."""
import ctypes as ct
import threading

import numpy as np
import pytest

from go2netspectra_amd import HeavyHistory, _lib
from go2netspectra_amd.exact import HeavyHitter
from go2netspectra_amd.heavy_history import pack_rows
from heavy_history_trim_truth import assert_fold_keeps_answers, log_of, trim_out, trimmed
from heavy_history_truth import HeavyTruth
from helpers import assert_same_list, sizes_u32, zipf_keys

pytestmark = pytest.mark.gpu

LENGTHS = {0: [4096, 1, 63, 4097, 65, 256], 3: [0, 64, 257, 0, 4096, 1]}  # per type, over the six snapshots
TS6 = [-(1 << 40), -7, 0, 3, 1 << 33, (1 << 62) + 5]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def entries(flows, vals):
    return [(bytes(f), int(v)) for f, v in zip(flows, vals)]


# --- comparing a history with a truth, in numpy (the lists are long and the checks are many) ---
def truth_list(tr, type, T, K):
    rows = tr.query_bytes(type, end_time=T)
    fl = np.frombuffer(b"".join(k for k, _ in rows), np.uint8).reshape(-1, K)
    return fl, np.array([v for _, v in rows], np.uint64)


def assert_answers(hist, tr, types, what, limits=(1, 10), thresholds=(3,)):
    """Every probe time x type: the whole list, each limit, the list length - 1, each threshold
    alone and with a limit.  A limit is a prefix of the truth's ordered list, a threshold a filter."""
    K = hist.key_bytes
    for T in tr.probe_times():
        for type in types:
            fl, va = truth_list(tr, type, T, K)
            cases = [(0, 0)] + [(0, l) for l in limits] + ([(0, len(va) - 1)] if len(va) > 1 else [])
            cases += [(t, 0) for t in thresholds] + [(t, 10) for t in thresholds]
            for thr, limit in cases:
                f, v = hist.heavy_hitters(type, thr, limit, end_time=T)
                sel = va >= thr
                wf, wv = (fl[sel][:limit], va[sel][:limit]) if limit else (fl[sel], va[sel])
                assert v.dtype == np.uint64 and np.array_equal(v, wv) and np.array_equal(f, wf), \
                    f"{what}: type {type} T {T} threshold {thr} limit {limit}"


def assert_log(hist, tr, types, what):
    """times, the three stats the truth knows, and the exported log, row by row in log order."""
    assert hist.times() == tr.times, what
    st = hist.stats()
    assert st["snapshots"] == len(tr.times) and st["rows"] == len(tr.rows), what
    assert st["keys"] == len({(ty, s) for _, ty, s, _ in tr.rows}), what
    ty, fl, va, wr, ts = hist.export_log()
    assert ts.tolist() == tr.times and len(ty) == len(tr.rows), what
    assert np.all(np.diff(ty.astype(int)) >= 0), what
    for type in types:
        sel = ty == type
        got = list(zip(wr[sel].tolist(), [bytes(f) for f in fl[sel]], va[sel].tolist()))
        assert_same_list(got, log_of(tr, type), f"{what}: log of type {type}")
    assert set(np.unique(ty).tolist()) <= set(types), what


def assert_points(hist, tr, types, flows, what, device=False):
    """hist.query of `flows` (uint8 [n, K]) at every probe time x type against the truth's latest()."""
    for T in tr.probe_times():
        for type in types:
            latest = tr.latest(type, T)
            want = [latest.get(tr.decode(bytes(f))) for f in flows]
            if device:
                v, f = hist.query_device(type, dev(flows), end_time=T)
                v, f = v.cpu().numpy().view(np.uint64), f.cpu().numpy()
            else:
                v, f = hist.query(type, flows, end_time=T)
            assert v.dtype == np.uint64 and f.dtype == bool and len(v) == len(f) == len(flows)
            assert f.tolist() == [w is not None for w in want], f"{what}: found, type {type} T {T}"
            assert v.tolist() == [w or 0 for w in want], f"{what}: values, type {type} T {T}"


def state_of(hist, types=(0, 1, 3)):
    ans = [(T, ty, lim, [a.tobytes() for a in hist.heavy_hitters(ty, 0, lim, end_time=T)])
           for T in [None] + hist.times() for ty in types for lim in (0, 3)]
    return hist.times(), hist.stats(), [a.tobytes() for a in hist.export_log()], ans


# --- 1. every boundary ---
def six_snapshots(K):
    """The table of test_synthetic_rows_every_boundary: a truth and the history's exported log."""
    rng = np.random.default_rng(100 + K)
    pool = np.unique(rng.integers(0, 256, (20_000 if K > 1 else 4000, K), dtype=np.uint8), axis=0)
    pool = pool[rng.permutation(len(pool))]
    hist = HeavyHistory(K, max_rows=64, max_flows=64)
    tr = HeavyTruth(decode=bytes.hex)
    fresh_at, used = 0, np.zeros(len(pool), bool)
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
            vals = np.where(rng.random(n) < 0.5, rng.integers(0, 6, n), rng.integers(0, 1 << 32, n)).astype(np.uint64)
            if n > 2:
                vals[0], vals[1] = 0xFFFFFFFF, 0
            if n or type == 0:
                lists[type] = (flows, vals.astype(np.uint32))
                want[type] = entries(flows, vals)
            used[idx] = True
            fresh_at += n_new
        hist.append(t, {ty: dev(pack_rows(f, v, K)) for ty, (f, v) in lists.items()} if s % 2 == 0 else lists)
        tr.record(t, want)
    return hist, tr, pool


_SIX = {}


@pytest.fixture
def six(gpu, tmp_path_factory):
    def get(K):
        if K not in _SIX:
            hist, tr, pool = six_snapshots(K)
            path = tmp_path_factory.mktemp("six") / f"k{K}.npz"
            hist.save(path)
            hist.close()
            _SIX[K] = (path, tr, pool)
        return _SIX[K]
    return get


def restored(path, K):
    hist = HeavyHistory(K, max_rows=64, max_flows=64)
    hist.restore(path)
    return hist


def cuts_of(times):
    out = [times[0] - 1]
    for i, t in enumerate(times):
        out.append(t)
        if i + 1 < len(times):
            out.append(t + (times[i + 1] - t) // 2)
    return out + [times[-1] + 1]


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("K", [1, 13, 37])
def test_trim_at_every_boundary(six, K, fold):
    """`before` at each snapshot time, between each two, below the first and above the last; each
    trim starts from a history restored from the same exported log."""
    path, tr, _ = six(K)
    for before in cuts_of(TS6):
        hist = restored(path, K)
        slots = hist.stats()["index_slots"]
        out = hist.trim(before, fold=fold)
        ttr = trimmed(tr, before, fold)
        what = f"K {K} fold {fold} before {before}"
        assert [out[k] for k in HeavyHistory.TRIM] == trim_out(tr, before, fold), what
        assert_log(hist, ttr, (0, 3), what)
        assert_answers(hist, ttr, (0, 3, 9), what, thresholds=(3, 1 << 31))
        st = hist.stats()
        assert st["lanes"] == 2 and st["index_slots"] <= slots, what
        if fold:
            if before in (TS6[2], TS6[5] + 1):
                assert_fold_keeps_answers(tr, ttr, (0, 3))
            assert out["pairs_forgotten"] == 0 and st["index_slots"] == slots, what
        hist.close()


# --- 2. compaction past one block and one scan step ---
def keys_of(ids):
    return np.ascontiguousarray(ids.astype(">u4")).view(np.uint8).reshape(-1, 4)  # byte order == numeric order


@pytest.mark.parametrize("fold", [False, True])
def test_compaction_past_one_scan_tile(gpu, fold):
    """One lane whose expired prefix holds 2^18 + 3 rows -- 1,025 blocks of 256, one more than a
    scan tile -- over three snapshots; snapshot 1 re-lists whole 256-row blocks of snapshot 0 (no
    row of them stays), leaves others alone and takes a random half of the rest; snapshot 2 re-lists
    a random part of 0 and 1 but for every eighth block of 0 (every row of those stays).  Truth by numpy."""
    K, N0, N1, N2, N3 = 4, 1 << 17, (1 << 16) + 3, 1 << 16, 5000
    rng = np.random.default_rng(22)
    ids0 = rng.permutation(N0).astype(np.uint32)
    blk = np.arange(N0) // 256
    pick = np.where(blk % 4 == 0, True, np.where(blk % 4 == 1, False, rng.random(N0) < 0.5))
    cand = ids0[pick]
    ids1 = np.concatenate([cand[:N1 - 1000], np.arange(N0, N0 + 1000, dtype=np.uint32)])  # some new flows too
    assert len(cand) >= N1 - 1000 and np.all(pick[:256]) and not np.any(pick[256:512])
    ids1 = ids1[rng.permutation(N1)]
    quiet = np.concatenate([ids0[blk % 8 != 1], np.arange(N0, N0 + 1000, dtype=np.uint32)])  # blocks 1, 9, ... stay whole
    ids2 = rng.choice(quiet, N2, replace=False).astype(np.uint32)
    ids3 = rng.choice(N0 + 2000, N3, replace=False).astype(np.uint32)
    lists = [ids0, ids1, ids2, ids3]
    vals = [rng.integers(0, 1 << 32, len(i), dtype=np.uint64).astype(np.uint32) for i in lists]
    times = [10, 20, 30, 40]
    hist = HeavyHistory(K, max_rows=1 << 17, max_flows=1 << 17)
    for s, (ids, v) in enumerate(zip(lists, vals)):
        hist.append(times[s], {0: dev(pack_rows(keys_of(ids), v, K))})
    M = N0 + 2000
    # the untrimmed truth: latest[s][id], -1 without a row
    latest, cur = [], np.full(M, -1, np.int64)
    for ids, v in zip(lists, vals):
        cur = cur.copy()
        cur[ids] = v
        latest.append(cur)
    out = hist.trim(40, fold=fold)
    pre_ids, pre_vals = np.concatenate(lists[:3]), np.concatenate(vals[:3])
    assert len(pre_ids) == (1 << 18) + 3
    if fold:  # of the prefix, each flow's last row stays, in log order
        last = np.zeros(len(pre_ids), bool)
        last[len(pre_ids) - 1 - np.unique(pre_ids[::-1], return_index=True)[1]] = True
        assert not np.any(last[:256]) and np.all(last[256:512])  # a block without a kept row, one with every row kept
        want_ids, want_vals = np.concatenate([pre_ids[last], ids3]), np.concatenate([pre_vals[last], vals[3]])
        want_wr = np.concatenate([np.zeros(int(last.sum()), np.uint32), np.ones(N3, np.uint32)])
        assert out == dict(snapshots_removed=2, rows_removed=int((~last).sum()), pairs_forgotten=0, rows=len(want_ids))
        want_times, at = [30, 40], {29: None, 30: latest[2], 35: latest[2], 40: latest[3], None: latest[3]}
    else:
        want_ids, want_vals, want_wr = ids3, vals[3], np.zeros(N3, np.uint32)
        gone = int((latest[3] >= 0).sum()) - N3
        assert out == dict(snapshots_removed=3, rows_removed=len(pre_ids), pairs_forgotten=gone, rows=N3)
        only3 = np.full(M, -1, np.int64)
        only3[ids3] = vals[3]
        want_times, at = [40], {39: None, 40: only3, None: only3}
    ty, fl, va, wr, ts = hist.export_log()
    assert ts.tolist() == want_times == hist.times()
    assert np.array_equal(fl, keys_of(want_ids)) and np.array_equal(va, want_vals) and np.array_equal(wr, want_wr)
    st = hist.stats()
    assert st["rows"] == len(want_ids) and st["keys"] == len(np.unique(want_ids)) and st["row_capacity"] < 2 * len(want_ids)
    probe = np.arange(M, dtype=np.uint32)
    for T, lat in at.items():
        v, f = hist.query(0, keys_of(probe), end_time=T)
        if lat is None:
            assert not f.any() and not v.any() and hist.heavy_hitters(0, 0, 5, end_time=T)[1].tolist() == []
            continue
        assert np.array_equal(f, lat >= 0) and np.array_equal(v, np.maximum(lat, 0).astype(np.uint64)), T
        have = np.flatnonzero(lat >= 0)
        order = have[np.lexsort((have, -lat[have]))][:100]
        f, v = hist.heavy_hitters(0, 0, 100, end_time=T)
        assert np.array_equal(f, keys_of(order.astype(np.uint32))) and np.array_equal(v, lat[order].astype(np.uint64)), T
    hist.close()


# --- small random tables for the tests below ---
def pool_of(K, n, seed):
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 256, (3 * n, K), dtype=np.uint8), axis=0)
    return pool[rng.permutation(len(pool))][:n]


def feed(hist, tr, t, lists, device=True):
    """One snapshot into both: lists = {type: (flows, vals)}.  Returns the append's result."""
    K = hist.key_bytes
    before = {ty: set(tr.latest(ty)) for ty in lists}
    out = hist.append(t, {ty: dev(pack_rows(f, v, K)) for ty, (f, v) in lists.items()} if device else lists)
    tr.record(t, {ty: entries(f, v) for ty, (f, v) in lists.items()})
    assert out == (sum(len(v) for _, v in lists.values()), sum(len(set(tr.latest(ty)) - before[ty]) for ty in lists))
    return out


def draw(rng, pool, n, lo=0, hi=None):
    idx = rng.choice(np.arange(lo, hi if hi is not None else len(pool)), n, replace=False)
    vals = rng.integers(0, 50, n).astype(np.uint32)
    if n > 1:
        vals[0], vals[1] = 0xFFFFFFFF, 0
    return pool[idx], vals


def trim_both(hist, tr, before, fold, what):
    out = hist.trim(before, fold=fold)
    assert [out[k] for k in HeavyHistory.TRIM] == trim_out(tr, before, fold), what
    return trimmed(tr, before, fold)


# --- 3. lanes ---
@pytest.mark.parametrize("fold", [False, True])
def test_a_lane_created_later_and_a_flow_in_two_lanes(gpu, fold):
    K = 13
    rng, pool = np.random.default_rng(3), pool_of(K, 900, 3)
    times = [10, 20, 30, 40, 50, 60]
    for before in (25, 30, 31, 40, 41, 55):  # before, at and after snapshot 3, where type 7's lane is created
        hist, tr = HeavyHistory(K, max_rows=64, max_flows=64), HeavyTruth(decode=bytes.hex)
        rng = np.random.default_rng(33)
        for s, t in enumerate(times):
            lists = {0: draw(rng, pool, 300)}
            if s >= 3:
                lists[7] = draw(rng, pool, 70 + s)
            feed(hist, tr, t, lists, device=s % 2 == 0)
        tr = trim_both(hist, tr, before, fold, f"before {before}")
        assert_log(hist, tr, (0, 7), f"before {before}")
        assert_answers(hist, tr, (0, 7, 1), f"before {before}")
        assert hist.stats()["lanes"] == 2
        feed(hist, tr, 70, {0: draw(rng, pool, 200), 7: draw(rng, pool, 100), 1: draw(rng, pool, 5)})
        assert_log(hist, tr, (0, 1, 7), f"before {before}, appended")
        assert_answers(hist, tr, (0, 1, 7), f"before {before}, appended")
        hist.close()


def test_a_flow_dropped_from_one_of_two_lanes_and_an_emptied_history(gpu):
    K = 16
    pool = pool_of(K, 400, 4)
    hist, tr = HeavyHistory(K, max_rows=64, max_flows=64), HeavyTruth(decode=bytes.hex)
    both, v = pool[:50], np.arange(50, dtype=np.uint32)
    feed(hist, tr, 10, {1: (both, v + 1000)})
    feed(hist, tr, 20, {1: (both[:10], v[:10])})
    feed(hist, tr, 30, {0: (pool[:200], np.arange(200, dtype=np.uint32))})  # `both` among them; type 0's lane starts here
    before, type0 = hist.stats(), [a.tobytes() for a in hist.heavy_hitters(0)]
    assert before["keys"] == 250
    tr2 = trim_both(hist, tr, 30, False, "drop")
    # type 1 loses every row and forgets its 50 pairs; type 0 names the same flows, so their keys stay in the
    # index and its answers are what they were
    after = hist.stats()
    assert tr2.query(1) == [] and after["keys"] == 200 and trim_out(tr, 30, False) == [2, 60, 50, 200]
    assert [a.tobytes() for a in hist.heavy_hitters(0)] == type0
    assert_log(hist, tr2, (0, 1), "drop")
    assert_answers(hist, tr2, (0, 1), "drop")
    assert_points(hist, tr2, (0, 1), pool[:60], "drop")
    assert after["lanes"] == 2 and after["index_slots"] == 512 <= before["index_slots"]  # hist_index_slots(200)
    # drop everything: the lanes still work, and every pair of the next append is new
    out = hist.clear()
    assert [out[k] for k in HeavyHistory.TRIM] == [1, 200, 200, 0]
    st = hist.stats()
    assert hist.times() == [] and st["rows"] == st["keys"] == st["snapshots"] == 0 and st["lanes"] == 2
    assert st["row_capacity"] == 0 and st["index_slots"] == 64
    assert hist.heavy_hitters(0)[1].tolist() == [] and not hist.query(0, pool[:5])[1].any()
    tr3 = HeavyTruth(decode=bytes.hex)
    assert feed(hist, tr3, -5, {0: (pool[:300], np.arange(300, dtype=np.uint32)), 1: (both, v)}) == (350, 350)
    assert_log(hist, tr3, (0, 1), "refilled")
    assert_answers(hist, tr3, (0, 1), "refilled")
    hist.close()


# --- 4. forgetting ---
def test_drop_shrinks_the_index_and_fold_does_not(gpu):
    K = 37
    rng, pool = np.random.default_rng(5), pool_of(K, 6000, 5)

    def filled():
        hist, tr = HeavyHistory(K, max_rows=64, max_flows=64), HeavyTruth(decode=bytes.hex)
        for s in range(4):  # disjoint thirds of the pool, then a part of everything
            lo, hi = (s * 2000, (s + 1) * 2000) if s < 3 else (0, 6000)
            feed(hist, tr, 10 * (s + 1), {0: draw(rng, pool, 1500, lo, hi), 2: draw(rng, pool, 100, lo, hi)})
        return hist, tr
    hist, tr = filled()
    before = hist.stats()
    out = hist.trim(30, fold=False)
    after = hist.stats()
    assert out["pairs_forgotten"] > 1000 and after["keys"] == before["keys"] - out["pairs_forgotten"]
    assert after["index_slots"] < before["index_slots"] and after["row_capacity"] < before["row_capacity"]
    tr = trimmed(tr, 30, False)
    assert_log(hist, tr, (0, 2), "drop")
    gone = pool[:10]
    assert_points(hist, tr, (0, 2), np.concatenate([gone, pool[4000:4050]]), "drop")
    # a forgotten pair that is appended again counts as new
    back = (pool[:2000], np.arange(2000, dtype=np.uint32))
    new = len({bytes(f).hex() for f in back[0]} - set(tr.latest(0)))
    assert feed(hist, tr, 50, {0: back}) == (2000, new) and new > 1000
    assert_answers(hist, tr, (0, 2), "drop, appended")
    hist.close()
    hist, tr = filled()
    before = hist.stats()
    out = hist.trim(41, fold=True)  # (the last list re-listed a part of every earlier one: those rows go)
    after = hist.stats()
    assert out["pairs_forgotten"] == 0 and after["keys"] == before["keys"] and after["index_slots"] == before["index_slots"]
    assert after["rows"] == out["rows"] == after["keys"] < before["rows"] and after["snapshots"] == 1
    assert_log(hist, trimmed(tr, 41, True), (0, 2), "fold")
    hist.close()


# --- 5. trim, append, trim, append; save / restore; the Manager's checkpoint ---
def same_history(a, b):
    assert a.times() == b.times()
    for x, y in zip(a.export_log(), b.export_log()):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    for T in [None] + a.times():
        for type in (0, 1, 2, 9):
            for limit in (0, 3):
                for x, y in zip(a.heavy_hitters(type, 0, limit, end_time=T), b.heavy_hitters(type, 0, limit, end_time=T)):
                    assert np.array_equal(x, y), (T, type, limit)


@pytest.mark.parametrize("order", [(False, True), (True, False), (True, True), (False, False)])
def test_trim_append_trim_append_and_restore(gpu, tmp_path, order):
    K = 4
    rng, pool = np.random.default_rng(6), pool_of(K, 1500, 6)
    hist, tr = HeavyHistory(K, max_rows=64, max_flows=64), HeavyTruth(decode=bytes.hex)
    t = 0
    for step, fold in enumerate(order):
        for _ in range(3):
            t += 10
            feed(hist, tr, t, {0: draw(rng, pool, 400), 1: draw(rng, pool, 30)} if t != 20 else {}, device=t % 20 == 0)
        tr = trim_both(hist, tr, t - 5 if step == 0 else t, fold, f"step {step}")
        assert_log(hist, tr, (0, 1), f"step {step}")
        assert_answers(hist, tr, (0, 1, 2), f"step {step}")
        assert_points(hist, tr, (0, 1), pool[:200], f"step {step}")
    t += 10
    feed(hist, tr, t, {0: draw(rng, pool, 400), 2: draw(rng, pool, 9)})
    assert_log(hist, tr, (0, 1, 2), "end")
    assert_answers(hist, tr, (0, 1, 2), "end")
    hist.save(tmp_path / "h.npz")
    back = HeavyHistory(K)
    back.restore(tmp_path / "h.npz")
    same_history(hist, back)
    assert_log(back, tr, (0, 1, 2), "restored")
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


@pytest.mark.parametrize("drop", [False, True])
def test_manager_checkpoint_round_trip_with_retain(gpu, tmp_path, drop):
    from go2netspectra_amd import HeaderBatch, Manager, parse_config
    from helpers import frames_from_tuples, random_tuples
    rng = np.random.default_rng(91)
    t = random_tuples(rng, 16_000, 1500, v6_frac=0.2)
    hdr = frames_from_tuples(t, rng)
    kw = dict(seeds=np.array([11, 22, 33, 44], np.uint32), hll_master=0x0123456789ABCDEF, rng_seed=0x0DDBA11CAFEF00D5)
    first, second = (Manager(parse_config(CM_AND_SS), **kw) for _ in range(2))
    hists = first.keep_heavy_history(retain=2, drop=drop, max_rows=64, max_flows=64)
    truths = {"cm_src": HeavyTruth(["SrcIP"]), "ss_src": HeavyTruth(["SrcIP", "Protocol"])}
    times = [100, 200, 300, 400]
    for i, ts in enumerate(times):
        first.process(HeaderBatch(hdr[i * 4000:(i + 1) * 4000], t["length"][i * 4000:(i + 1) * 4000]))
        snap = first.snapshot()
        first.record_heavy(ts)
        cm, ss = snap["cm_src"], snap["ss_src"]
        truths["cm_src"].record(ts, {0: [(h.Flow, h.Count) for h in cm.Count], 1: [(h.Flow, h.Size) for h in cm.Size]})
        truths["ss_src"].record(ts, {2: [(h.Flow, h.Count) for h in ss.Count]})
        for name, tr in truths.items():
            if len(tr.times) > 2:
                truths[name] = trimmed(tr, window_cut(tr.times, 2, drop), not drop)
        if i == 1:
            first.reset_all()

    def check(mgr):
        for task in mgr.tasks():
            tr = truths[task.name()]
            assert task.heavy_history.times() == tr.times == times[2:]
            for T in tr.probe_times():
                for type in (0, 1, 2):
                    want = [HeavyHitter(s, v) for s, v in tr.query(type, 7, 0, T)]
                    assert_same_list(task.query_heavy_hitters(type, 7, end_time=T), want, f"{task.name()} type {type} T {T}")
    check(first)
    first.checkpoint(str(tmp_path))
    second.keep_heavy_history(retain=2, drop=drop)
    second.restore(str(tmp_path))
    check(second)
    for a, b in zip(first.tasks(), second.tasks()):
        same_history(a.heavy_history, b.heavy_history)
    for mgr in (first, second):
        for task in mgr.tasks():
            task.heavy_history.close()
            task.sketch.close()
    assert list(hists) == ["cm_src", "ss_src"]


# --- 6. rejections and no-ops change nothing ---
def test_rejected_trims_and_noops_change_nothing(gpu):
    K = 13
    rng, pool = np.random.default_rng(7), pool_of(K, 800, 7)
    hist, tr = HeavyHistory(K, max_rows=64, max_flows=64), HeavyTruth(decode=bytes.hex)
    for t in (10, 20, 30):
        feed(hist, tr, t, {0: draw(rng, pool, 300), 1: draw(rng, pool, 40), 3: draw(rng, pool, 3)})
    before = state_of(hist)
    L, out = _lib.load(), (ct.c_uint64 * 4)(9, 9, 9, 9)
    for bad in (2, -1, 7):
        assert L.gns_hh_hist_trim(hist._h, 25, bad, out) == _lib.GNS_E_ARG
    assert L.gns_hh_hist_trim(None, 25, 0, out) == _lib.GNS_E_ARG and list(out) == [9, 9, 9, 9]
    with pytest.raises(ValueError, match="fold"):
        hist.trim(25, fold=2)
    rows = hist.stats()["rows"]
    for b, fold in ((10, False), (9, False), (-(1 << 63), False), (10, True), (11, True), (20, True), (5, True)):
        assert [hist.trim(b, fold=fold)[k] for k in HeavyHistory.TRIM] == [0, 0, 0, rows], (b, fold)  # c == 0; c == 1 under fold
    assert L.gns_hh_hist_trim(hist._h, 5, 0, None) == _lib.GNS_OK
    # rejected queries: a null array, an unknown memory kind, host memory handed in as device memory
    flows, v, f = np.ascontiguousarray(pool[:4]), np.zeros(4, np.uint64), np.zeros(4, np.uint8)
    q = L.gns_hh_hist_query
    assert q(hist._h, None, 0, None, 4, _lib.MEM_HOST, v.ctypes.data, f.ctypes.data) == _lib.GNS_E_ARG
    assert q(hist._h, None, 0, flows.ctypes.data, 4, _lib.MEM_HOST, None, f.ctypes.data) == _lib.GNS_E_ARG
    assert q(hist._h, None, 0, flows.ctypes.data, 4, 77, v.ctypes.data, f.ctypes.data) == _lib.GNS_E_ARG
    assert q(hist._h, None, 0, flows.ctypes.data, 4, _lib.MEM_DEVICE, v.ctypes.data, f.ctypes.data) == _lib.GNS_E_ARG
    assert q(None, None, 0, flows.ctypes.data, 4, _lib.MEM_HOST, v.ctypes.data, f.ctypes.data) == _lib.GNS_E_ARG
    assert q(hist._h, None, 0, None, 0, _lib.MEM_HOST, None, None) == _lib.GNS_OK  # n == 0 is legal
    assert state_of(hist) == before
    assert_answers(hist, tr, (0, 1, 3), "after the rejections")
    hist.close()


# --- 7. point queries ---
@pytest.mark.parametrize("K", [4, 37])
def test_point_queries_before_and_after_trims(gpu, K):
    rng, pool = np.random.default_rng(70 + K), pool_of(K, 6000, 70 + K)
    hist, tr = HeavyHistory(K, max_rows=64, max_flows=64), HeavyTruth(decode=bytes.hex)
    for s, t in enumerate((-30, -20, 0, 5, 1 << 40)):
        lists = {0: draw(rng, pool, 1200, 0, 5000), 2: draw(rng, pool, 100 + s, 0, 5000)}
        if s == 1:
            del lists[2]
        feed(hist, tr, t, lists, device=s % 2 == 1)
    listed = np.array([np.frombuffer(b, np.uint8) for b in tr.bytes.values()])
    never = pool[5000:]
    assert len(listed) > 3000 and {v for _, _, _, v in tr.rows} >= {0, 0xFFFFFFFF}
    everything = np.concatenate([listed, never[:500], listed[:700][::-1], never[:3]])  # with duplicates of both kinds
    batches = [everything[:n] for n in (0, 1, 63, 64, 65, 4097)] + [np.concatenate([listed[:1]] * 5 + [never[:1]] * 3)]
    assert len(everything) >= 4097

    def check(tr, what):
        stats = hist.stats()
        assert_points(hist, tr, (0, 2, 9), everything, what)
        assert_points(hist, tr, (0, 2), everything, what + " (device)", device=True)
        for b in batches:
            assert_points(hist, tr, (0, 2), b, f"{what} batch {len(b)}")
            assert_points(hist, tr, (2,), b, f"{what} batch {len(b)} (device)", device=True)
        assert hist.stats() == stats, what  # no query inserts: not even one for a flow the index never saw
    check(tr, "untrimmed")
    tr = trim_both(hist, tr, 0, True, "fold")
    check(tr, "folded")
    tr = trim_both(hist, tr, 5, False, "drop")
    check(tr, "dropped")
    assert not hist.query(0, listed[:50], end_time=4)[1].any()
    hist.close()


# --- 8. through the engines, with retain ---
TS8 = [1_000, 2_000, 2_001, 5_000, 1 << 40, (1 << 40) + 1, 1 << 50, 1 << 60]
RESET_AFTER = (1, 4)


def window_cut(times, retain, drop):
    """`before` of the trim record_heavy makes once more than `retain` snapshots are held."""
    if drop:
        return times[-retain]
    return times[-(retain - 1)] if retain > 1 else times[-1] + 1


def run_engine(task, sketch, orc, insert, record_truth, types, K, retain, drop):
    from test_heavy_history_gpu import FIELDS_OF_K
    hist = task.keep_heavy_history(retain=retain, drop=drop, max_rows=64, max_flows=64)
    tr = HeavyTruth(FIELDS_OF_K[K])
    for i, t in enumerate(TS8):
        insert(i)
        task.record_heavy(t)
        record_truth(tr, t)
        if len(tr.times) > retain:
            tr = trimmed(tr, window_cut(tr.times, retain, drop), not drop)
        assert hist.times() == tr.times and len(hist.times()) <= retain
        for T in tr.probe_times():
            for type in types:
                want = [HeavyHitter(s, v) for s, v in tr.query(type, 1000, 0, T)]
                got = task.query_heavy_hitters(type, 1000, end_time=T)
                assert_same_list(got, want, f"interval {i} type {type} T {T}")
                top = got[:40]
                if top:  # the point query agrees with the list on the listed flows, by string and by bytes
                    assert task.query_heavy([h.Flow for h in top], type, end_time=T) == [h.Value for h in top]
                    assert task.query_heavy(tr.bytes[top[0].Flow], type, end_time=T) == top[0].Value
        if i in RESET_AFTER:
            sketch.reset()
            orc.reset()
    assert task.query_heavy(bytes(K), types[0]) == tr.latest(types[0]).get(tr.decode(bytes(K)))
    hist.close()
    sketch.close()


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("retain", [1, 2, 4])
@pytest.mark.parametrize("K", [4, 37])
def test_count_min_with_retain(gpu, oracle, K, retain, drop):
    from test_cm_gpu import make_pair
    from test_heavy_history_gpu import bare_task
    rng = np.random.default_rng(80 + K)
    cm, orc = make_pair(oracle, 64, 2, K, st=1, ct=1)
    flows = np.unique(rng.integers(0, 256, (400, K), dtype=np.uint8), axis=0)[:300]

    def insert(i):
        fl = flows[(i % 3) * 100:(i % 3) * 100 + 150]  # the lists move through the flows: some leave, some return
        keys = np.ascontiguousarray(fl[zipf_keys(rng, 2000, len(fl), 1)[2]])
        sizes = sizes_u32(rng, 2000)
        cm.insert_keys(keys, sizes)
        orc.insert_keys(keys, sizes)
    run_engine(bare_task(cm, K), cm, orc, insert, lambda tr, t: tr.record_cm(t, orc), (0, 1), K, retain, drop)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("retain", [1, 2, 4])
@pytest.mark.parametrize("K", [4, 37])
def test_superspread_with_retain(gpu, oracle, K, retain, drop):
    from test_heavy_history_gpu import bare_task
    from test_ss_gpu import make_pair
    rng = np.random.default_rng(90 + K)
    ss, orc = make_pair(oracle, 64, 2, 16, 5, K, 4, thr=1)
    flows = np.unique(rng.integers(0, 256, (400, K), dtype=np.uint8), axis=0)[:300]

    def insert(i):
        fl = flows[(i % 3) * 100:(i % 3) * 100 + 150]
        f = np.ascontiguousarray(fl[zipf_keys(rng, 2000, len(fl), 1)[2]])
        e = rng.integers(0, 256, (2000, 4), dtype=np.uint8)
        ss.insert_keys(f, e)
        orc.insert(f, e)
    run_engine(bare_task(ss, K), ss, orc, insert, lambda tr, t: tr.record_ss(t, orc), (2,), K, retain, drop)


# --- 9. a reader thread during retained records ---
@pytest.mark.parametrize("drop", [False, True])
def test_reader_thread_during_retained_records(gpu, oracle, drop):
    """Every answer the reader gets -- the top lists, and the point query of a fixed batch -- is the
    truth of some state the store passes through: after an append, or after the trim that follows."""
    from test_cm_gpu import make_pair
    from test_heavy_history_gpu import bare_task
    K, NI = 13, 10
    rng = np.random.default_rng(9)
    cm, orc = make_pair(oracle, 64, 2, K, st=1, ct=1)
    flows = np.unique(rng.integers(0, 256, (400, K), dtype=np.uint8), axis=0)[:300]
    batch = np.concatenate([flows[::3], flows[:20]])
    parts = []
    for i in range(NI):
        fl = flows[(i % 3) * 100:(i % 3) * 100 + 150]
        parts.append((np.ascontiguousarray(fl[zipf_keys(rng, 2000, len(fl), 1)[2]]), sizes_u32(rng, 2000)))

    def newest(tr):
        lat = tr.latest(0)
        want = [lat.get(bytes(f).hex()) for f in batch]
        return tr.query_bytes(0, 5), tr.query_bytes(1, 0), ([w is not None for w in want], [w or 0 for w in want])
    # the states, from the sequential oracle alone: empty, then per record the append and the trim after it
    tr = HeavyTruth(decode=bytes.hex)
    want = [newest(tr)]
    for i, (keys, sizes) in enumerate(parts):
        orc.insert_keys(keys, sizes)
        tr.record_cm(1000 + 10 * i, orc)
        want.append(newest(tr))
        if len(tr.times) > 2:
            tr = trimmed(tr, window_cut(tr.times, 2, drop), not drop)
            want.append(newest(tr))
        if i == 4:
            orc.reset()
    task = bare_task(cm, K)
    hist = task.keep_heavy_history(retain=2, drop=drop, max_rows=64, max_flows=64)
    stop, errors, seen = threading.Event(), [], set()

    def reader():
        try:
            while True:
                last = stop.is_set()  # one full round after the writer is done
                v, f = hist.query(0, batch)
                got = (entries(*hist.heavy_hitters(0, 0, 5)), entries(*hist.heavy_hitters(1)), (f.tolist(), v.tolist()))
                for part, g in enumerate(got):  # (three calls: a record may fall between them)
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
        for i, (keys, sizes) in enumerate(parts):
            cm.insert_keys(keys, sizes)
            task.record_heavy(1000 + 10 * i)
            assert len(hist.times()) <= 2
            if i == 4:
                cm.reset()
    finally:
        stop.set()
        th.join(timeout=60)
    assert not th.is_alive(), "the reader did not finish"
    assert not errors, errors
    assert len(want) - 1 in seen  # the last round saw the final state
    assert_log(hist, tr, (0, 1), "after the writer")
    hist.close()
    cm.close()
