"""Exact spread pair set on the GPU: export, delta export and union (gns_pairs_*).

The ground truth is test_spread_gpu's and shares no code with the engine:
np.unique over the rows flow bytes ‖ element bytes.  Exports are compared as sets
of row bytes, and no export may hold a row twice."""
import ctypes as ct
import functools

import numpy as np
import pytest

from helpers import assert_same_flows
from test_spread_gpu import growth_stream, keys4, new_exact, snap, truth_of

pytestmark = pytest.mark.gpu

TINY = dict(max_flows=64, max_pairs=256, batch_packets=5000)
SENTINEL = 0x5E5E5E5E5E5E5E5E


def pairs_of(fl, el) -> set:
    """The distinct rows flow ‖ elem, as bytes."""
    if len(fl) == 0:
        return set()
    rows = np.ascontiguousarray(np.concatenate([fl, el], axis=1))
    u = np.unique(rows.view(np.dtype((np.void, rows.shape[1]))).ravel())
    return set(u.tolist())


def rows_of(pairs: set, fb: int):
    """A pair set back as (flows, elems) arrays, in sorted order."""
    a = np.frombuffer(b"".join(sorted(pairs)), np.uint8).reshape(len(pairs), -1)
    return np.ascontiguousarray(a[:, :fb]), np.ascontiguousarray(a[:, fb:])


def exported(ex, since=0, device=False):
    """(set of row bytes, cursor, flows, elems) of one export; a row twice fails."""
    f, e, cur = ex.export_pairs(since=since, device=device)
    if device:
        assert f.is_cuda and e.is_cuda and f.device.index == ex.device
        f, e = f.cpu().numpy(), e.cpu().numpy()
    assert f.dtype == np.uint8 and e.dtype == np.uint8
    assert f.shape == (len(f), ex.flow_bytes) and e.shape == (len(f), ex.elem_bytes)
    rows = [bytes(r) for r in np.concatenate([f, e], axis=1)] if len(f) else []
    s = set(rows)
    assert len(s) == len(rows), "the export holds a row twice"
    return s, cur, f, e


def grouped(pairs: set, fb: int) -> dict:
    d = {}
    for r in pairs:
        d[r[:fb]] = d.get(r[:fb], 0) + 1
    return d


def check_export(ex, want: set):
    """Host and device exports are the wanted set, group to the snapshot, and count pairs_claimed."""
    host = exported(ex)[0]
    dev = exported(ex, device=True)[0]
    assert host == want and dev == want
    assert grouped(host, ex.flow_bytes) == snap(ex)
    assert len(host) == ex.dict_stats()["pairs_claimed"]


@functools.lru_cache(maxsize=None)
def stream():
    fl, el = growth_stream()
    fl.setflags(write=False)
    el.setflags(write=False)
    return fl, el


def arg_error(fn, *a, **kw):
    from go2netspectra_amd import GnsError, _lib
    with pytest.raises(GnsError) as e:
        fn(*a, **kw)
    assert e.value.code == _lib.GNS_E_ARG
    return str(e.value)


# --- 1 ---------------------------------------------------------------------
def test_degenerate(gpu):
    from go2netspectra_amd import _lib
    ex = new_exact()
    L, h = ex._L, ex._h
    n, cur = ct.c_uint64(0), ct.c_uint64(SENTINEL)
    assert L.gns_pairs_export(h, 0, None, None, ct.byref(n), ct.byref(cur), _lib.MEM_HOST) == 0
    assert n.value == 0 and cur.value != SENTINEL
    f, e = np.full((4, 16), 0xAB, np.uint8), np.full((4, 16), 0xAB, np.uint8)
    n = ct.c_uint64(4)
    assert L.gns_pairs_export(h, 0, f.ctypes.data, e.ctypes.data, ct.byref(n), ct.byref(cur), _lib.MEM_HOST) == 0
    assert n.value == 0 and (f == 0xAB).all() and (e == 0xAB).all()
    s0, c0, _, _ = exported(ex)
    assert s0 == set() and exported(ex, since=c0)[0] == set() and exported(ex, device=True)[0] == set()
    a, b = keys4([7]), keys4([9])
    ex.insert_keys(a, b)
    one = {bytes(a[0]) + bytes(b[0])}
    check_export(ex, one)
    assert exported(ex, since=c0)[0] == one  # the empty handle's cursor is usable
    ex.reset()
    ex.insert_keys(np.repeat(a, 4096, axis=0), np.repeat(b, 4096, axis=0))
    check_export(ex, one)


# --- 2 ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 300])
def test_compaction_at_wave_and_workgroup_edges(gpu, n):
    rng = np.random.default_rng(n)
    fl, el = keys4(np.arange(n) % 7), keys4(1000 + np.arange(n))
    idx = rng.permutation(np.repeat(np.arange(n), 2))  # every pair twice: 2n rows in one batch
    ex = new_exact(max_flows=64, max_pairs=256)
    assert ex.dict_stats()["pair_slots"] == 512
    ex.insert_keys(fl[idx], el[idx])
    assert (ex.dict_stats()["pair_growths"] >= 1) == (n >= 255)
    want = pairs_of(fl, el)
    assert len(want) == n
    check_export(ex, want)


# --- 3 ---------------------------------------------------------------------
@pytest.mark.parametrize("fb,eb", [(16, 16), (37, 37), (5, 6), (2, 1), (37, 1)])
def test_key_shapes(gpu, fb, eb):
    """Both record widths (pair keys up to 32 bytes, and wider), word and byte row writers,
    and a flow / element split inside a word."""
    from go2netspectra_amd import ExactSpread
    rng = np.random.default_rng(100 * fb + eb)
    n = 20_000
    flows = rng.integers(0, 256, (50, fb), dtype=np.uint8)
    elems = rng.integers(0, 256, (3000, eb), dtype=np.uint8)
    elems[:, : eb - 1] = elems[0, : eb - 1]  # elements that differ in their last byte only
    fl = np.ascontiguousarray(flows[rng.integers(0, 50, n)])
    el = np.ascontiguousarray(elems[rng.integers(0, 3000, n)])
    want = pairs_of(fl, el)
    assert 1000 < len(want) < n
    ex = ExactSpread(None, None, flow_bytes=fb, elem_bytes=eb, max_flows=8, max_pairs=64, batch_packets=3000)
    ex.insert_keys(fl, el)
    assert ex.dict_stats()["pair_growths"] >= 2
    assert_same_flows(snap(ex), truth_of(fl, el))
    check_export(ex, want)


# --- 4 ---------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_capacity(gpu, device):
    import torch
    from go2netspectra_amd import _lib
    fl, el = keys4(np.arange(1000) % 13), keys4(5000 + np.arange(1000))
    ex = new_exact(max_pairs=4096)
    ex.insert_keys(fl, el)
    f, e = np.full((40, 16), 0xAB, np.uint8), np.full((40, 16), 0xAB, np.uint8)
    where = _lib.MEM_HOST
    fp, ep = f.ctypes.data, e.ctypes.data
    if device:
        tf, te = torch.from_numpy(f).to("cuda:0"), torch.from_numpy(e).to("cuda:0")
        torch.cuda.synchronize()
        fp, ep, where = tf.data_ptr(), te.data_ptr(), _lib.MEM_DEVICE
    n, cur = ct.c_uint64(10), ct.c_uint64(SENTINEL)
    assert ex._L.gns_pairs_export(ex._h, 0, fp, ep, ct.byref(n), ct.byref(cur), where) == 0
    if device:
        f, e = tf.cpu().numpy(), te.cpu().numpy()
    assert n.value == 1000
    assert (f[10:] == 0xAB).all() and (e[10:] == 0xAB).all()
    assert cur.value == SENTINEL  # an export that did not fit gives no cursor
    assert len(exported(ex, device=device)[0]) == 1000


# --- 5 ---------------------------------------------------------------------
def test_delta(gpu):
    fl, el = stream()
    cutA, cutM = 700, 150_000
    ex = new_exact(**TINY)
    for lo, hi in ((0, 60), (60, cutA)):  # small calls: both tables are still small at the first cursor
        ex.insert_keys(fl[lo:hi], el[lo:hi])
    sA, cA, _, _ = exported(ex)
    pA = pairs_of(fl[:cutA], el[:cutA])
    assert sA == pA
    dsA = ex.dict_stats()
    ex.insert_keys(fl[cutA:cutM], el[cutA:cutM])
    sM, cM, _, _ = exported(ex, since=cA)
    pM = pairs_of(fl[:cutM], el[:cutM])
    assert sM == pM - pA
    ex.insert_keys(fl[cutM:], el[cutM:])
    dsB = ex.dict_stats()
    assert dsB["flow_growths"] > dsA["flow_growths"] and dsB["pair_growths"] > dsA["pair_growths"], (dsA, dsB)
    pall = pairs_of(fl, el)
    # B repeats many of A's pairs (the same Zipf flows): the delta is neither empty nor all of B's pairs
    for cut, p0, c in ((cutA, pA, cA), (cutM, pM, cM)):
        true = pall - p0
        assert 0 < len(true) < len(pairs_of(fl[cut:], el[cut:]))
        got, cB, _, _ = exported(ex, since=c)
        assert got == true
        assert exported(ex, since=c, device=True)[0] == true
    assert exported(ex, since=cB)[0] == set()
    check_export(ex, pall)


# --- 6 ---------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_merge_from_rows(gpu, device):
    import torch
    fl, el = stream()
    h = len(fl) // 2
    pA, pB = pairs_of(fl[:h], el[:h]), pairs_of(fl[h:], el[h:])
    ex = new_exact(**TINY)
    ex.insert_keys(fl[:h], el[:h])
    bf, be = rows_of(pB, 16)
    idx = np.random.default_rng(3).permutation(np.repeat(np.arange(len(bf)), 3))  # every row three times
    bf, be = np.ascontiguousarray(bf[idx]), np.ascontiguousarray(be[idx])
    c0, d0 = ex.counters(), ex.dict_stats()
    if device:
        ex.merge_pairs(torch.from_numpy(bf).to("cuda:0"), torch.from_numpy(be).to("cuda:0"))
    else:
        ex.merge_pairs(bf, be)
    assert_same_flows(snap(ex), truth_of(fl, el))
    c1, d1 = ex.counters(), ex.dict_stats()
    for k in ("inserted", "dropped", "unsupported", "records", "batches"):
        assert c1[k] == c0[k], k
    assert c1["new_pairs"] - c0["new_pairs"] == len(pB - pA) > 0
    assert c1["flows"] == len(truth_of(fl, el))
    assert d1["pair_growths"] > d0["pair_growths"]  # the table grew under the merge
    check_export(ex, pA | pB)


def test_merge_hot_flow_and_shared_element(gpu):
    """test_contention_both_ways' stream as a merge: one flow with 100 000 new elements (one
    hot counter), 100 000 flows that share one element, into tables that start tiny."""
    rng = np.random.default_rng(6)
    n = 100_000
    fl = np.concatenate([keys4(np.arange(n)), np.repeat(keys4([6_000_000]), n, axis=0)])
    el = np.concatenate([np.repeat(keys4([5_000_000]), n, axis=0), keys4(1_000_000 + np.arange(n))])
    perm = rng.permutation(len(fl))
    fl, el = fl[perm], el[perm]
    ex = new_exact(max_flows=64, max_pairs=256, batch_packets=50_000)
    ex.insert_keys(fl[:1000], el[:1000])
    ex.merge_pairs(fl, el)
    want = truth_of(fl, el)
    assert want[bytes(keys4([6_000_000])[0])] == n and len(want) == n + 1
    assert_same_flows(snap(ex), want)
    c = ex.counters()
    assert c["inserted"] == 1000 and c["new_pairs"] == 2 * n and c["batches"] == 1


# --- 7 ---------------------------------------------------------------------
def test_merge_from_handle(gpu):
    from go2netspectra_amd import ExactSpread
    fl, el = stream()
    half = np.random.default_rng(12).random(len(fl)) < 0.5  # split by packet, not by flow
    dst, src, whole = new_exact(**TINY), new_exact(**TINY), new_exact(**TINY)
    dst.insert_keys(fl[half], el[half])
    src.insert_keys(fl[~half], el[~half])
    whole.insert_keys(fl, el)
    src_before = snap(src)
    c1 = dst.merge_from(src)
    want = truth_of(fl, el)
    assert_same_flows(snap(dst), want)
    assert snap(dst) == snap(whole)
    for a, b in zip(dst.heavy_hitters_arrays(100), whole.heavy_hitters_arrays(100)):
        assert len(a) > 10 and np.array_equal(a, b)
    assert snap(src) == src_before
    assert src.counters()["new_pairs"] == len(pairs_of(fl[~half], el[~half]))
    # the delta only: more traffic into src, of which some repeats what both handles hold
    xf = np.concatenate([keys4(np.arange(5000) % 40), fl[:5000]])
    xe = np.concatenate([keys4(9_000_000 + np.arange(5000)), el[:5000]])
    src.insert_keys(xf, xe)
    before = dst.counters()["new_pairs"]
    c2 = dst.merge_from(src, since=c1)
    assert c2 != c1
    assert dst.counters()["new_pairs"] - before == 5000
    allf, alle = np.concatenate([fl, xf]), np.concatenate([el, xe])
    assert_same_flows(snap(dst), truth_of(allf, alle))
    check_export(dst, pairs_of(allf, alle))
    assert dst.merge_from(src, since=c2) == c2 and dst.counters()["new_pairs"] - before == 5000
    # refused before any device work, dst untouched
    got = snap(dst)
    stats = dst.counters()
    assert "same handle" in arg_error(dst.merge_from, dst)
    wide = ExactSpread(None, None, flow_bytes=37, elem_bytes=37, max_flows=8, max_pairs=64)
    arg_error(wide.merge_from, dst)
    arg_error(dst.merge_from, wide)
    assert snap(wide) == {} and snap(dst) == got and dst.counters() == stats


def test_tables_of_several_pieces(gpu):
    """A source table of 2^22 slots is walked in four staged pieces: the host export copies
    each out, merge_from gathers them behind one another before it merges."""
    fl, el = stream()
    src = new_exact(max_flows=4096, max_pairs=1 << 21, batch_packets=100_000)
    assert src.dict_stats()["pair_slots"] == 1 << 22
    src.insert_keys(fl, el)
    want = pairs_of(fl, el)
    check_export(src, want)
    h = 120_000
    _, cur, _, _ = exported(src)
    dst = new_exact(**TINY)
    dst.insert_keys(fl[:h], el[:h])
    before = dst.counters()["new_pairs"]
    dst.merge_from(src)
    assert dst.counters()["new_pairs"] - before == len(want - pairs_of(fl[:h], el[:h]))
    assert snap(dst) == snap(src)
    check_export(dst, want)
    assert src.dict_stats()["pair_growths"] == 0 and exported(src, since=cur)[0] == set()


# --- 8 ---------------------------------------------------------------------
def test_chained_deltas(gpu):
    fl, el = stream()
    src, coll = new_exact(**TINY), new_exact(**TINY)
    last, seen = 0, set()
    for part in np.array_split(np.arange(len(fl)), 3):
        src.insert_keys(fl[part], el[part])
        new = pairs_of(fl[part], el[part]) - seen
        seen |= new
        assert 0 < len(new)
        # what this delta moves, alone in an empty handle: the new pairs and no others
        probe = new_exact(**TINY)
        probe.merge_from(src, since=last)
        assert probe.dict_stats()["pairs_claimed"] == len(new)
        probe.close()
        before = coll.counters()["new_pairs"]
        last = coll.merge_from(src, since=last)
        assert coll.counters()["new_pairs"] - before == len(new)
    # a collector of the collector sees the merged pairs: they are stamped at the merge
    down = new_exact(**TINY)
    down.merge_from(coll)
    want = truth_of(fl, el)
    assert snap(src) == snap(coll) == snap(down)
    assert_same_flows(snap(coll), want)
    check_export(coll, seen)


# --- 9 ---------------------------------------------------------------------
def test_reset_and_cursors(gpu):
    fl, el = stream()
    fl, el = fl[:40_000], el[:40_000]
    ex, other = new_exact(**TINY), new_exact(**TINY)
    ex.insert_keys(fl, el)
    _, c, _, _ = exported(ex)
    assert "full export" in arg_error(ex.export_pairs, since=c + 7)  # a point the handle has not reached
    assert exported(ex, since=c)[0] == set()
    ex.reset()
    assert "full export" in arg_error(ex.export_pairs, since=c)
    arg_error(other.merge_from, ex, since=c)
    assert snap(other) == {}
    assert exported(ex)[0] == set()
    ex.insert_keys(fl[:20_000], el[:20_000])
    check_export(ex, pairs_of(fl[:20_000], el[:20_000]))
    _, c2, _, _ = exported(ex)
    ex.insert_keys(fl[20_000:], el[20_000:])
    assert exported(ex, since=c2)[0] == pairs_of(fl, el) - pairs_of(fl[:20_000], el[:20_000])


# --- 10 --------------------------------------------------------------------
def test_epoch_wrap(gpu, monkeypatch):
    """The 32-bit launch counter wraps inside the stream: the tags are rewritten, a new
    cursor generation begins, and nothing is lost, counted twice or run twice."""
    fl, el = stream()
    monkeypatch.setenv("GNS_EXS_TEST_EPOCH", str(2**32 - 40))  # a batch is two launches or more
    ex = new_exact(**TINY)
    monkeypatch.delenv("GNS_EXS_TEST_EPOCH")
    a, b = 10_000, 250_000
    ex.insert_keys(fl[:a], el[:a])
    _, c_pre, _, _ = exported(ex)
    assert exported(ex, since=c_pre)[0] == set()
    ex.insert_keys(fl[a:b], el[a:b])  # 48 batches: the wrap is in here
    assert_same_flows(snap(ex), truth_of(fl[:b], el[:b]))
    assert "full export" in arg_error(ex.export_pairs, since=c_pre)
    s_post, c_post, _, _ = exported(ex)
    assert s_post == pairs_of(fl[:b], el[:b])
    ex.insert_keys(fl[b:], el[b:])
    delta = pairs_of(fl, el) - s_post
    assert 0 < len(delta) < len(pairs_of(fl[b:], el[b:]))
    assert exported(ex, since=c_post)[0] == delta
    assert_same_flows(snap(ex), truth_of(fl, el))
    check_export(ex, pairs_of(fl, el))
    c = ex.counters()
    assert c["batches"] == len(fl) // 5000 and c["inserted"] == len(fl)
    assert c["new_pairs"] == len(pairs_of(fl, el))
    plain = new_exact(**TINY)  # without the hook no cursor of this stream is refused
    plain.insert_keys(fl[:a], el[:a])
    _, c0, _, _ = exported(plain)
    plain.insert_keys(fl[a:b], el[a:b])
    assert exported(plain, since=c0)[0] == s_post - pairs_of(fl[:a], el[:a])


# --- 11 --------------------------------------------------------------------
def test_checkpoint(gpu, tmp_path):
    from go2netspectra_amd import ExactSpread
    fl, el = stream()
    h = 100_000
    kw = dict(max_flows=4096, max_pairs=1 << 16)
    ex = ExactSpread(["SrcIP"], ["DstIP"], **kw)
    ex.insert_keys(fl[:h], el[:h])
    path = tmp_path / "spread.npz"
    ex.save(path)
    back = ExactSpread(["SrcIP"], ["DstIP"], **kw)
    back.insert_keys(fl[-50:], el[-50:])  # restore replaces what the handle held
    back.restore(path)
    assert snap(back) == snap(ex)
    assert_same_flows(snap(back), truth_of(fl[:h], el[:h]))
    for e in (ex, back):
        e.insert_keys(fl[h:], el[h:])
    assert snap(back) == snap(ex)
    assert_same_flows(snap(back), truth_of(fl, el))
    other = ExactSpread(["SrcIP"], ["SrcIP"], **kw)
    with pytest.raises(ValueError, match="'elem_fields'"):
        other.restore(path)
    assert snap(other) == {}
