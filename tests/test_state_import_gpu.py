"""The write side of the state interface on the GPU: gns_cm_import_state,
gns_ss_import_state, gns_ex_merge and the Python layer above them
(checkpoint files, Manager.checkpoint / restore, dist.load_global).  Every
comparison is bit-exact: an imported handle exports the bytes it was given,
answers as the exporting handle did, and continues as the sequential oracle
does from that state."""

import numpy as np
import pytest

from helpers import (assert_same_flows, assert_same_list, frames_from_tuples, pcapgen_records, random_tuples,
                     sizes_u32, zipf_index, zipf_keys)

pytestmark = pytest.mark.gpu

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
CM_NAMES = ("C", "S", "FPc", "FPs")
SS_NAMES = ("values", "keys", "regs", "pbits")
HLL_MASTER, RNG_SEED = 0x0123456789ABCDEF, 0x0DDBA11CAFEF00D5


def assert_same_arrays(names, got, want, what=""):
    for name, a, b in zip(names, got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)  # bit patterns
        if a.shape != b.shape or not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0] if a.ndim == 1 else np.nonzero((a != b).any(axis=1))[0]
            raise AssertionError(f"{what}{name} differs in {len(bad)} cells, first {bad[:5]}: "
                                 f"got={a[bad[:3]]} want={b[bad[:3]]}")


def cm_seeds(d, seed=1):
    return np.random.default_rng(seed).integers(0, 2**32, d, dtype=np.uint64).astype(np.uint32)


def cm_new(w, d, K, st=1000, ct=10, **kw):
    from go2netspectra_amd import CountMin
    return CountMin(w, d, st, ct, key_bytes=K, seeds=cm_seeds(d), **kw)


def cm_lists(cm):
    hh = cm.heavy_hitters()
    return [(h.Flow, h.Count) for h in hh.Count], [(h.Flow, h.Size) for h in hh.Size]


def cm_counters3(cm):
    c = cm.counters()
    return [c["inserted"], c["dropped"], c["unsupported"]]


def distinct_fingerprints(Fc, Fs):
    fp = np.concatenate([Fc, Fs])
    fp = fp[fp.any(axis=1)]
    return len(np.unique(fp, axis=0))


# ---------------------------------------------------------------------------
# Count-Min
# ---------------------------------------------------------------------------
CM_GEOMETRIES = [(1, 1, 4), (1, 4, 16), (16, 2, 8), (1000, 3, 13), (4096, 4, 37), (4096, 8, 37), (65536, 4, 16)]
_cm_exports = {}


def cm_exported(w, d, K):
    """(exporting handle, its export, the flows of its stream), made once per geometry."""
    key = (w, d, K)
    if key not in _cm_exports:
        rng = np.random.default_rng(w * 7 + d * 3 + K)
        x = cm_new(w, d, K)
        keys, flows, _ = zipf_keys(rng, 60_000, 5000, K)
        x.insert_keys(keys, sizes_u32(rng, 60_000, big_frac=0.01))
        x.flush()
        _cm_exports[key] = (x, x.export_state(), flows, rng.integers(0, 256, (100, K), dtype=np.uint8))
    return _cm_exports[key]


def check_imported(y, x, state, flows, absent):
    assert_same_arrays(CM_NAMES, y.export_state(), state)
    q = np.concatenate([flows, absent])
    assert np.array_equal(y.query_many(q), x.query_many(q))
    for got, want, what in zip(cm_lists(y), cm_lists(x), ("count list", "size list")):
        assert_same_list(got, want, what)
    nd = distinct_fingerprints(state[2], state[3])
    claimed = y.dict_stats()["claimed"]
    assert nd <= claimed <= nd + 1, (nd, claimed)  # + 1: the all-zero key, if a cell holds it


@pytest.mark.parametrize("w,d,K", CM_GEOMETRIES)
def test_cm_round_trip(gpu, w, d, K):
    x, state, flows, absent = cm_exported(w, d, K)
    y = cm_new(w, d, K)
    y.import_state(*state, counters=cm_counters3(x))
    check_imported(y, x, state, flows, absent)
    assert cm_counters3(y) == cm_counters3(x)
    assert y.counters()["dict_full"] == 0
    y.close()


@pytest.mark.parametrize("kind", ["keys", "headers"])
def test_cm_continuation_equals_the_oracle(gpu, oracle, kind):
    """import(export of X after A), then B == the oracle over A+B == X after B; B spans three
    device batches."""
    from go2netspectra_amd import CountMin
    rng = np.random.default_rng(31)
    w, d, n, cut = 4096, 4, 63_457, 23_457  # B = 40_000 packets = 16384 + 16384 + 7232
    seeds = cm_seeds(d)
    if kind == "keys":
        K = 16
        keys, _, _ = zipf_keys(rng, n, 5000, K)
        sizes = sizes_u32(rng, n, big_frac=0.01)
        mk = lambda: CountMin(w, d, 1000, 10, key_bytes=K, seeds=seeds, batch_packets=16384)
        put = lambda cm, lo, hi: cm.insert_keys(keys[lo:hi], sizes[lo:hi])
        orc = oracle.CountMin(w, d, 1000, 10, K, seeds)
        orc.insert_keys(keys, sizes)
    else:
        t = random_tuples(rng, n, 5000, v6_frac=0.2)
        hdr = frames_from_tuples(t, rng, vlan_frac=0.2)
        hdr[rng.random(n) < 0.02, 12:14] = [0x08, 0x06]  # ARP: dropped
        mk = lambda: CountMin(w, d, 1000, 10, flow_fields=FIVE, seeds=seeds, batch_packets=16384)
        put = lambda cm, lo, hi: cm.insert_headers(hdr[lo:hi], t["length"][lo:hi])
        orc = oracle.CountMin(w, d, 1000, 10, 37, seeds)
        orc.insert_hdr64(hdr, t["length"], FIVE)
    x, y = mk(), mk()
    put(x, 0, cut)
    x.flush()
    y.import_state(*x.export_state(), counters=cm_counters3(x))
    put(x, cut, n)
    put(y, cut, n)
    x.flush()
    y.flush()
    assert_same_arrays(CM_NAMES, y.export_state(), orc.export(), "oracle ")
    assert_same_arrays(CM_NAMES, y.export_state(), x.export_state(), "uninterrupted ")
    assert cm_counters3(y) == cm_counters3(x)
    assert_same_list(cm_lists(y)[0], orc.heavy("count"))
    assert_same_list(cm_lists(y)[1], orc.heavy("size"))


def test_cm_import_over_a_used_handle_with_a_view(gpu):
    from go2netspectra_amd import GnsError
    w, d, K = 4096, 4, 37
    x, state, flows, absent = cm_exported(w, d, K)
    rng = np.random.default_rng(5)
    y = cm_new(w, d, K)
    other, _, _ = zipf_keys(rng, 50_000, 8000, K)
    y.insert_keys(other, sizes_u32(rng, 50_000))
    view = y.view()
    view.refresh()
    assert view.query_many(other[:10]).any()
    y.import_state(*state)
    check_imported(y, x, state, flows, absent)
    with pytest.raises(GnsError) as e:
        view.query_many(flows[:10])  # taken before the import: stale, as after a reset
    assert e.value.code == -1
    with pytest.raises(GnsError):
        view.heavy_hitters()
    view.refresh()
    q = np.concatenate([flows, absent])
    assert np.array_equal(view.query_many(q), x.query_many(q))
    hh = view.heavy_hitters()
    assert_same_list([(h.Flow, h.Count) for h in hh.Count], cm_lists(x)[0])
    assert_same_list([(h.Flow, h.Size) for h in hh.Size], cm_lists(x)[1])
    view.close()
    y.close()


def test_cm_import_grows_a_tiny_dictionary(gpu):
    from go2netspectra_amd import CountMin
    rng = np.random.default_rng(41)
    w, d = 65536, 4
    seeds = cm_seeds(d)
    hdr, wl = pcapgen_records(rng, 50_000)
    x = CountMin(w, d, 1000, 10, flow_fields=FIVE, seeds=seeds)
    x.insert_headers(hdr, wl)
    x.flush()
    state = x.export_state()
    y = CountMin(w, d, 1000, 10, flow_fields=FIVE, seeds=seeds, max_flows=64)
    y.import_state(*state)
    assert_same_arrays(CM_NAMES, y.export_state(), state)
    ds = y.dict_stats()
    assert ds["growths"] > 0 and ds["slots"] > 128, ds
    nd = distinct_fingerprints(state[2], state[3])
    assert nd <= ds["claimed"] <= nd + 1, (nd, ds)
    assert y.counters()["dict_full"] == 0
    y.insert_headers(hdr[:20_000], wl[:20_000])  # and it keeps counting
    x.insert_headers(hdr[:20_000], wl[:20_000])
    x.flush()
    y.flush()
    assert_same_arrays(CM_NAMES, y.export_state(), x.export_state())


def test_cm_hand_made_state_against_pyref(gpu):
    """A start state nobody has to earn by ingest: C == 0 under a live FPc, S == 0 under a live
    FPs, the all-zero key, a size counter about to wrap and a full count counter; then 3K
    packets, against the pure-Python restatement started from the same arrays."""
    from oracle import pyref
    w, d, K = 16, 2, 16
    rng = np.random.default_rng(8)
    seeds = [int(s) for s in cm_seeds(d)]
    flows = [bytes(K)] + [bytes(f) for f in rng.integers(0, 256, (39, K), dtype=np.uint8)]
    cell = lambda key, row: row * w + pyref.mm3(key, seeds[row]) % w
    # four more keys (rows 0, 0, 1, 1) whose cells are distinct from each other and the zero key's
    zero = flows[0]
    picks, used = [], {cell(zero, 0)}
    for f in flows[1:]:
        row = (0, 0, 1, 1)[len(picks)]
        if cell(f, row) not in used:
            used.add(cell(f, row))
            picks.append(f)
            if len(picks) == 4:
                break
    k0, k1, k2, k3 = picks
    ref = pyref.CountMinSeq(w, d, 1000, 10, K, seeds)

    def put(c, C=None, Fc=None, S=None, Fs=None):
        if C is not None:
            ref.C[c], ref.Fc[c] = C, Fc
        if S is not None:
            ref.S[c], ref.Fs[c] = S, Fs

    put(cell(k0, 0), C=0, Fc=k0, S=7, Fs=k0)                 # C == 0 under a live FPc
    put(cell(k1, 0), C=3, Fc=k1, S=0, Fs=k1)                 # S == 0 under a live FPs
    put(cell(zero, 0), C=5, Fc=zero)                         # the all-zero key owns a count cell
    put(cell(k2, 1), C=2, Fc=k2, S=2**32 - 100, Fs=k2)       # S wraps when the stream feeds k2
    put(cell(k3, 1), C=2**32 - 1, Fc=k3, S=10, Fs=k3)        # C wraps
    to_np = lambda fp: np.frombuffer(b"".join(fp), np.uint8).reshape(d * w, K)
    start = (np.array(ref.C, np.uint32), np.array(ref.S, np.uint32), to_np(ref.Fc), to_np(ref.Fs))
    cm = cm_new(w, d, K)
    cm.import_state(*start)
    assert_same_arrays(CM_NAMES, cm.export_state(), start, "start ")
    idx = np.concatenate([np.arange(40), zipf_index(rng, 2960, 40)])  # every flow at least once
    rng.shuffle(idx)
    sizes = sizes_u32(rng, 3000)
    keys = np.frombuffer(b"".join(flows[i] for i in idx), np.uint8).reshape(3000, K)
    cm.insert_keys(keys, sizes)
    cm.flush()
    for i, s in zip(idx, sizes):
        ref.insert(flows[i], int(s))
    want = (np.array(ref.C, np.uint32), np.array(ref.S, np.uint32), to_np(ref.Fc), to_np(ref.Fs))
    assert_same_arrays(CM_NAMES, cm.export_state(), want)
    q = cm.query_many(keys[:200])
    assert np.array_equal(q, np.array([ref.query(bytes(k)) for k in keys[:200]], np.uint64))


def test_cm_null_pointer_leaves_the_handle_untouched(gpu):
    from go2netspectra_amd import _lib
    x, state, flows, absent = cm_exported(16, 2, 8)
    C, S, Fc, Fs = [np.ascontiguousarray(a) for a in state]
    ptrs = [C.ctypes.data, S.ctypes.data, Fc.ctypes.data, Fs.ctypes.data]
    for i in range(4):
        args = list(ptrs)
        args[i] = None
        assert x._L.gns_cm_import_state(x._h, *args, None) == _lib.GNS_E_ARG
    assert_same_arrays(CM_NAMES, x.export_state(), state)
    with pytest.raises(ValueError):
        x.import_state(C[:-1], S, Fc, Fs)


# ---------------------------------------------------------------------------
# SuperSpread
# ---------------------------------------------------------------------------
def ss_new(w, d, m, size, Kf=None, Ke=None, thr=20, **kw):
    from go2netspectra_amd import SuperSpread
    seeds = cm_seeds(d, 2)
    return SuperSpread(w, d, thr, m, size, 0.5, 1.08, flow_bytes=Kf, elem_bytes=Ke, seeds=seeds,
                       hll_master=HLL_MASTER, rng_seed=RNG_SEED, **kw)


def ss_counters3(ss):
    c = ss.counters()
    return [c["inserted"], c["dropped"], c["unsupported"]]


@pytest.mark.parametrize("w,d,m,size", [(1, 1, 1, 3), (16, 2, 32, 5), (1000, 3, 128, 5), (4096, 2, 128, 8)])
def test_ss_round_trip(gpu, w, d, m, size):
    rng = np.random.default_rng(w + m)
    Kf, Ke, n = 13, 7, 60_000
    flows = rng.integers(0, 256, (3000, Kf), dtype=np.uint8)
    fl = np.ascontiguousarray(flows[zipf_index(rng, n, 3000)])
    el = rng.integers(0, 256, (n // 4, Ke), dtype=np.uint8)[rng.integers(0, n // 4, n)]
    x = ss_new(w, d, m, size, Kf, Ke)
    x.insert_keys(fl, el)
    x.flush()
    state = x.export_state()
    y = ss_new(w, d, m, size, Kf, Ke)
    y.import_state(*state, x.counters()["records"], counters=ss_counters3(x))
    assert_same_arrays(SS_NAMES, y.export_state(), state)
    assert np.array_equal(y.query_many(flows), x.query_many(flows))
    assert_same_list([(h.Flow, h.Count) for h in y.heavy_hitters().Count],
                     [(h.Flow, h.Count) for h in x.heavy_hitters().Count])
    cy, cx = y.counters(), x.counters()
    assert ss_counters3(y) == ss_counters3(x) and cy["records"] == cx["records"]
    nd = distinct_fingerprints(state[1], state[1][:0])
    assert nd <= y.dict_stats()["claimed"] <= nd + 1
    # the same stream again: both draw the same uniforms from the restored position
    x.insert_keys(fl[:20_000], el[:20_000])
    y.insert_keys(fl[:20_000], el[:20_000])
    x.flush()
    y.flush()
    assert_same_arrays(SS_NAMES, y.export_state(), x.export_state())


def test_ss_continuation_through_headers(gpu, oracle):
    """A holds non-IP records, so the generator's position differs from the packets inserted."""
    from go2netspectra_amd import SuperSpread
    rng = np.random.default_rng(12)
    w, d, m, size, n, cut = 1024, 2, 64, 5, 50_000, 21_003
    seeds = cm_seeds(d, 2)
    t = random_tuples(rng, n, 3000, v6_frac=0.2)
    hdr = frames_from_tuples(t, rng, vlan_frac=0.2)
    hdr[rng.random(n) < 0.05, 12:14] = [0x08, 0x06]  # ARP: dropped, yet it advances the generator
    mk = lambda: SuperSpread(w, d, 20, m, size, 0.5, 1.08, flow_fields=["SrcIP"], elem_fields=["DstIP"], seeds=seeds,
                             hll_master=HLL_MASTER, rng_seed=RNG_SEED, batch_packets=16384)
    x, y = mk(), mk()
    x.insert_headers(hdr[:cut], t["length"][:cut])
    x.flush()
    c = x.counters()
    assert c["records"] == cut and c["inserted"] < cut
    y.import_state(*x.export_state(), c["records"], counters=ss_counters3(x))
    y.insert_headers(hdr[cut:], t["length"][cut:])
    y.flush()
    orc = oracle.SuperSpread(w, d, 20, m, size, 0.5, 1.08, 16, 16, seeds, HLL_MASTER, RNG_SEED)
    orc.insert_hdr64(hdr, t["length"], ["SrcIP"], ["DstIP"])
    assert_same_arrays(SS_NAMES, y.export_state(), orc.export(), "oracle ")
    assert y.counters()["records"] == n


def test_ss_register_out_of_range(gpu):
    from go2netspectra_amd import GnsError
    rng = np.random.default_rng(3)
    w, d, m, size = 64, 2, 32, 5
    y = ss_new(w, d, m, size, 8, 8)
    fl = rng.integers(0, 256, (5000, 8), dtype=np.uint8)
    y.insert_keys(fl, fl[::-1].copy())
    y.flush()
    before, rec = y.export_state(), y.counters()["records"]
    v, k, r, p = [a.copy() for a in before]
    r[w * d - 1, m - 1] = 2**size
    with pytest.raises(GnsError) as e:
        y.import_state(v, k, r, p, 0)
    assert e.value.code == -1
    assert_same_arrays(SS_NAMES, y.export_state(), before)
    assert y.counters()["records"] == rec
    r[w * d - 1, m - 1] = 2**size - 1  # the largest legal register
    y.import_state(v, k, r, p, 7)
    assert y.export_state()[2][w * d - 1, m - 1] == 2**size - 1 and y.counters()["records"] == 7


# ---------------------------------------------------------------------------
# Exact
# ---------------------------------------------------------------------------
def gpu_flows(task):
    return {f.Key: (f.StartTime, f.EndTime, f.PacketCount, f.ByteCount) for f in task.flows()}


def ex_stream(rng, n, nflows):
    t = random_tuples(rng, n, nflows, v6_frac=0.3, s=1.05)
    ipver = np.where(t["v6"], 6, 4).astype(np.uint8)
    ts = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)  # not monotonic: order is stream order
    return t, ipver, ts


def ex_put(task, orc, s, lo, hi):
    from go2netspectra_amd import PacketBatch
    t, ipver, ts = s
    a = [t[k][lo:hi] for k in ("src16", "dst16", "sport", "dport", "proto", "length")]
    if task is not None:
        task.process_packets(PacketBatch(*a, ipver[lo:hi], ts[lo:hi]))
        task.flush()
    if orc is not None:
        orc.insert_tuples(*a[:5], ipver[lo:hi], a[5], ts[lo:hi])


@pytest.mark.parametrize("fields", [FIVE, ["SrcIP"]])
def test_ex_restore_then_continue(gpu, oracle, fields):
    from go2netspectra_amd import ExactTask
    rng = np.random.default_rng(len(fields))
    s = ex_stream(rng, 50_000, 6000)
    x, y, orc = ExactTask("x", fields), ExactTask("y", fields), oracle.Exact(fields)
    ex_put(x, orc, s, 0, 30_000)
    snap = x.agg.snapshot_arrays()
    before = y.agg.counters()
    y.agg.merge(*snap)
    assert_same_flows(gpu_flows(y), gpu_flows(x), "restored")
    assert_same_flows(gpu_flows(y), orc.export(), "restored vs oracle")
    after = y.agg.counters()
    assert after["flows"] == len(snap[3]) and {k: v for k, v in after.items() if k != "flows"} == \
        {k: v for k, v in before.items() if k != "flows"}
    ex_put(y, orc, s, 30_000, 50_000)
    assert_same_flows(gpu_flows(y), orc.export(), "continued")


def test_ex_overlapping_shards_unite(gpu, oracle):
    """X(A) merged with the snapshot of Y(B) == the oracle over A then B: a flow in both keeps
    A's start and takes B's end."""
    from go2netspectra_amd import ExactTask
    rng = np.random.default_rng(9)
    s = ex_stream(rng, 40_000, 4000)
    x, y, orc = ExactTask("x", FIVE), ExactTask("y", FIVE), oracle.Exact(FIVE)
    ex_put(x, orc, s, 0, 20_000)
    ex_put(y, orc, s, 20_000, 40_000)
    fx, fy = gpu_flows(x), gpu_flows(y)
    x.agg.merge(*y.agg.snapshot_arrays())
    got = gpu_flows(x)
    assert_same_flows(got, orc.export())
    both = [k for k in fx if k in fy]
    assert both and all(got[k][0] == fx[k][0] and got[k][1] == fy[k][1] for k in both)


def test_ex_duplicate_keys_in_one_call_follow_row_order(gpu, oracle):
    from go2netspectra_amd import ExactTask
    rng = np.random.default_rng(10)
    s = ex_stream(rng, 30_000, 2000)
    a1, a2, orc = ExactTask("a1", FIVE), ExactTask("a2", FIVE), oracle.Exact(FIVE)
    ex_put(a1, orc, s, 0, 15_000)
    ex_put(a2, orc, s, 15_000, 30_000)
    rows = [np.concatenate([p, q]) for p, q in zip(a1.agg.snapshot_arrays(), a2.agg.snapshot_arrays())]
    z = ExactTask("z", FIVE)
    z.agg.merge(*rows)
    assert_same_flows(gpu_flows(z), orc.export())
    assert z.agg.counters()["flows"] < len(rows[3])  # some keys did occur twice


def sorted_rows(arrs):
    keys, st, en, pk, by = arrs
    order = np.lexsort(keys.T[::-1])
    return [np.ascontiguousarray(a[order]) for a in (keys, st, en, pk, by)]


def synthetic_rows(rng, n, K=37):
    keys = rng.integers(0, 256, (n, K), dtype=np.uint8)
    keys[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)  # distinct
    st = rng.integers(-(1 << 50), 1 << 50, n).astype(np.int64)
    en = st + rng.integers(0, 1 << 30, n)
    pk = rng.integers(2, 1 << 40, n).astype(np.uint64)
    by = rng.integers(0, 1 << 62, n).astype(np.uint64)
    return keys, st, en, pk, by


def test_ex_merge_grows_the_table(gpu):
    from go2netspectra_amd import ExactAggregator
    rng = np.random.default_rng(11)
    rows = synthetic_rows(rng, 100_000)
    ex = ExactAggregator(FIVE, max_flows=4096)
    slots0 = ex.dict_stats()["slots"]
    ex.merge(*rows)
    ds = ex.dict_stats()
    assert ds["growths"] > 0 and ds["slots"] > slots0, ds
    assert ex.counters()["flows"] == 100_000 and ex.counters()["dict_full"] == 0
    assert_same_arrays(("keys", "start", "end", "pkts", "bytes"), sorted_rows(ex.snapshot_arrays()), sorted_rows(rows))
    # u64 wrap of the counts, start kept, end taken
    k, st, en, pk, by = [a[:1000] for a in rows]
    ex.merge(k, st + 1, en + 5, np.full(1000, 2**64 - 1, np.uint64), np.full(1000, 2**63, np.uint64))
    want = sorted_rows((k, st, en + 5, pk - np.uint64(1), by + np.uint64(2**63)))
    got = sorted_rows(ex.snapshot_arrays())
    have = {bytes(r): i for i, r in enumerate(got[0])}
    idx = np.array([have[bytes(r)] for r in want[0]])
    assert_same_arrays(("keys", "start", "end", "pkts", "bytes"), [a[idx] for a in got], want)


def test_ex_device_rows_zero_packet_rows_and_the_query_plane(gpu, oracle):
    import torch
    from go2netspectra_amd import ExactTask
    from go2netspectra_amd.exact import make_filter
    rng = np.random.default_rng(13)
    s = ex_stream(rng, 30_000, 3000)
    x = ExactTask("x", FIVE)
    ex_put(x, None, s, 0, 30_000)
    keys, st, en, pk, by = x.agg.snapshot_arrays()
    # rows without packets are ignored: a flow exists iff it has packets
    ghost = synthetic_rows(rng, 50)
    rows = [np.concatenate([a, b]) for a, b in zip((keys, st, en, pk, by), ghost)]
    rows[3][len(pk):] = 0
    perm = rng.permutation(len(rows[3]))
    rows = [np.ascontiguousarray(a[perm]) for a in rows]
    host, dev = ExactTask("h", FIVE), ExactTask("d", FIVE)
    host.agg.merge(*rows)
    dev.agg.merge(torch.from_numpy(rows[0]).cuda(), torch.from_numpy(rows[1]).cuda(), torch.from_numpy(rows[2]).cuda(),
                  torch.from_numpy(rows[3].view(np.int64)).cuda(), torch.from_numpy(rows[4].view(np.int64)).cuda())
    want = gpu_flows(x)
    for t in (host, dev):
        assert_same_flows(gpu_flows(t), want, t.name())
        assert t.agg.counters()["flows"] == len(pk)
        assert t.agg.aggregate([make_filter()]) == x.agg.aggregate([make_filter()])
        flt = [make_filter(protocol=6), make_filter(src_port=int(s[0]["sport"][0]))]
        assert t.agg.aggregate(flt) == x.agg.aggregate(flt)
        for metric, thr, lim in ((0, 0, 0), (1, 0, 100), (0, 5, 0)):
            gk, gv = t.agg.heavy_hitters(metric, thr, lim)
            wk, wv = x.agg.heavy_hitters(metric, thr, lim)
            assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (t.name(), metric)
        assert np.array_equal(t.agg.query_many(keys[:500]), x.agg.query_many(keys[:500]))


# ---------------------------------------------------------------------------
# Python surface
# ---------------------------------------------------------------------------
THREE_TASKS = """
aggregator:
  types: ["sketch", "exact"]
  sketch:
    tasks:
      - {name: ss_src_dst, skt_type: 1, flow_fields: [SrcIP], element_fields: [DstIP], width: 4096, depth: 2,
         count_thereshold: 1, m: 128, size: 5, b: 1.08, base: 0.5}
      - {name: cm_src_left, skt_type: 0, flow_fields: [SrcIP], element_fields: [DstIP, SrcPort, DstPort, Protocol],
         width: 4096, depth: 2, size_thereshold: 100000, count_thereshold: 50}
  exact:
    tasks:
      - {name: per_five_tuple, key_fields: [SrcIP, DstIP, SrcPort, DstPort, Protocol]}
"""


def task_state(t):
    if hasattr(t, "sketch"):
        return [np.asarray(a).view(np.uint64) if np.asarray(a).dtype == np.float64 else np.asarray(a)
                for a in t.sketch.export_state()]
    return gpu_flows(t)


def test_manager_checkpoint_and_restore(gpu, tmp_path):
    from go2netspectra_amd import HeaderBatch, Manager, parse_config
    cfg = parse_config(THREE_TASKS)
    rng = np.random.default_rng(55)
    n, cut = 50_000, 27_001
    t = random_tuples(rng, n, 3000, v6_frac=0.2)
    hdr = frames_from_tuples(t, rng, vlan_frac=0.2)
    hdr[rng.random(n) < 0.03, 12:14] = [0x08, 0x06]
    ts = np.cumsum(rng.integers(0, 5000, n)).astype(np.int64)
    batch = lambda lo, hi: HeaderBatch(hdr[lo:hi], t["length"][lo:hi], ts[lo:hi])
    kw = dict(seeds=np.array([11, 22, 33, 44], np.uint32))
    whole, first, second = Manager(cfg, **kw), Manager(cfg, **kw), Manager(cfg, **kw)
    assert [x.name() for x in whole.tasks()] == ["ss_src_dst", "cm_src_left", "per_five_tuple"]
    whole.process(batch(0, cut))
    whole.process(batch(cut, n))
    first.process(batch(0, cut))
    paths = first.checkpoint(tmp_path / "ckpt")
    assert len(paths) == 3
    second.restore(tmp_path / "ckpt")
    second.process(batch(cut, n))
    want, got = whole.stop(), second.stop()
    for a, b in zip(whole.tasks(), second.tasks()):
        sa, sb = task_state(a), task_state(b)
        if isinstance(sa, dict):
            assert_same_flows(sb, sa, a.name())
        else:
            assert_same_arrays(["a0", "a1", "a2", "a3"], sb, sa, a.name() + " ")
        assert got[a.name()] == want[a.name()], a.name()
    # a file saved under other parameters is refused by name
    other = Manager(cfg, seeds=np.array([1, 2, 3, 4], np.uint32))
    with pytest.raises(ValueError, match="'seeds'"):
        other.restore(tmp_path / "ckpt")


def test_load_global_ends_the_exact_global_mode_on_the_device(gpu, oracle):
    from go2netspectra_amd import CountMin
    from go2netspectra_amd.dist import assemble_slices, bucket_slice, load_global
    rng = np.random.default_rng(77)
    w, d, K = 5000, 4, 16
    seeds = cm_seeds(d)
    keys, flows, _ = zipf_keys(rng, 20_000, 3000, K)
    sizes = sizes_u32(rng, 20_000)
    orc = oracle.CountMin(w, d, 1000, 10, K, seeds)
    orc.insert_keys(keys, sizes)
    states, ranges = [], []
    for r in range(2):
        rg = bucket_slice(r, 2, w)
        cm = CountMin(w, d, 1000, 10, key_bytes=K, seeds=seeds, bucket_range=rg)
        cm.insert_keys(keys, sizes)
        cm.flush()
        states.append(cm.export_state())
        ranges.append(rg)
        with pytest.raises(ValueError):
            load_global(cm, states[-1])  # a slice handle is no global sketch
        cm.close()
    glob = CountMin(w, d, 1000, 10, key_bytes=K, seeds=seeds)
    load_global(glob, assemble_slices(states, ranges, w, d))
    assert_same_arrays(CM_NAMES, glob.export_state(), orc.export())
    assert np.array_equal(glob.query_many(flows), np.array([orc.query(bytes(f)) for f in flows], np.uint64))
    assert_same_list(cm_lists(glob)[0], orc.heavy("count"))
    assert_same_list(cm_lists(glob)[1], orc.heavy("size"))
