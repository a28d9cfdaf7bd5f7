"""Exact spread engine on the GPU (gns_exs_*): every flow's spread against a
ground truth that shares no code with the engine -- numpy np.unique over the
rows flow bytes ‖ element bytes and a bincount per flow -- on keys built by the
host-side encoders (PacketBatch.keys, helpers.frame64, the golden parser vectors)."""
import ctypes as ct
import json
import os

import numpy as np
import pytest

from helpers import assert_same_flows, assert_same_list, frame64, zipf_index

pytestmark = pytest.mark.gpu

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def truth_of(fk: np.ndarray, ek: np.ndarray) -> dict:
    """flow bytes -> number of distinct rows flow ‖ elem."""
    if len(fk) == 0:
        return {}
    rows = np.ascontiguousarray(np.concatenate([fk, ek], axis=1))
    pairs = np.unique(rows.view(np.dtype((np.void, rows.shape[1]))).ravel())
    pf = np.ascontiguousarray(pairs.view(np.uint8).reshape(len(pairs), -1)[:, : fk.shape[1]])
    uf, inv = np.unique(pf.view(np.dtype((np.void, pf.shape[1]))).ravel(), return_inverse=True)
    cnt = np.bincount(inv.ravel(), minlength=len(uf))
    return {bytes(f): int(c) for f, c in zip(uf.tolist(), cnt)}


def snap(ex) -> dict:
    f, v = ex.snapshot_arrays()
    d = {bytes(f[i]): int(v[i]) for i in range(len(v))}
    assert len(d) == len(v), "snapshot lists a flow twice"
    return d


def keys4(idx) -> np.ndarray:
    """index -> a 16-byte IPv4 slot (4 bytes + 12 zero bytes), distinct per index."""
    idx = np.asarray(idx, np.uint32)
    k = np.zeros((len(idx), 16), np.uint8)
    k[:, :4] = (idx * np.uint32(2654435761)).astype(">u4").view(np.uint8).reshape(-1, 4)
    return k


def new_exact(**kw):
    from go2netspectra_amd import ExactSpread
    return ExactSpread(None, None, flow_bytes=16, elem_bytes=16, **kw)


# --- 1 ---------------------------------------------------------------------
def test_degenerate_sizes(gpu):
    from go2netspectra_amd import ExactSpread
    ex = ExactSpread(["SrcIP"], ["DstIP"])
    ex.insert_keys(np.zeros((0, 16), np.uint8), np.zeros((0, 16), np.uint8))
    ex.insert_headers(np.zeros((0, 64), np.uint8), np.zeros(0, np.uint32))
    ex.flush()
    assert snap(ex) == {}
    assert ex.counters()["inserted"] == 0
    a, b = keys4([7]), keys4([9])
    ex.insert_keys(a, b)
    ex.flush()
    assert snap(ex) == {bytes(a[0]): 1}
    # the same pair in every lane of many waves and workgroups: one claim wins the slot
    ex.reset()
    ex.insert_keys(np.repeat(a, 4096, axis=0), np.repeat(b, 4096, axis=0))
    ex.flush()
    assert snap(ex) == {bytes(a[0]): 1}
    c = ex.counters()
    assert c["new_pairs"] == 2 and c["flows"] == 1  # counters keep counting over a reset


# --- 2 ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one_batch", "batch700", "three_calls"])
def test_one_flow_many_elements(gpu, mode):
    rng = np.random.default_rng(5)
    el = keys4(np.repeat(np.arange(20_000), 3))
    rng.shuffle(el, axis=0)
    fl = np.repeat(keys4([1]), len(el), axis=0)
    ex = new_exact(batch_packets=700 if mode == "batch700" else 0)
    if mode == "three_calls":
        for part in np.array_split(np.arange(len(el)), 3):
            ex.insert_keys(fl[part], el[part])
    else:
        ex.insert_keys(fl, el)
    ex.flush()
    assert snap(ex) == {bytes(fl[0]): 20_000}
    assert ex.counters()["batches"] == {"one_batch": 1, "batch700": 86, "three_calls": 3}[mode]


# --- 3 ---------------------------------------------------------------------
def test_contention_both_ways(gpu):
    rng = np.random.default_rng(6)
    n = 100_000
    shared = keys4([5_000_000])
    fl = np.concatenate([keys4(np.arange(n)),                      # n flows share one element
                         np.repeat(keys4([6_000_000]), n, axis=0),  # one flow, n elements: one hot counter
                         np.repeat(keys4([7_000_000]), n, axis=0)])  # one pair, n times
    el = np.concatenate([np.repeat(shared, n, axis=0), keys4(1_000_000 + np.arange(n)),
                         np.repeat(keys4([8_000_000]), n, axis=0)])
    perm = rng.permutation(len(fl))
    fl, el = fl[perm], el[perm]
    want = truth_of(fl, el)
    assert len(want) == n + 2 and want[bytes(keys4([6_000_000])[0])] == n and want[bytes(keys4([7_000_000])[0])] == 1
    ex = new_exact()
    ex.insert_keys(fl, el)
    ex.flush()
    assert_same_flows(snap(ex), want)
    assert ex.counters()["new_pairs"] == 2 * n + 1


# --- 4, 9 ------------------------------------------------------------------
def growth_stream():
    rng = np.random.default_rng(7)
    n = 300_000
    fi = zipf_index(rng, n, 3000, 1.1)
    ei = rng.integers(0, 1300, n)  # a pool per flow: the hot flows saturate it, about half the packets repeat a pair
    return keys4(fi), keys4(100_000 + fi * 1300 + ei)


def test_growth(gpu):
    fl, el = growth_stream()
    want = truth_of(fl, el)
    npairs = sum(want.values())
    assert 100_000 < npairs < 200_000 and len(want) > 2000
    ex = new_exact(max_flows=64, max_pairs=256, batch_packets=5000)
    assert ex.dict_stats()["flow_slots"] == 128 and ex.dict_stats()["pair_slots"] == 512
    # small calls first, so that both tables also grow while they hold records
    for lo, hi in ((0, 60), (60, 700), (700, len(fl))):
        ex.insert_keys(fl[lo:hi], el[lo:hi])
    ex.flush()
    got = snap(ex)
    assert_same_flows(got, want)
    ds = ex.dict_stats()
    assert ds["flow_growths"] >= 2 and ds["pair_growths"] >= 2, ds
    assert ds["flows_claimed"] == len(want) and ds["pairs_claimed"] == npairs
    big = new_exact()
    big.insert_keys(fl, el)
    big.flush()
    assert big.dict_stats()["flow_growths"] == 0 and big.dict_stats()["pair_growths"] == 0
    assert_same_flows(snap(big), got)
    # queries and the heavy list read through the grown tables
    probe = keys4(np.arange(0, 3000, 7))
    assert_same_list(ex.query_many(probe).tolist(), [want.get(bytes(k), 0) for k in probe])

    # 9: reset after a growth, then half the stream
    ex.reset()
    assert snap(ex) == {}
    h = len(fl) // 2
    ex.insert_keys(fl[:h], el[:h])
    ex.flush()
    assert_same_flows(snap(ex), truth_of(fl[:h], el[:h]))


def test_growth_wide_keys(gpu):
    """37 + 37 key bytes: the 20-word probe helpers and 128-byte records, through growths."""
    from go2netspectra_amd import ExactSpread
    rng = np.random.default_rng(11)
    n = 30_000
    flows = rng.integers(0, 256, (200, 37), dtype=np.uint8)
    elems = rng.integers(0, 256, (3000, 37), dtype=np.uint8)
    elems[:, :36] = elems[0, :36]  # elements that differ in their last byte only (and many equal ones)
    fl = np.ascontiguousarray(flows[zipf_index(rng, n, 200, 1.1)])
    el = np.ascontiguousarray(elems[rng.integers(0, 3000, n)])
    want = truth_of(fl, el)
    assert max(want.values()) > 100
    ex = ExactSpread(None, None, flow_bytes=37, elem_bytes=37, max_flows=8, max_pairs=64, batch_packets=3000)
    for lo, hi in ((0, 40), (40, 400), (400, n)):
        ex.insert_keys(fl[lo:hi], el[lo:hi])
    ex.flush()
    assert_same_flows(snap(ex), want)
    ds = ex.dict_stats()
    assert ds["flow_growths"] >= 2 and ds["pair_growths"] >= 2, ds
    assert ds["pairs_claimed"] == sum(want.values())
    rec = ex.heavy_hitters(100)
    assert_same_list([(h.Flow, h.Count) for h in rec.Count],
                     sorted(((k, v) for k, v in want.items() if v >= 100), key=lambda kv: (-kv[1], kv[0])))


def test_reset(gpu):
    fl, el = growth_stream()
    fl, el = fl[:60_000], el[:60_000]
    ex = new_exact()
    ex.insert_keys(fl, el)
    ex.flush()
    assert_same_flows(snap(ex), truth_of(fl, el))
    ex.reset()
    assert snap(ex) == {} and ex.query_many(fl[:50]).tolist() == [0] * 50
    assert ex.heavy_hitters(1).Count == []
    ex.insert_keys(fl[:30_000], el[:30_000])
    ex.flush()
    assert_same_flows(snap(ex), truth_of(fl[:30_000], el[:30_000]))


# --- 5 ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_packets():
    """40K packets, 30 % IPv6: Zipf sources, destinations from a pool of the source's IP
    version, a few ports: every layout below sees repeated and distinct pairs."""
    rng = np.random.default_rng(8)
    n, nsrc, ndst = 40_000, 300, 3000
    v6s = rng.random(nsrc) < 0.3
    src = np.zeros((nsrc, 16), np.uint8)
    src[:, :4] = rng.integers(0, 256, (nsrc, 4))
    src[v6s] = rng.integers(0, 256, (int(v6s.sum()), 16))
    dst4 = np.zeros((ndst, 16), np.uint8)
    dst4[:, :4] = rng.integers(0, 256, (ndst, 4))
    dst6 = rng.integers(0, 256, (ndst, 16), dtype=np.uint8)
    si = zipf_index(rng, n, nsrc, 1.1)
    di = rng.integers(0, ndst, n)
    v6 = v6s[si]
    t = dict(src16=src[si], dst16=np.where(v6[:, None], dst6[di], dst4[di]),
             sport=rng.choice(np.array([53, 80, 443, 8080, 50000], np.uint16), n),
             dport=rng.choice(np.arange(1000, 1016, dtype=np.uint16), n),
             proto=np.where(rng.random(n) < 0.7, 6, 17).astype(np.uint8),
             length=rng.integers(100, 1519, n).astype(np.uint32), v6=v6)  # whole L4 headers on the wire
    hdr = np.zeros((n, 64), np.uint8)
    for i in range(n):
        hdr[i] = np.frombuffer(frame64(t["src16"][i], t["dst16"][i], t["sport"][i], t["dport"][i], t["proto"][i],
                                       int(t["length"][i]), v6=bool(v6[i])), np.uint8)
    return t, hdr


@pytest.mark.parametrize("flow,elem", [
    (["SrcIP"], ["DstIP"]),
    (["DstIP"], ["SrcIP"]),                                     # the shape ss_test.go uses
    (["SrcIP", "DstPort"], ["DstIP", "SrcPort", "Protocol"]),   # generic byte-table plan
    (FIVE, ["SrcIP"]),                                          # 37 + 16 bytes
    (["SrcIP", "DstIP", "Protocol"], FIVE),                     # 33 + 37 bytes: 128-byte pair records
])
def test_layouts_and_entry_points(gpu, mixed_packets, flow, elem):
    import torch
    from go2netspectra_amd import ExactSpread, PacketBatch
    t, hdr = mixed_packets
    batch = PacketBatch(t["src16"], t["dst16"], t["sport"], t["dport"], t["proto"], t["length"])
    fk, ek = batch.keys(flow), batch.keys(elem)
    want = truth_of(fk, ek)
    assert len(want) > 100 and sum(want.values()) < len(fk)  # many flows, and pairs that repeat
    dev = torch.device("cuda", 0)
    feeds = {
        "keys": lambda ex: ex.insert_keys(fk, ek),
        "keys_dev": lambda ex: ex.insert_keys(torch.from_numpy(fk).to(dev), torch.from_numpy(ek).to(dev)),
        "tuples": lambda ex: ex.insert_tuples(batch),
        "tuples_dev": lambda ex: ex.insert_tuples(batch.to(dev)),
        "headers": lambda ex: ex.insert_headers(hdr, t["length"]),
        "headers_dev": lambda ex: ex.insert_headers(torch.from_numpy(hdr).to(dev),
                                                    torch.from_numpy(t["length"].view(np.int32)).to(dev)),
    }
    for name, feed in feeds.items():
        ex = ExactSpread(flow, elem, batch_packets=9000)
        feed(ex)
        ex.flush()
        assert_same_flows(snap(ex), want, name)
        assert ex.counters()["inserted"] == len(fk), name
        ex.close()


def test_pair_order_matters(gpu):
    a, b = keys4([1])[:, :4], keys4([2])[:, :4]
    from go2netspectra_amd import ExactSpread
    ex = ExactSpread(None, None, flow_bytes=4, elem_bytes=4)
    ex.insert_keys(np.concatenate([a, b, a, b, a]), np.concatenate([b, a, a, b, b]))
    ex.flush()
    assert snap(ex) == {bytes(a[0]): 2, bytes(b[0]): 2}


# --- 6 ---------------------------------------------------------------------
def test_record_handling_matches_superspread(gpu, mixed_packets):
    """Good frames interleaved with every golden parser vector (non-IP ethertypes,
    unsupported shapes, truncated records): the kept set is the truth over the
    records the parser keeps, and the three record counters equal SuperSpread's."""
    from go2netspectra_amd import ExactSpread, SuperSpread
    t, hdr = mixed_packets
    vec = json.load(open(os.path.join(GOLD, "parse_vectors.json")))["vectors"]
    by_status = {s: [v for v in vec if v["status"] == s] for s in (0, 1, 2)}
    assert by_status[1] and by_status[2] and any("trunc" in v["name"] for v in vec)
    good = 3000
    recs, wl, fk, ek = [], [], [], []
    for i in range(good):
        recs.append(hdr[i]); wl.append(int(t["length"][i])); fk.append(t["src16"][i]); ek.append(t["dst16"][i])
        v = vec[i % len(vec)]
        recs.append(np.frombuffer(bytes.fromhex(v["record"]), np.uint8)); wl.append(v["wirelen"])
        if v["status"] == 0:
            fk.append(np.frombuffer(bytes.fromhex(v["src16"]), np.uint8))
            ek.append(np.frombuffer(bytes.fromhex(v["dst16"]), np.uint8))
    recs, wl = np.ascontiguousarray(np.stack(recs)), np.array(wl, np.uint32)
    fk, ek = np.stack(fk), np.stack(ek)
    reps = [sum(1 for i in range(good) if vec[i % len(vec)]["status"] == s) for s in (0, 1, 2)]
    ex = ExactSpread(["SrcIP"], ["DstIP"], batch_packets=1000)
    ss = SuperSpread(1 << 10, 2, 50, 128, 5, flow_fields=["SrcIP"], elem_fields=["DstIP"])
    ex.insert_headers(recs, wl)
    ss.insert_headers(recs, wl)
    ex.flush()
    ss.flush()
    assert_same_flows(snap(ex), truth_of(fk, ek))
    ce, cs = ex.counters(), ss.counters()
    assert (ce["inserted"], ce["dropped"], ce["unsupported"]) == (good + reps[0], reps[1], reps[2])
    assert (ce["inserted"], ce["dropped"], ce["unsupported"]) == (cs["inserted"], cs["dropped"], cs["unsupported"])


# --- 7 ---------------------------------------------------------------------
def test_heavy_list(gpu):
    rng = np.random.default_rng(9)
    spreads = np.concatenate([np.full(50, 10), np.full(50, 11), rng.integers(1, 10, 200)])
    fidx = rng.permutation(300)
    fl = keys4(np.repeat(fidx, spreads))
    el = keys4(np.concatenate([1000 + np.arange(s) for s in spreads]))
    fl, el = np.concatenate([fl, fl[::3]]), np.concatenate([el, el[::3]])  # duplicates change nothing
    perm = rng.permutation(len(fl))
    ex = new_exact()
    ex.insert_keys(fl[perm], el[perm])
    ex.flush()
    want = truth_of(fl, el)
    ordered = sorted(((k, v) for k, v in want.items()), key=lambda kv: (-kv[1], kv[0]))
    for thr, n in ((10, 100), (11, 50), (12, 0)):
        rec = ex.heavy_hitters(thr)
        assert rec.Size is None
        assert_same_list([(h.Flow, h.Count) for h in rec.Count], [kv for kv in ordered if kv[1] >= thr], f"thr {thr}")
        assert len(rec.Count) == n
    # capacity 5 against a list of 100: the length is reported, the buffers stay as they were
    f = np.full((5, 16), 0xAB, np.uint8)
    v = np.full(5, 0xCDCDCDCD, np.uint32)
    n = ct.c_uint64(5)
    assert ex._L.gns_exs_heavy_hitters(ex._h, 10, f.ctypes.data, v.ctypes.data, ct.byref(n)) == 0
    assert n.value == 100 and (f == 0xAB).all() and (v == 0xCDCDCDCD).all()
    assert ex.heavy_hitters_arrays(10, capacity=5)[2] == 100
    f100, v100, n100 = ex.heavy_hitters_arrays(10, capacity=100)
    assert n100 == 100 and [(bytes(a), int(b)) for a, b in zip(f100, v100)] == ordered[:100]


# --- 8 ---------------------------------------------------------------------
def test_query(gpu):
    import torch
    fl, el = growth_stream()
    fl, el = fl[:50_000], el[:50_000]
    want = truth_of(fl, el)
    ex = new_exact()
    ex.insert_keys(fl, el)
    ex.flush()
    probe = np.concatenate([keys4(np.arange(0, 3000, 3)), keys4(9_000_000 + np.arange(200))])  # seen and unseen
    host = ex.query_many(probe)
    assert host.dtype == np.uint64
    assert_same_list(host.tolist(), [want.get(bytes(k), 0) for k in probe])
    assert (host[-200:] == 0).all() and ex.query(bytes(probe[-1])) == 0
    devq = ex.query_many(torch.from_numpy(probe).to("cuda:0"))
    assert devq.is_cuda and devq.dtype == torch.int64
    assert_same_list(devq.cpu().numpy().tolist(), host.astype(np.int64).tolist())
    if torch.cuda.device_count() > 1:
        other = torch.from_numpy(probe).to("cuda:1")
        with pytest.raises(ValueError):
            ex.query_many(other)
        with pytest.raises(ValueError):
            ex.insert_keys(other, other)


# --- 10 --------------------------------------------------------------------
def test_accuracy_protocol_end_to_end(gpu):
    """ss_test.go:86-136 on the stream of test_ss_gpu.test_superspreader_accuracy (1.5M
    packets, 20,000 sources, 400,000 destinations, w=2^13, d=2, m=128, threshold 750):
    ExactSpread is the numpy truth for every flow, and spread_report's numbers equal the
    ones worked out on the host from numpy sets.  are: the device sums in float64 in
    another order than numpy, n * 2^-53 relative at worst, far inside 1e-9."""
    from go2netspectra_amd import SuperSpread
    from go2netspectra_amd.accuracy import spread_report
    rng = np.random.default_rng(21)
    n, nsrc, ndst, thr = 1_500_000, 20_000, 400_000, 750
    src = rng.integers(0, 256, (nsrc, 16), dtype=np.uint8)
    src[:, 4:] = 0
    dst = rng.integers(0, 256, (ndst, 16), dtype=np.uint8)
    dst[:, 4:] = 0
    si = zipf_index(rng, n, nsrc, 1.1)
    di = rng.integers(0, ndst, n)
    fl, el = np.ascontiguousarray(src[si]), np.ascontiguousarray(dst[di])
    seeds = np.random.default_rng(1).integers(0, 2**32, 2, dtype=np.uint64).astype(np.uint32)
    ss = SuperSpread(1 << 13, 2, thr, 128, 5, 0.5, 1.08, flow_bytes=16, elem_bytes=16, seeds=seeds,
                     hll_master=0x0123456789ABCDEF, rng_seed=0x0DDBA11CAFEF00D5)
    ex = new_exact()
    ss.insert_keys(fl, el)
    ex.insert_keys(fl, el)
    ss.flush()
    ex.flush()
    # truth: distinct (source address, destination address) words, counted per source address
    f4 = fl[:, :4].copy().view(">u4").ravel().astype(np.uint64)
    e4 = el[:, :4].copy().view(">u4").ravel().astype(np.uint64)
    pairs = np.unique(f4 << np.uint64(32) | e4)
    uf, cnt = np.unique(pairs >> np.uint64(32), return_counts=True)
    ukeys = np.zeros((len(uf), 16), np.uint8)
    ukeys[:, :4] = uf.astype(">u4").view(np.uint8).reshape(-1, 4)
    want = {bytes(k): int(c) for k, c in zip(ukeys, cnt)}
    assert_same_flows(snap(ex), want)

    rep = spread_report(ss, ex, thr)
    print("spread_report:", json.dumps(rep))
    est = ss.query_many(ukeys).astype(np.float64)
    are = float(np.mean(np.abs(est - cnt) / cnt))
    true_ss = {k for k, c in want.items() if c >= thr}
    det = {h.Flow for h in ss.heavy_hitters().Count}
    assert rep["flows"] == len(want) and rep["true_superspreaders"] == len(true_ss) > 10
    assert (rep["tp"], rep["fp"], rep["fn"]) == (len(true_ss & det), len(det - true_ss), len(true_ss - det))
    assert abs(rep["are"] - are) <= 1e-9 * are
    assert rep["precision"] == rep["tp"] / max(1, rep["tp"] + rep["fp"])
    assert rep["recall"] == rep["tp"] / max(1, rep["tp"] + rep["fn"])
    assert rep["recall"] >= 0.8 and rep["precision"] >= 0.8
