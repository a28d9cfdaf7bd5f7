"""Host inputs through the engines' shared staging (gns_common HostStage) and the
shared dictionary recovery (DictRecovery).

Staging: for every engine and every input kind it accepts, two handles with the
same parameters and the engine's smallest batch (one chunk).  One is fed HOST arrays
in one call that spans three batches with a ragged tail; the other the same records
as DEVICE tensors in two calls split at n // 3, so its batch boundaries differ.
Every engine's result is independent of where a batch ends, so exported state,
heavy-hitter lists and the counters that count records (not batches or chunks of a
batch) must be identical.

Recovery: a two-chunk host batch of all-new flows against a dictionary too small
for it has to reclaim, retry and split; the result is the oracle's and the retries
are counted."""
import numpy as np
import pytest

from helpers import assert_same_list, frames_from_tuples, random_tuples, sizes_u32, zipf_index

pytestmark = pytest.mark.gpu

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
CHUNK = 16384       # kChunk (gns_cm.hip), kSsChunk (gns_ss.hip), kXChunk (gns_exact.hip)
EXS_CHUNK = 4096    # kExsChunk (gns_spread.hip)
N = 2 * CHUNK + 777
NFLOWS = 3000


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(view.get(a.dtype, a.dtype))).to("cuda")


@pytest.fixture(scope="module")
def world():
    """One stream of N packets over NFLOWS 5-tuples (a fifth of them IPv6) in every input form.
    The sources come from a pool of 200 per IP version, so a source meets many
    destinations (the spread engines' flows) and a few thousand 5-tuples remain."""
    from go2netspectra_amd.packets import PacketBatch
    rng = np.random.default_rng(20261019)
    t = random_tuples(rng, N, NFLOWS, v6_frac=0.2)
    pool4 = np.zeros((200, 16), np.uint8)
    pool4[:, :4] = rng.integers(0, 256, (200, 4))
    pool6 = rng.integers(0, 256, (200, 16), dtype=np.uint8)
    who = zipf_index(rng, N, 200, 0.8)
    t["src16"] = np.where(t["v6"][:, None], pool6[who], pool4[who])
    ts = np.cumsum(rng.integers(1, 1000, N)).astype(np.int64) + 1_700_000_000_000_000_000
    batch = PacketBatch(t["src16"], t["dst16"], t["sport"], t["dport"], t["proto"], t["length"],
                        np.where(t["v6"], 6, 4).astype(np.uint8), ts)
    return dict(batch=batch, keys=batch.keys(FIVE), hdr=frames_from_tuples(t, rng, vlan_frac=0.1),
                wl=t["length"], ts=ts)


def batch_slice(b, lo, hi, device):
    from go2netspectra_amd.packets import PacketBatch
    s = PacketBatch(b.src16[lo:hi], b.dst16[lo:hi], b.sport[lo:hi], b.dport[lo:hi], b.proto[lo:hi], b.length[lo:hi],
                    b.ipver[lo:hi], b.ts[lo:hi])
    return s.to("cuda") if device else s


def feed(host, devh, n, insert):
    """insert(handle, lo, hi, device): the host handle in one call, the device handle in two."""
    insert(host, 0, n, False)
    insert(devh, 0, n // 3, True)
    insert(devh, n // 3, n, True)
    host.flush()
    devh.flush()


def same_counters(a, b, names):
    ca, cb = a.counters(), b.counters()
    assert {k: ca[k] for k in names} == {k: cb[k] for k in names}
    return ca


# --- Count-Min ---------------------------------------------------------------
def cm_insert(kind, w):
    from go2netspectra_amd import compact_headers
    if kind == "keys":
        return lambda h, lo, hi, d: h.insert_keys(dev(w["keys"][lo:hi]) if d else w["keys"][lo:hi],
                                                  dev(w["wl"][lo:hi]) if d else w["wl"][lo:hi])
    if kind == "tuples":
        return lambda h, lo, hi, d: h.insert_tuples(batch_slice(w["batch"], lo, hi, d))
    if kind == "headers":
        return lambda h, lo, hi, d: h.insert_headers(dev(w["hdr"][lo:hi]) if d else w["hdr"][lo:hi],
                                                     dev(w["wl"][lo:hi]) if d else w["wl"][lo:hi])
    emb = kind == "compact16"  # the 16-byte form: wire lengths inside the records, IPv6 escapes to the side array
    rec, side = compact_headers(dev(w["hdr"]), dev(w["wl"]), rec_len=emb)
    assert len(side) > 0, "the stream must hold a side-record escape"
    hrec, hside = rec.cpu().numpy(), side.cpu().numpy()

    def ins(h, lo, hi, d):  # escapes index the side array of the whole stream
        if d:
            h.insert_compact(rec[lo:hi], None if emb else dev(w["wl"][lo:hi]), side)
        else:
            h.insert_compact(hrec[lo:hi], None if emb else w["wl"][lo:hi], hside)
    return ins


@pytest.mark.parametrize("kind", ["keys", "tuples", "headers", "compact", "compact16"])
def test_count_min(gpu, world, kind):
    from go2netspectra_amd import CountMin
    seeds = np.random.default_rng(3).integers(0, 2**32, 3, dtype=np.uint64).astype(np.uint32)
    kw = dict(key_bytes=37) if kind == "keys" else dict(flow_fields=FIVE)
    a, b = (CountMin(1024, 3, 4000, 8, seeds=seeds, batch_packets=CHUNK, **kw) for _ in range(2))
    feed(a, b, N, cm_insert(kind, world))
    for name, x, y in zip(("C", "S", "FPc", "FPs"), a.export_state(), b.export_state()):
        assert np.array_equal(x, y), name
    ha, hb = a.heavy_hitters(), b.heavy_hitters()
    assert len(ha.Count) > 10 and len(ha.Size) > 10
    assert_same_list([(h.Flow, h.Count) for h in ha.Count], [(h.Flow, h.Count) for h in hb.Count], "count list")
    assert_same_list([(h.Flow, h.Size) for h in ha.Size], [(h.Flow, h.Size) for h in hb.Size], "size list")
    c = same_counters(a, b, ["inserted", "dropped", "unsupported", "dict_full", "ovf_full"])
    assert c["inserted"] == N


# --- SuperSpread and the exact spread engine ----------------------------------
def spread_insert(kind, w):
    fl, el = w["batch"].src16, w["batch"].dst16
    if kind == "keys":
        return lambda h, lo, hi, d: h.insert_keys(dev(fl[lo:hi]) if d else fl[lo:hi], dev(el[lo:hi]) if d else el[lo:hi])
    if kind == "tuples":
        return lambda h, lo, hi, d: h.insert_tuples(batch_slice(w["batch"], lo, hi, d))
    return lambda h, lo, hi, d: h.insert_headers(dev(w["hdr"][lo:hi]) if d else w["hdr"][lo:hi],
                                                 dev(w["wl"][lo:hi]) if d else w["wl"][lo:hi])


@pytest.mark.parametrize("kind", ["keys", "tuples", "headers"])
def test_super_spread(gpu, world, kind):
    from go2netspectra_amd import SuperSpread
    seeds = np.random.default_rng(4).integers(0, 2**32, 2, dtype=np.uint64).astype(np.uint32)
    kw = dict(flow_bytes=16, elem_bytes=16) if kind == "keys" else dict(flow_fields=["SrcIP"], elem_fields=["DstIP"])
    a, b = (SuperSpread(512, 2, 2, 32, 5, seeds=seeds, batch_packets=CHUNK, **kw) for _ in range(2))
    feed(a, b, N, spread_insert(kind, world))
    for name, x, y in zip(("values", "keys", "regs", "pbits"), a.export_state(), b.export_state()):
        assert np.array_equal(x.view(np.uint64) if name == "pbits" else x, y.view(np.uint64) if name == "pbits" else y), name
    ha, hb = a.heavy_hitters().Count, b.heavy_hitters().Count
    assert len(ha) > 10
    assert_same_list([(h.Flow, h.Count) for h in ha], [(h.Flow, h.Count) for h in hb], "spread list")
    c = same_counters(a, b, ["inserted", "dropped", "unsupported", "dict_full", "records"])
    assert c["records"] == N


@pytest.mark.parametrize("kind", ["keys", "tuples", "headers"])
def test_exact_spread(gpu, world, kind):
    from go2netspectra_amd import ExactSpread
    n = 2 * EXS_CHUNK + 777
    mk = (lambda: ExactSpread(None, None, flow_bytes=16, elem_bytes=16, batch_packets=EXS_CHUNK)) if kind == "keys" \
        else (lambda: ExactSpread(["SrcIP"], ["DstIP"], batch_packets=EXS_CHUNK))
    a, b = mk(), mk()
    feed(a, b, n, spread_insert(kind, world))
    sa, sb = ({bytes(f): int(v) for f, v in zip(*h.snapshot_arrays())} for h in (a, b))
    assert len(sa) > 100 and sa == sb
    fa, va = a.heavy_hitters_arrays(2)
    fb, vb = b.heavy_hitters_arrays(2)
    assert len(va) > 10 and np.array_equal(fa, fb) and np.array_equal(va, vb)
    c = same_counters(a, b, ["inserted", "dropped", "unsupported", "probe_full", "new_pairs", "flows", "records"])
    assert c["records"] == n


# --- the exact aggregator ------------------------------------------------------
@pytest.mark.parametrize("kind", ["tuples", "headers"])
def test_exact(gpu, world, kind):
    from go2netspectra_amd.exact import ExactAggregator
    w = world
    a, b = (ExactAggregator(FIVE, batch_packets=CHUNK) for _ in range(2))
    if kind == "tuples":
        ins = lambda h, lo, hi, d: h.insert_tuples(batch_slice(w["batch"], lo, hi, d))
    else:
        ins = lambda h, lo, hi, d: h.insert_headers(*((dev(w[k][lo:hi]) if d else w[k][lo:hi]) for k in ("hdr", "wl", "ts")))
    feed(a, b, N, ins)

    def state(h):  # dictionary slot order depends on the claim order: compare by key
        keys, st, en, pk, by = h.snapshot_arrays()
        o = np.lexsort(keys.T[::-1])
        return keys[o], st[o], en[o], pk[o], by[o]

    sa, sb = state(a), state(b)
    assert len(sa[0]) > 1000
    for name, x, y in zip(("keys", "start", "end", "packets", "bytes"), sa, sb):
        assert np.array_equal(x, y), name
    for metric in (0, 1):
        (ka, va), (kb, vb) = a.heavy_hitters(metric, 0, 50), b.heavy_hitters(metric, 0, 50)
        assert len(va) == 50 and np.array_equal(ka, kb) and np.array_equal(va, vb)
    c = same_counters(a, b, ["inserted", "dropped", "unsupported", "dict_full", "flows", "records"])
    assert c["records"] == N


# --- dictionary recovery with host input ---------------------------------------
def test_count_min_host_batch_reclaims_retries_and_splits(gpu, oracle):
    """One two-chunk host batch of all-new flows per call; 4096 slots hold 3072 claims,
    so every batch aborts, is retried on a rebuilt dictionary and split (the table then
    grows to hold a chunk's flows beside the live ones).  Oracle-exact, retries counted."""
    from go2netspectra_amd import CountMin
    rng = np.random.default_rng(77)
    w, d, K = 256, 2, 16
    seeds = np.random.default_rng(1).integers(0, 2**32, d, dtype=np.uint64).astype(np.uint32)
    cm = CountMin(w, d, 1000, 10, key_bytes=K, seeds=seeds, max_flows=2048, batch_packets=2 * CHUNK)
    orc = oracle.CountMin(w, d, 1000, 10, K, seeds)
    for _ in range(2):
        keys = rng.integers(0, 256, (2 * CHUNK, K), dtype=np.uint8)
        sizes = sizes_u32(rng, len(keys))
        cm.insert_keys(keys, sizes)
        orc.insert_keys(keys, sizes)
    cm.flush()
    for name, x, y in zip(("C", "S", "FPc", "FPs"), cm.export_state(), orc.export()):
        assert np.array_equal(x, y), name
    ds = cm.dict_stats()
    assert ds["retried_batches"] > 0 and ds["reclaims"] > 0, ds
    assert cm.counters()["dict_full"] == 0
    assert_same_list([(h.Flow, h.Count) for h in cm.heavy_hitters().Count], orc.heavy("count"))


def test_super_spread_host_batch_reclaims_retries_and_splits(gpu, oracle):
    """As above for SuperSpread: the flows that encode in a two-chunk batch of new
    sources overflow a 4096-slot dictionary."""
    from go2netspectra_amd import SuperSpread
    rng = np.random.default_rng(78)
    w, d, m = 256, 2, 32
    seeds = np.random.default_rng(1).integers(0, 2**32, d, dtype=np.uint64).astype(np.uint32)
    hm, rs = 0x1234ABCD5678EF01, 0x0DDBA11CAFEF00D5
    ss = SuperSpread(w, d, 20, m, 5, 0.5, 1.08, flow_bytes=16, elem_bytes=16, seeds=seeds, hll_master=hm, rng_seed=rs,
                     max_flows=2048, batch_packets=2 * CHUNK)
    orc = oracle.SuperSpread(w, d, 20, m, 5, 0.5, 1.08, 16, 16, seeds, hm, rs)
    for _ in range(2):
        fl = rng.integers(0, 256, (2 * CHUNK, 16), dtype=np.uint8)
        el = rng.integers(0, 256, (2 * CHUNK, 16), dtype=np.uint8)
        ss.insert_keys(fl, el)
        orc.insert(fl, el)
    ss.flush()
    for name, x, y in zip(("values", "keys", "regs", "pbits"), ss.export_state(), orc.export()):
        assert np.array_equal(x.view(np.uint64) if name == "pbits" else x, y.view(np.uint64) if name == "pbits" else y), name
    ds = ss.dict_stats()
    assert ds["retried_batches"] > 0 and ds["reclaims"] > 0, ds
    assert ss.counters()["dict_full"] == 0
    assert_same_list([(h.Flow, h.Count) for h in ss.heavy_hitters().Count], orc.heavy())


# --- point queries through the shared staging (query_keys) ----------------------
SENTINEL = 0xEEEEEEEEEEEEEEEE


def query_engine(name, w):
    """(the object to close last, raw handle, host query, device query or None, keys [>= 257, K],
    what a handle without a device query is compared with)."""
    from go2netspectra_amd import CountMin, ExactSpread, SuperSpread, _lib
    from go2netspectra_amd.exact import ExactAggregator
    L = _lib.load()
    rng = np.random.default_rng(len(name))
    b = w["batch"]
    if name in ("cm", "cm_view"):
        seeds = np.random.default_rng(3).integers(0, 2**32, 3, dtype=np.uint64).astype(np.uint32)
        h = CountMin(1 << 14, 3, 4000, 8, seeds=seeds, key_bytes=37)
        h.insert_keys(w["keys"], w["wl"])
        present = w["keys"]
        fns = (L.gns_cm_query, L.gns_cm_query_device)
    elif name in ("ss", "ss_view"):
        seeds = np.random.default_rng(4).integers(0, 2**32, 2, dtype=np.uint64).astype(np.uint32)
        h = SuperSpread(512, 2, 2, 32, 5, seeds=seeds, flow_bytes=16, elem_bytes=16)
        h.insert_keys(b.src16, b.dst16)
        present = b.src16
        fns = (L.gns_ss_query, L.gns_ss_query_device)
    elif name == "exact":
        h = ExactAggregator(FIVE)
        h.insert_tuples(b)
        present, v4 = w["keys"].copy(), b.ipver == 4
        for off in (0, 16):  # an IPv4 flow is found through its IPv4-mapped form (task.go:298-326)
            present[v4, off + 12:off + 16] = w["keys"][v4, off:off + 4]
            present[v4, off:off + 10] = 0
            present[v4, off + 10:off + 12] = 0xFF
        fns = (L.gns_ex_query, L.gns_ex_query_device)
    else:
        h = ExactSpread(None, None, flow_bytes=16, elem_bytes=16)
        h.insert_keys(b.src16, b.dst16)
        present = b.src16
        fns = (L.gns_exs_query, L.gns_exs_query_device)
    h.flush()
    present = np.unique(present, axis=0)
    keys = np.concatenate([present[:250], rng.integers(0, 256, (257 - min(250, len(present)), present.shape[1]),
                                                       dtype=np.uint8)])
    keys = np.ascontiguousarray(keys[rng.permutation(len(keys))])
    if name == "cm_view":
        v = h.view()
        v.refresh()
        want = h.query_many(dev(keys)).cpu().numpy().view(np.uint64)  # the handle at the refresh point
        return (v, h), v._h, L.gns_cm_view_query, None, keys, want
    if name == "ss_view":
        v = h.view()
        v.refresh()
        return (v, h), v._h, L.gns_ss_view_query, L.gns_ss_view_query_device, keys, None
    return (h,), h._h, fns[0], fns[1], keys, None


@pytest.mark.parametrize("name", ["cm", "ss", "exact", "spread", "cm_view", "ss_view"])
def test_host_and_device_queries_agree(gpu, world, name):
    """A query of host keys (staged through the handle's grow-only scratch; a SuperSpread view's
    through its pinned memory) answers what the query of the same keys in device memory does,
    at one key, a full block and one past it; the argument checks are the same for both."""
    import torch
    from go2netspectra_amd import _lib
    owners, h, host_fn, dev_fn, keys, want = query_engine(name, world)
    K = keys.shape[1]
    dkeys = dev(keys)
    torch.cuda.synchronize()

    def host(n, lo=0, stride=K):
        out = np.full(n + 1, SENTINEL, np.uint64)
        return host_fn(h, keys[lo:].ctypes.data, stride, n, out.ctypes.data), out

    def device(n, stride=K, skew=0):
        out = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        code = dev_fn(h, dkeys.data_ptr(), stride, n, out.data_ptr() + skew)
        return code, out.cpu().numpy().view(np.uint64)

    answers = {}
    for n in (257, 1, 256):  # the largest first: the later calls reuse its scratch
        code, got = host(n)
        assert code == 0 and got[n] == SENTINEL
        answers[n] = got[:n]
        if dev_fn is not None:
            code, d = device(n)
            assert code == 0 and d[n] == 2**64 - 1
            want_n = d[:n]
        else:
            want_n = want[:n]
        assert np.array_equal(got[:n], want_n), f"{name}: host and device answers differ at n={n}"
    # not a comparison of zeros: 250 of the keys were inserted (a sketch answers for those that own a cell)
    assert int((answers[257] != 0).sum()) >= 26
    assert np.array_equal(answers[1], answers[257][:1]) and np.array_equal(answers[256], answers[257][:256])
    code, one = host(1, lo=200)  # one key after 257: the larger scratch is reused
    assert code == 0 and one[0] == answers[257][200] and one[1] == SENTINEL
    # n = 0 is fine and writes nothing; a stride below the key size is an argument error
    code, got = host(0)
    assert code == 0 and got[0] == SENTINEL
    assert host(4, stride=K - 1)[0] == _lib.GNS_E_ARG
    if dev_fn is not None:
        code, d = device(0)
        assert code == 0 and (d == 2**64 - 1).all()
        assert device(4, stride=K - 1)[0] == _lib.GNS_E_ARG
        code, d = device(4, skew=4)  # answers not 8-byte aligned
        assert code == _lib.GNS_E_ARG and (d == 2**64 - 1).all()
    for x in owners:
        x.close()


def test_count_min_compact16_host_reuses_both_buffers(gpu, world):
    """Count-Min's 16-byte compact records from host memory in one call of four staged batches
    at the smallest batch the handle takes (one chunk; cm_insert's cold first batch is
    min(batch, max(64 chunks, batch / 32)) = the batch there): buffer 0, 1, 0, 1 with a ragged
    tail, the sizes unpacked into each staged batch.  The state is that of the same records
    inserted from device memory in two calls."""
    from go2netspectra_amd import CountMin, compact_headers
    w = world
    n = 3 * CHUNK + 777
    hdr = np.concatenate([w["hdr"], w["hdr"][:n - N]])
    wl = np.concatenate([w["wl"], w["wl"][:n - N]])
    rec, side = compact_headers(dev(hdr), dev(wl), rec_len=True)
    assert len(rec) == n and len(side) > 0
    hrec, hside = rec.cpu().numpy(), side.cpu().numpy()
    seeds = np.random.default_rng(3).integers(0, 2**32, 3, dtype=np.uint64).astype(np.uint32)
    a, b = (CountMin(1024, 3, 4000, 8, seeds=seeds, batch_packets=CHUNK, flow_fields=FIVE) for _ in range(2))
    a.insert_compact(hrec, None, hside)
    b.insert_compact(rec[:n // 3], None, side)
    b.insert_compact(rec[n // 3:], None, side)
    a.flush()
    b.flush()
    for name, x, y in zip(("C", "S", "FPc", "FPs"), a.export_state(), b.export_state()):
        assert np.array_equal(x, y), name
    c = same_counters(a, b, ["inserted", "dropped", "unsupported", "dict_full", "ovf_full"])
    assert c["inserted"] == n
