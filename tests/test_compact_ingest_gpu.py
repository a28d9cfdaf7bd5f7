"""Compact records (IN_REC16) into SuperSpread, the exact spread engine and the exact
aggregator: an insert of the compact form -- 20-byte or 16-byte, from host arrays or
device tensors, through the pipelined or the generic S1 -- is the insert of the 64-byte
records it was made from.  State against the sequential oracle over the 64-byte records,
counters against a handle fed those records.

The stream is the one of test_host_staging_gpu.py::world (seed 20261019: 2 chunks + 777
packets over 3000 tuples, a fifth IPv6, a tenth of the frames behind a VLAN tag, 200
pooled sources), so every comparison holds side-record escapes, more than one batch and
a ragged tail."""
import numpy as np
import pytest

from helpers import assert_same_flows, assert_same_list, frame64, frames_from_tuples, pcapgen_records, random_tuples, \
    zipf_index

pytestmark = pytest.mark.gpu

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
CHUNK = 16384       # kSsChunk (gns_ss.hip), kXChunk (gns_exact.hip)
EXS_CHUNK = 4096    # kExsChunk (gns_spread.hip)
N = 2 * CHUNK + 777
N_EXS = 2 * EXS_CHUNK + 777
NFLOWS = 3000
SS_SEEDS = np.random.default_rng(4).integers(0, 2**32, 2, dtype=np.uint64).astype(np.uint32)
HM, RS = 0x1234ABCD5678EF01, 0x0DDBA11CAFEF00D5
SS_ARGS = (512, 2, 2, 32, 5, 0.5, 1.08)   # width, depth, threshold, m, size, base, b
FORMS = ["compact", "compact16"]


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(view.get(a.dtype, a.dtype))).to("cuda")


class Forms:
    """The 64-byte records of a stream and both compact forms of them, on the device (made by
    compact_headers) and copied to the host."""

    def __init__(self, hdr, wl, ts=None):
        from go2netspectra_amd import compact_headers
        self.hdr, self.wl, self.ts = hdr, np.ascontiguousarray(wl, np.uint32), ts
        self.d, self.h = {}, {}
        dh, dw = dev(hdr), dev(self.wl)
        for form in FORMS:
            rec, side = compact_headers(dh, dw, rec_len=form == "compact16")
            self.d[form] = (rec, side)
            self.h[form] = (rec.cpu().numpy(), side.cpu().numpy())
        assert len(self.h["compact"][1]) > 0 and len(self.h["compact16"][1]) > 0, "the stream must hold escapes"

    def insert(self, handle, form, placement, n=None, with_ts=False, side=True):
        """The first n records into the handle: placement 'host' in one call, 'device' in two
        calls split at n // 3.  Escapes index the side array of the whole stream."""
        n = len(self.wl) if n is None else n
        for lo, hi in ([(0, n)] if placement == "host" else [(0, n // 3), (n // 3, n)]):
            if placement == "host":
                rec, sd = self.h[form]
                wl = None if form == "compact16" else self.wl[lo:hi]
                ts = self.ts[lo:hi] if with_ts else None
            else:
                rec, sd = self.d[form]
                wl = None if form == "compact16" else dev(self.wl[lo:hi])
                ts = dev(self.ts[lo:hi]) if with_ts else None
            args = (rec[lo:hi], wl) + ((ts,) if with_ts else ()) + ((sd if side else None),)
            handle.insert_compact(*args)
        handle.flush()


@pytest.fixture(scope="module")
def world(gpu):
    rng = np.random.default_rng(20261019)
    t = random_tuples(rng, N, NFLOWS, v6_frac=0.2)
    pool4 = np.zeros((200, 16), np.uint8)
    pool4[:, :4] = rng.integers(0, 256, (200, 4))
    pool6 = rng.integers(0, 256, (200, 16), dtype=np.uint8)
    who = zipf_index(rng, N, 200, 0.8)
    t["src16"] = np.where(t["v6"][:, None], pool6[who], pool4[who])
    ts = np.cumsum(rng.integers(1, 1000, N)).astype(np.int64) + 1_700_000_000_000_000_000
    return Forms(frames_from_tuples(t, rng, vlan_frac=0.1), t["length"], ts)


def new_ss(**kw):
    from go2netspectra_amd import SuperSpread
    kw.setdefault("batch_packets", CHUNK)
    return SuperSpread(*SS_ARGS, flow_fields=["SrcIP"], elem_fields=["DstIP"], seeds=SS_SEEDS, hll_master=HM,
                       rng_seed=RS, **kw)


def ss_oracle(oracle, hdr, wl, args=SS_ARGS):
    orc = oracle.SuperSpread(*args, 16, 16, SS_SEEDS, HM, RS)
    done = orc.insert_hdr64(hdr, wl, ["SrcIP"], ["DstIP"])
    return orc.export(), orc.heavy(), done


def assert_ss_state(ss, want):
    for name, x, y in zip(("values", "keys", "regs", "pbits"), ss.export_state(), want):
        assert np.array_equal(x.view(np.uint64) if name == "pbits" else x, y.view(np.uint64) if name == "pbits" else y), name


def pick(c, names):
    return {k: c[k] for k in names}


# --- 1. SuperSpread -----------------------------------------------------------------
@pytest.fixture(scope="module")
def ss_ref(world, oracle):
    """The oracle over the 64-byte records, and the counters of a handle fed them."""
    state, heavy, done = ss_oracle(oracle, world.hdr, world.wl)
    h = new_ss()
    h.insert_headers(world.hdr, world.wl)
    h.flush()
    assert done == N and len(heavy) > 10
    return state, heavy, pick(h.counters(), ["inserted", "dropped", "unsupported", "records"])


@pytest.mark.parametrize("pipe", ["0", "1"])
@pytest.mark.parametrize("placement", ["host", "device"])
@pytest.mark.parametrize("form", FORMS)
def test_super_spread(world, ss_ref, monkeypatch, form, placement, pipe):
    monkeypatch.setenv("GNS_SS_PIPE", pipe)  # read when the handle is created
    state, heavy, counters = ss_ref
    ss = new_ss()
    world.insert(ss, form, placement)
    assert_ss_state(ss, state)
    assert_same_list([(h.Flow, h.Count) for h in ss.heavy_hitters().Count], heavy, "spread list")
    c = ss.counters()
    assert pick(c, counters) == counters and c["inserted"] == N and c["records"] == N


# --- 2. the S1 pipeline's prologue and tails ------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, CHUNK + 1])
def test_super_spread_pipeline_tails(world, oracle, monkeypatch, n):
    """One lane, one short of a block's stride, one past it, one record into a second block."""
    monkeypatch.setenv("GNS_SS_PIPE", "1")
    state, heavy, done = ss_oracle(oracle, world.hdr[:n], world.wl[:n])
    assert done == n and state[2].any()
    for form in FORMS:
        ss = new_ss()
        world.insert(ss, form, "host" if form == "compact" else "device", n=n)
        assert_ss_state(ss, state)
        assert ss.counters()["inserted"] == n
        assert_same_list([(h.Flow, h.Count) for h in ss.heavy_hitters().Count], heavy, "spread list")


# --- 3. the exact aggregator ------------------------------------------------------------
def new_exact_task(**kw):
    from go2netspectra_amd import ExactTask
    kw.setdefault("batch_packets", CHUNK)
    return ExactTask("per_five_tuple", FIVE, 16, **kw)


def task_flows(task):
    return {f.Key: (f.StartTime, f.EndTime, f.PacketCount, f.ByteCount) for f in task.flows()}


@pytest.fixture(scope="module")
def ex_ref(world, oracle):
    orc = oracle.Exact(FIVE)
    assert orc.insert_hdr64(world.hdr, world.wl, world.ts) == N
    want = orc.export()
    assert len(want) > 1000
    t = new_exact_task()
    t.agg.insert_headers(world.hdr, world.wl, world.ts)
    t.flush()
    heavy = [t.agg.heavy_hitters(metric, 0, 50) for metric in (0, 1)]
    assert all(len(v) == 50 for _, v in heavy)
    return want, heavy, pick(t.agg.counters(), ["inserted", "dropped", "unsupported", "dict_full", "flows", "records"])


@pytest.mark.parametrize("placement", ["host", "device"])
@pytest.mark.parametrize("form", FORMS)
def test_exact_aggregator(world, ex_ref, form, placement):
    want, heavy, counters = ex_ref
    t = new_exact_task()
    world.insert(t.agg, form, placement, with_ts=True)
    assert_same_flows(task_flows(t), want)
    for metric in (0, 1):
        k, v = t.agg.heavy_hitters(metric, 0, 50)
        assert np.array_equal(k, heavy[metric][0]) and np.array_equal(v, heavy[metric][1]), metric
    c = t.agg.counters()
    assert pick(c, counters) == counters and c["inserted"] == N


# --- 4. the exact spread engine -----------------------------------------------------------
def true_spreads(oracle, hdr, wl):
    """{flow: distinct elements} and the number of distinct (flow, element) pairs."""
    p = oracle.parse_hdr64_batch(hdr, wl)
    ok = p["status"] == 0
    pairs = {(bytes(s), bytes(d)) for s, d in zip(p["src16"][ok], p["dst16"][ok])}
    spread = {}
    for s, _ in pairs:
        spread[s] = spread.get(s, 0) + 1
    return spread, len(pairs), int(ok.sum())


@pytest.fixture(scope="module")
def exs_ref(world, oracle):
    return true_spreads(oracle, world.hdr[:N_EXS], world.wl[:N_EXS])


@pytest.mark.parametrize("placement", ["host", "device"])
@pytest.mark.parametrize("form", FORMS)
def test_exact_spread(world, exs_ref, form, placement):
    from go2netspectra_amd import ExactSpread
    spread, npairs, ok = exs_ref
    h = ExactSpread(["SrcIP"], ["DstIP"], batch_packets=EXS_CHUNK)
    world.insert(h, form, placement, n=N_EXS)
    got = {bytes(f): int(v) for f, v in zip(*h.snapshot_arrays())}
    assert len(spread) > 100 and ok == N_EXS
    assert_same_flows(got, spread)
    c = h.counters()
    assert c["inserted"] == N_EXS and c["records"] == N_EXS
    assert c["new_pairs"] == npairs and c["flows"] == len(spread)


# --- 5. record classes ------------------------------------------------------------------------
NCLS = 4096


@pytest.fixture(scope="module")
def classes(world):
    """4096 records of the stream with an ARP frame among them (class 1) and, per form, one
    tuple record rewritten by hand into an escape whose index is n_side; `hdr_edit` are the
    corresponding 64-byte records: that record carries IPv4 options there, which the device
    parser leaves unsupported."""
    hdr = world.hdr[:NCLS].copy()
    wl, ts = world.wl[:NCLS], world.ts[:NCLS]
    hdr[10, :] = 0
    hdr[10, 0:6], hdr[10, 12:14] = 0xFF, (0x08, 0x06)
    f = Forms(hdr, wl, ts)
    cls20 = f.h["compact"][0][:, 13]
    assert (cls20 == 1).sum() == 1 and (cls20 == 2).sum() > 0 and (cls20 == 0).sum() > 1000
    j = int(np.nonzero((cls20 == 0) & (hdr[:, 12] == 0x08) & (hdr[:, 13] == 0x00))[0][5])  # an untagged IPv4 tuple
    assert f.h["compact16"][0][j, 13] == 0
    for form in FORMS:
        rec, side = f.h[form]
        w = rec.view("<u4").reshape(-1, 4)
        w[j] = (len(side), 0, 0, (w[j, 3] & 0xFFFF0000 if form == "compact16" else 0) | 2 << 8)
        f.d[form] = (dev(rec), f.d[form][1])
    f.hdr_edit = hdr.copy()
    f.hdr_edit[j, 14] = 0x46
    f.escapes = {form: int((f.h[form][0][:, 13] == 2).sum()) for form in FORMS}
    f.tuples = {form: int((f.h[form][0][:, 13] == 0).sum()) for form in FORMS}
    return f


def engine(kind):
    from go2netspectra_amd import ExactSpread
    from go2netspectra_amd.exact import ExactAggregator
    if kind == "ss":
        return new_ss()
    if kind == "exs":
        return ExactSpread(["SrcIP"], ["DstIP"], batch_packets=EXS_CHUNK)
    return ExactAggregator(FIVE, batch_packets=CHUNK)


def engine_state(kind, h):
    if kind == "ss":
        v, k, r, p = h.export_state()
        return [v, k, r, p.view(np.uint64)]
    if kind == "exs":
        f, v = h.snapshot_arrays()
        o = np.lexsort(f.T[::-1])
        return [f[o], v[o]]
    keys, st, en, pk, by = h.snapshot_arrays()
    o = np.lexsort(keys.T[::-1])
    return [keys[o], st[o], en[o], pk[o], by[o]]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["ss", "exs", "ex"])
def test_record_classes(classes, kind, form):
    f = classes
    ref, got, bare = engine(kind), engine(kind), engine(kind)
    if kind == "ex":
        ref.insert_headers(f.hdr_edit, f.wl, f.ts)
    else:
        ref.insert_headers(f.hdr_edit, f.wl)
    ref.flush()
    placement = "host" if form == "compact" else "device"
    f.insert(got, form, placement, with_ts=kind == "ex")
    cr, cg = (pick(h.counters(), ["inserted", "dropped", "unsupported"]) for h in (ref, got))
    assert cr == cg
    assert cg["dropped"] == 1 and cg["unsupported"] >= 1 and cg["inserted"] > 1000
    assert sum(cg.values()) == NCLS
    for i, (x, y) in enumerate(zip(engine_state(kind, got), engine_state(kind, ref))):
        assert np.array_equal(x, y), (kind, form, i)
    # no side array: every escape is unsupported and none is read
    f.insert(bare, form, placement, with_ts=kind == "ex", side=False)
    cb = pick(bare.counters(), ["inserted", "dropped", "unsupported"])
    assert cb == {"inserted": f.tuples[form], "dropped": 1, "unsupported": f.escapes[form]}


# --- 6. dictionary recovery through compact input ----------------------------------------------
def new_sources(rng, n):
    """n records of new flows (uniform random IPv4 addresses), every 16th an IPv6 one: an escape."""
    hdr, wl = pcapgen_records(rng, n)
    for i in range(0, n, 16):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        hdr[i] = np.frombuffer(frame64(a[:16], a[16:], 1000 + i % 5000, 443, 6, int(wl[i]), v6=True), np.uint8)
    return hdr, np.ascontiguousarray(wl, np.uint32)


@pytest.mark.parametrize("form", FORMS)
def test_super_spread_compact_batch_reclaims_retries_and_splits(gpu, oracle, form):
    """The geometry of test_super_spread_host_batch_reclaims_retries_and_splits: two-chunk
    batches of new sources against a 4096-slot dictionary.  The halves of a split batch
    index the same, whole side array."""
    rng = np.random.default_rng(78)
    args = (256, 2, 20, 32, 5, 0.5, 1.08)
    from go2netspectra_amd import SuperSpread
    ss = SuperSpread(*args, flow_fields=["SrcIP"], elem_fields=["DstIP"], seeds=SS_SEEDS, hll_master=HM, rng_seed=RS,
                     max_flows=2048, batch_packets=2 * CHUNK)
    orc = oracle.SuperSpread(*args, 16, 16, SS_SEEDS, HM, RS)
    for call in range(2):
        hdr, wl = new_sources(rng, 2 * CHUNK)
        f = Forms(hdr, wl)
        f.insert(ss, form, "host" if call == 0 else "device")
        assert orc.insert_hdr64(hdr, wl, ["SrcIP"], ["DstIP"]) == 2 * CHUNK
    assert_ss_state(ss, orc.export())
    ds = ss.dict_stats()
    assert ds["retried_batches"] > 0 and ds["reclaims"] > 0, ds
    c = ss.counters()
    assert c["dict_full"] == 0 and c["inserted"] == 4 * CHUNK
    assert_same_list([(h.Flow, h.Count) for h in ss.heavy_hitters().Count], orc.heavy())


@pytest.mark.parametrize("form", FORMS)
def test_exact_aggregator_compact_batch_overflows_and_reruns(gpu, oracle, form):
    """A two-chunk compact batch of new flows overflows a 4096-slot table: the batch is undone,
    the table grows and the batch runs again over the same records and side array."""
    rng = np.random.default_rng(79)
    t = new_exact_task(max_flows=2048, batch_packets=2 * CHUNK)
    orc = oracle.Exact(FIVE)
    for call in range(2):
        hdr, wl = new_sources(rng, 2 * CHUNK)
        ts = np.cumsum(rng.integers(1, 1000, len(wl))).astype(np.int64) + call * (1 << 40)
        f = Forms(hdr, wl, ts)
        f.insert(t.agg, form, "host" if call == 0 else "device", with_ts=True)
        assert orc.insert_hdr64(hdr, wl, ts) == 2 * CHUNK
    assert_same_flows(task_flows(t), orc.export())
    assert t.agg.dict_stats()["retried_batches"] > 0
    c = t.agg.counters()
    assert c["dict_full"] == 0 and c["inserted"] == 4 * CHUNK and c["flows"] > 1000


# --- 7. the Manager ---------------------------------------------------------------------------------
CFG = """
aggregator:
  types: ["sketch", "exact"]
  sketch:
    tasks:
      - {name: cm5, skt_type: 0, flow_fields: [SrcIP, DstIP, SrcPort, DstPort, Protocol], width: 1024, depth: 3,
         size_thereshold: 4000, count_thereshold: 8}
      - {name: ss_src_dst, skt_type: 1, flow_fields: [SrcIP], element_fields: [DstIP], width: 512, depth: 2,
         count_thereshold: 2, m: 32, size: 5, b: 1.08, base: 0.5}
  exact:
    tasks:
      - {name: per_five_tuple, key_fields: [SrcIP, DstIP, SrcPort, DstPort, Protocol], num_shards: 16}
"""


def plain(snap):
    """A task's snapshot as plain comparable data."""
    if hasattr(snap, "Shards"):
        return {k: (f.StartTime, f.EndTime, f.PacketCount, f.ByteCount) for s in snap.Shards for k, f in s.Flows.items()}
    return ([(h.Flow, h.Count) for h in snap.Count], None if snap.Size is None else [(h.Flow, h.Size) for h in snap.Size])


@pytest.fixture(scope="module")
def mgr_ref(world):
    from go2netspectra_amd import HeaderBatch
    m = new_manager()
    m.process(HeaderBatch(world.hdr, world.wl, world.ts))
    snaps = {k: plain(v) for k, v in m.stop().items()}
    assert len(snaps) == 3 and len(snaps["per_five_tuple"]) > 1000
    assert len(snaps["cm5"][0]) > 10 and len(snaps["ss_src_dst"][0]) > 10
    return snaps


def new_manager():
    from go2netspectra_amd import Manager, parse_config
    m = Manager(parse_config(CFG), seeds=np.array([11, 22, 33], np.uint32), hll_master=HM, rng_seed=RS,
                batch_packets=CHUNK)
    m.start()
    return m


@pytest.mark.parametrize("form", FORMS)
def test_manager_host_compact_batch(world, mgr_ref, form):
    from go2netspectra_amd import CompactBatch
    rec, side = world.h[form]
    m = new_manager()
    m.process(CompactBatch(rec, None if form == "compact16" else world.wl, side, world.ts))
    got = {k: plain(v) for k, v in m.stop().items()}
    for name in mgr_ref:
        assert got[name] == mgr_ref[name], name


@pytest.mark.parametrize("form", FORMS)
def test_manager_device_header_batch_compacted(world, mgr_ref, form):
    from go2netspectra_amd import HeaderBatch
    cb = HeaderBatch(dev(world.hdr), dev(world.wl), dev(world.ts)).compact(rec_len=form == "compact16")
    assert cb.is_device() and len(cb) == N and len(cb.side) > 0 and (cb.wirelen is None) == (form == "compact16")
    m = new_manager()
    m.process(cb)
    got = {k: plain(v) for k, v in m.stop().items()}
    for name in mgr_ref:
        assert got[name] == mgr_ref[name], name
