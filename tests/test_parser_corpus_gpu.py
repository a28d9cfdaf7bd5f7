"""The device record parser (parse_fast_ipv4 / parse_record / parse_l3, gns_device.cuh)
through every kernel it is inlined into, on the boundary corpus of
tests/parser_corpus.py plus 8,000 mutants, in the three orderings that exercise the
wave ballot of parse_record_fast and at the short lengths 1, 63, 64, 65, 257.

Every expected value comes from the C oracle (or_parse_hdr64_len and the sequential
engines built on it), never from another device path."""
import numpy as np
import pytest

import parser_corpus as pc
from helpers import assert_same_flows, owner_of_records

pytestmark = pytest.mark.gpu

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
PORTS = ["SrcPort", "DstPort", "Protocol"]
ORDERS = ["slow", "lane", "tail"]
SEEDS = np.array([0x9747B28C, 0x1B873593, 0xCC9E2D51, 0x85EBCA6B, 0xA1, 0xB2, 0xC3, 0xD4], np.uint32)


class Seq:
    """A record sequence and the oracle's parse of each record (gathered from one parse of
    the distinct records)."""

    def __init__(self, hdr, wl, idx, table):
        self.hdr, self.wl, self.idx = np.ascontiguousarray(hdr), np.ascontiguousarray(wl), idx
        self.p = {k: v[idx] for k, v in table.items()}
        st = self.p["status"]
        self.counts = tuple(int((st == s).sum()) for s in (0, 1, 2))

    def head(self, n):
        s = object.__new__(Seq)
        s.hdr, s.wl, s.idx = self.hdr[:n].copy(), self.wl[:n].copy(), self.idx[:n]
        s.p = {k: v[:n] for k, v in self.p.items()}
        s.counts = tuple(int((s.p["status"] == x).sum()) for x in (0, 1, 2))
        return s

    def keep(self, mask):
        s = object.__new__(Seq)
        s.hdr, s.wl, s.idx = self.hdr[mask].copy(), self.wl[mask].copy(), self.idx[mask]
        s.p = {k: v[mask] for k, v in self.p.items()}
        s.counts = tuple(int((s.p["status"] == x).sum()) for x in (0, 1, 2))
        return s

    def keys37(self):
        p = self.p
        return np.concatenate([p["src16"], p["dst16"], p["sport"].astype(">u2").view(np.uint8).reshape(-1, 2),
                               p["dport"].astype(">u2").view(np.uint8).reshape(-1, 2), p["proto"][:, None]], axis=1)


@pytest.fixture(scope="module")
def world(oracle):
    base = pc.corpus()
    recs = base + pc.mutants(8000, base=base)
    hdr, wl = pc.to_arrays(recs)
    fh, fw = pc.filler_pool()
    th, tw = np.concatenate([hdr, fh]), np.concatenate([wl, fw])  # the distinct records
    table = oracle.parse_hdr64_batch(th, tw)
    assert (table["status"][len(wl):] == 0).all()  # the filler is countable
    assert all((table["status"][:len(wl)] == s).any() for s in (0, 1, 2))
    assert any(n.startswith("preparsed/ver") for n, _, _ in base)  # the only observable of bytes 38/39
    seqs = {}
    for name, (oh, ow, origin) in pc.orderings(hdr, wl).items():
        idx = np.where(origin >= 0, origin, len(wl) + (-1 - origin))
        seqs[name] = Seq(oh, ow, idx, table)
    return {"seqs": seqs, "table_hdr": th, "table_wl": tw, "cache": {}}


def seq_of(world, order, length=None):
    s = world["seqs"][order]
    return s if length is None else s.head(length)


def dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def cached(world, key, make):
    if key not in world["cache"]:
        world["cache"][key] = make()
    return world["cache"][key]


def oracle_cm(oracle, world, order, length, fields, depth, width):
    def make():
        s = seq_of(world, order, length)
        K = 37 if fields is FIVE else 5
        orc = oracle.CountMin(width, depth, 1 << 16, 50, K, SEEDS[:depth])
        assert orc.insert_hdr64(s.hdr, s.wl, fields) == s.counts[0]
        return orc.export()
    return cached(world, ("cm", order, length, tuple(fields), depth, width), make)


def assert_cm(cm, want, counts, what):
    cm.flush()
    for name, a, b in zip(("C", "S", "FPc", "FPs"), cm.export_state(), want):
        assert np.array_equal(a, b), f"{what}: {name} differs from the oracle in {int((a != b).sum())} places"
    st = cm.stats()
    assert (st["inserted"], st["dropped"], st["unsupported"]) == counts, what


# --- compact records ---------------------------------------------------------
def check_compact(oracle, world, s, emb, what):
    from go2netspectra_amd import CountMin, compact_headers
    if emb:
        s = s.keep(s.wl <= 0xFFFF)
    n = len(s.wl)
    if n == 0:
        return
    rec, side = compact_headers(dev(s.hdr), dev(s.wl), rec_len=emb)
    rec, side = rec.cpu().numpy(), side.cpu().numpy()
    p = s.p
    narrow = ~p["src16"][:, 4:].any(axis=1) & ~p["dst16"][:, 4:].any(axis=1)
    v4 = (p["sver"] == 4) & (p["dver"] == 4) if emb else np.ones(n, bool)
    cls = np.where(p["status"] == 1, 1, np.where((p["status"] == 0) & narrow & v4, 0, 2))
    bad = np.nonzero(rec[:, 13] != cls)[0]
    assert len(bad) == 0, f"{what}: class of record {bad[:5]} is {rec[bad[:5], 13]}, want {cls[bad[:5]]}"
    t = cls == 0
    want = np.concatenate([p["src16"][:, :4], p["dst16"][:, :4], p["sport"].astype(">u2").view(np.uint8).reshape(-1, 2),
                           p["dport"].astype(">u2").view(np.uint8).reshape(-1, 2), p["proto"][:, None]], axis=1)
    bad = np.nonzero((rec[t, :13] != want[t]).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: tuple record {np.nonzero(t)[0][bad[:5]]} differs from the oracle's tuple"
    if emb:
        assert np.array_equal(rec[:, 14:16].copy().view("<u2").ravel(), s.wl.astype(np.uint16)), what
    else:
        assert np.array_equal(rec[t, 14], p["dver"][t]) and np.array_equal(rec[t, 15], p["sver"][t]), what
    assert not rec[cls == 1, :13].any(), what
    e = cls == 2
    slot = rec[e, :4].copy().view("<u4").ravel()
    assert len(side) == int(e.sum()) and sorted(slot.tolist()) == list(range(len(side))), what
    assert np.array_equal(side[slot], s.hdr[e]), f"{what}: a side slot does not hold its input record"
    # the compact stream is the same stream: Count-Min state and counters of the oracle
    orc = oracle.CountMin(4096, 4, 1 << 16, 50, 37, SEEDS[:4])
    assert orc.insert_hdr64(s.hdr, s.wl, FIVE) == s.counts[0]
    cm = CountMin(4096, 4, 1 << 16, 50, flow_fields=FIVE, seeds=SEEDS[:4])
    cm.insert_compact(rec, None if emb else s.wl, side)
    assert_cm(cm, orc.export(), s.counts, what + " insert_compact")
    cm.close()


@pytest.mark.parametrize("emb", [False, True], ids=["rec20", "rec16"])
@pytest.mark.parametrize("order", ORDERS)
def test_compact_headers(gpu, oracle, world, order, emb):
    check_compact(oracle, world, seq_of(world, order), emb, f"{order}")


@pytest.mark.parametrize("emb", [False, True], ids=["rec20", "rec16"])
def test_compact_headers_short(gpu, oracle, world, emb):
    for order in ORDERS:
        for n in pc.SHORT_LENGTHS:
            check_compact(oracle, world, seq_of(world, order, n), emb, f"{order}[:{n}]")
    # a thinned sequence: other records share a wave than in the full one
    s = world["seqs"]["slow"]
    check_compact(oracle, world, s.keep(np.arange(len(s.wl)) % 97 == 0), emb, "slow[::97]")


# --- Count-Min ---------------------------------------------------------------
@pytest.mark.parametrize("depth,width", [(4, 4096), (8, 4096), (3, 1000)])
@pytest.mark.parametrize("fields", [FIVE, PORTS], ids=["five", "ports"])
@pytest.mark.parametrize("order", ORDERS)
def test_countmin_insert_headers(gpu, oracle, world, order, fields, depth, width):
    from go2netspectra_amd import CountMin
    s = seq_of(world, order)
    want = oracle_cm(oracle, world, order, None, fields, depth, width)
    for batch in (0, 1000):
        cm = CountMin(width, depth, 1 << 16, 50, flow_fields=fields, seeds=SEEDS[:depth], batch_packets=batch)
        cm.insert_headers(s.hdr, s.wl)
        assert_cm(cm, want, s.counts, f"{order} batch_packets={batch}")
        cm.close()


@pytest.mark.parametrize("depth", [4, 3])
def test_countmin_insert_headers_short(gpu, oracle, world, depth):
    from go2netspectra_amd import CountMin
    for order in ORDERS:
        for n in pc.SHORT_LENGTHS:
            s = seq_of(world, order, n)
            want = oracle_cm(oracle, world, order, n, FIVE, depth, 4096)
            cm = CountMin(4096, depth, 1 << 16, 50, flow_fields=FIVE, seeds=SEEDS[:depth])
            cm.insert_headers(dev(s.hdr), dev(s.wl))
            assert_cm(cm, want, s.counts, f"{order}[:{n}]")
            cm.close()


# --- SuperSpread -------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["1", "0"])
@pytest.mark.parametrize("order", ORDERS)
def test_superspread_insert_headers(gpu, oracle, world, monkeypatch, order, pipe):
    from go2netspectra_amd import SuperSpread
    monkeypatch.setenv("GNS_SS_PIPE", pipe)
    ff, ef = ["SrcIP", "SrcPort"], ["DstIP", "DstPort", "Protocol"]
    s = seq_of(world, order)

    def make():
        orc = oracle.SuperSpread(1024, 2, 20, 128, 5, 0.5, 1.08, 18, 19, SEEDS[:2], 77, 99)
        assert orc.insert_hdr64(s.hdr, s.wl, ff, ef) == s.counts[0]
        return orc.export()
    want = cached(world, ("ss", order), make)
    ss = SuperSpread(1024, 2, 20, 128, 5, 0.5, 1.08, flow_fields=ff, elem_fields=ef, seeds=SEEDS[:2], hll_master=77,
                     rng_seed=99)
    ss.insert_headers(s.hdr, s.wl)
    ss.flush()
    for name, a, b in zip(("values", "keys", "regs", "pbits"), ss.export_state(), want):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), f"{name} differs"
    st = ss.stats()
    assert (st["inserted"], st["dropped"], st["unsupported"]) == s.counts
    ss.close()


# --- exact aggregator --------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_exact_flows(gpu, oracle, world, order):
    """Key text (the only observable of the IP version bytes 38/39), counts, bytes, first and
    last time of every flow."""
    import torch
    from go2netspectra_amd import ExactTask
    s = seq_of(world, order)
    ts = 1_700_000_000_000_000_000 + np.arange(len(s.wl), dtype=np.int64) * 1000
    # a tuple whose address is no 4- or 16-byte net.IP (version byte 0: nil IPs, odd Thrift
    # lengths) has no canonical key text: the aggregator counts it as unsupported (gns_exact.hip ex_key_tw)
    nokey = int(((s.p["status"] == 0) & ((s.p["sver"] == 0) | (s.p["dver"] == 0))).sum())
    assert nokey > 0
    oex = oracle.Exact(FIVE)
    assert oex.insert_hdr64(s.hdr, s.wl, ts) == s.counts[0] - nokey
    ex = ExactTask("t", FIVE)
    ex.agg.insert_headers(s.hdr, s.wl, ts)
    ex.flush()
    torch.cuda.synchronize()
    got = {f.Key: (f.StartTime, f.EndTime, f.PacketCount, f.ByteCount) for f in ex.flows()}
    assert_same_flows(got, oex.export())
    c = ex.agg.counters()
    assert (c["inserted"], c["dropped"], c["unsupported"]) == (s.counts[0] - nokey, s.counts[1], s.counts[2] + nokey)


# --- exact spread ------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_exact_spread_keys(gpu, world, order):
    from go2netspectra_amd import ExactSpread
    s = seq_of(world, order)
    ex = ExactSpread(FIVE, ["SrcIP"])
    ex.insert_headers(s.hdr, s.wl)
    ex.flush()
    f, v = ex.snapshot_arrays()
    got = {bytes(f[i]): int(v[i]) for i in range(len(v))}
    assert len(got) == len(v)
    want = {bytes(k): 1 for k in s.keys37()[s.p["status"] == 0]}
    assert_same_flows(got, want)
    c = ex.counters()
    assert (c["inserted"], c["dropped"], c["unsupported"]) == s.counts
    ex.close()


# --- router ------------------------------------------------------------------
@pytest.mark.parametrize("G", [3, 64])
def test_router_partition(gpu, oracle, world, G):
    from go2netspectra_amd.dist import Router
    owner_t = owner_of_records(oracle, world["table_hdr"], world["table_wl"], G)
    r = Router(G)
    for order in ORDERS:
        for n in (None,) + pc.SHORT_LENGTHS:
            s = seq_of(world, order, n)
            owner = owner_t[s.idx]
            oh, ow, counts = r.partition(dev(s.hdr), dev(s.wl))
            assert np.array_equal(counts, np.bincount(owner, minlength=G)), (order, n)
            o = np.argsort(owner, kind="stable")
            assert np.array_equal(oh.cpu().numpy(), s.hdr[o]), (order, n)
            assert np.array_equal(ow.cpu().numpy().view(np.uint32), s.wl[o]), (order, n)
