"""Spread roll-up on the GPU (gns_spread_rollup): the pair set of an ExactSpread derived from
the resident table of an ExactAggregator equals an ExactSpread of the same layouts fed the same
packets -- flows, spreads, heavy list, point queries and the exported pair set.

Truth shares no code with either engine: np.unique over the rows flow bytes ‖ element bytes
built by the host-side EncodeFlow encoder (PacketBatch.keys), cross-checked against a handle
fed directly on the device.

Streams: the tricky stream of exact_query_truth.py (IPv4, genuine IPv6, and 16-byte addresses
whose bytes equal an IPv4 slot: "aliases"), 60 000 packets over 5 000 five-tuples, with its
IPv4-mapped arrivals rewritten to the 4-byte form ("plain").  IPv4 sources are folded onto 256
values so that a source has many destinations and many flows; the aliases with an even first
byte are folded too, so that for those an alias flow and an IPv4 flow -- two flows of the
aggregator -- project onto one pair.  Device batches are 16K packets."""
import contextlib
import ctypes as ct

import numpy as np
import pytest

from exact_query_truth import FIVE, batch_of, tricky_stream
from helpers import assert_same_flows, assert_same_list

pytestmark = pytest.mark.gpu

N = 60_000
_CACHE = {}


def is_mapped(x):
    return (x[:, :10] == 0).all(1) & (x[:, 10:12] == 0xFF).all(1)


def plain_stream():
    """(t, ipver, ts) without IPv4-mapped arrivals; see the module docstring."""
    if "plain" not in _CACHE:
        t, ipver, ts = tricky_stream(23, N, 5000)
        for a in ("src16", "dst16"):
            x = t[a]
            m = is_mapped(x)
            x[m, 0:4] = x[m, 12:16]
            x[m, 4:] = 0
            ipver[m] = 4
        s = t["src16"]
        slot = (s[:, 4:] == 0).all(1)
        fold = slot & ((ipver == 4) | (s[:, 0] % 2 == 0))
        s[fold, 1:4] = 0
        assert not is_mapped(t["src16"]).any() and not is_mapped(t["dst16"]).any()
        assert ((ipver == 6) & slot).sum() > 1000  # the alias form is there
        _CACHE["plain"] = (t, ipver, ts)
    return _CACHE["plain"]


def mapped_stream():
    """The plain stream + 4 000 IPv4-mapped arrivals of its IPv4 packets; and the same after the
    mapped addresses are rewritten to the 4-byte form (copies of existing packets)."""
    if "mapped" not in _CACHE:
        t, ipver, ts = plain_stream()
        rng = np.random.default_rng(5)
        pick = rng.choice(np.flatnonzero(ipver == 4), 4000, replace=False)
        raw = {k: np.concatenate([v, v[pick]]) for k, v in t.items()}
        rewritten = {k: v.copy() for k, v in raw.items()}
        for a in ("src16", "dst16"):
            x = raw[a]
            x[N:, 12:16] = x[N:, 0:4]
            x[N:, 0:10] = 0
            x[N:, 10:12] = 0xFF
        iv = np.concatenate([ipver, np.full(len(pick), 6, np.uint8)])
        _CACHE["mapped"] = (raw, rewritten, iv, np.concatenate([ts, ts[pick]]))
    return _CACHE["mapped"]


def rows_set(f, e):
    rows = np.concatenate([np.asarray(f), np.asarray(e)], axis=1)
    out = set(map(bytes, rows))
    assert len(out) == len(rows), "a pair is listed twice"
    return out


def truth(t, ipver, ts, flow, elem, sel=slice(None)):
    """(flow bytes -> spread, set of pair bytes) of packets ``sel`` from their EncodeFlow bytes."""
    b = batch_of(t, ipver, ts, sel)
    fk, ek = b.keys(flow), b.keys(elem)
    rows = np.ascontiguousarray(np.concatenate([fk, ek], axis=1))
    pairs = np.unique(rows.view(np.dtype((np.void, rows.shape[1]))).ravel())
    pairs = pairs.view(np.uint8).reshape(len(pairs), -1)
    spread = {}
    for p in pairs:
        k = bytes(p[: fk.shape[1]])
        spread[k] = spread.get(k, 0) + 1
    return spread, set(map(bytes, pairs))


def to16_five(t, ipver, sel=slice(None)):
    """The aggregator's FIVE key of every packet of ``sel``, restated: IPs in To16 form."""
    b = batch_of(t, ipver, ts=np.zeros(len(ipver), np.int64), sel=sel)
    k = np.ascontiguousarray(b.keys(FIVE))
    v4 = np.asarray(ipver[sel]) == 4
    for off in (0, 16):
        a = k[v4, off:off + 4].copy()
        k[v4, off:off + 10] = 0
        k[v4, off + 10:off + 12] = 0xFF
        k[v4, off + 12:off + 16] = a
    return k


def distinct(rows):
    return set(map(bytes, rows))


def new_agg(fields, max_flows=1 << 12):
    from go2netspectra_amd import ExactAggregator
    return ExactAggregator(fields, max_flows=max_flows, batch_packets=16384)


def new_spread(flow, elem, **kw):
    from go2netspectra_amd import ExactSpread
    kw.setdefault("max_flows", 1 << 12)
    kw.setdefault("max_pairs", 1 << 13)
    kw.setdefault("batch_packets", 16384)
    return ExactSpread(flow, elem, **kw)


def feed(h, t, ipver, ts, sel=slice(None), pieces=3):
    idx = np.arange(len(ipver))[sel]
    for part in np.array_split(idx, pieces):
        h.insert_tuples(batch_of(t, ipver, ts, part))
    h.flush()


def snap(ex):
    f, v = ex.snapshot_arrays()
    d = {bytes(f[i]): int(v[i]) for i in range(len(v))}
    assert len(d) == len(v), "snapshot lists a flow twice"
    return d


def pair_set(ex):
    f, e, _ = ex.export_pairs()
    return rows_set(f, e)


def heavy(ex, thr):
    f, v = ex.heavy_hitters_arrays(thr)
    return [(bytes(f[i]), int(v[i])) for i in range(len(v))]


def same_arrays(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@contextlib.contextmanager
def untouched(src):
    """src is read only: snapshot arrays, counters, table statistics and position bit-equal."""
    view = src.view()
    before = (src.snapshot_arrays(), src.counters(), src.dict_stats(), view.refresh())
    yield
    after = (src.snapshot_arrays(), src.counters(), src.dict_stats(), view.refresh())
    view.close()
    assert same_arrays(before[0], after[0]) and before[1:] == after[1:], "the roll-up changed its source"


def assert_equal_handles(got, want, spread, pairs, what):
    """``got`` (rolled up) against ``want`` (fed directly) and the host truth: snapshot, heavy
    list at two thresholds, point queries, pair set."""
    assert_same_flows(snap(want), spread, f"{what}: the handle fed directly against the host truth")
    assert_same_flows(snap(got), spread, f"{what}: snapshot")
    top = max(spread.values())
    for thr in (2, max(3, top // 2)):
        exp = sorted(((k, v) for k, v in spread.items() if v >= thr), key=lambda r: (-r[1], r[0]))
        assert_same_list(heavy(want, thr), exp, f"{what}: heavy list of the handle fed directly, threshold {thr}")
        assert_same_list(heavy(got, thr), exp, f"{what}: heavy list, threshold {thr}")
    keys = np.array([list(k) for k in spread], np.uint8)
    absent = np.random.default_rng(1).integers(0, 256, (50, keys.shape[1]), dtype=np.uint8)
    probes = np.concatenate([keys, absent])
    exp = np.array([spread.get(bytes(k), 0) for k in probes], np.uint64)
    assert np.array_equal(want.query_many(probes), exp) and np.array_equal(got.query_many(probes), exp), what
    assert pair_set(want) == pairs and pair_set(got) == pairs, f"{what}: pair set"
    assert got.counters()["flows"] == len(spread) and got.dict_stats()["pairs_claimed"] == len(pairs)


@pytest.fixture(scope="module")
def five(gpu):
    """The plain stream in a FIVE-keyed aggregator, three inserts of several device batches each."""
    t, ipver, ts = plain_stream()
    src = new_agg(FIVE)
    feed(src, t, ipver, ts)
    n_flows = len(distinct(to16_five(t, ipver)))
    assert src.counters()["flows"] == n_flows
    src.n_flows = n_flows
    yield src
    src.close()


# --- 1. parity per layout -----------------------------------------------------
LAYOUTS = [(["SrcIP"], ["DstIP"]), (["DstIP"], ["SrcIP"]), (["SrcIP", "DstIP"], ["DstPort"]),
           (["SrcPort", "Protocol"], ["DstPort"]), (["SrcIP"], FIVE)]


# pieces of 512 slots: the table spans many, and more than 512 staged rows are reached again and
# again; the default piece (one piece, one merge) on a word-sized, a byte-sized and the widest layout
CASES = [(f, e, "512") for f, e in LAYOUTS] + [LAYOUTS[i] + (None,) for i in (0, 3, 4)]


@pytest.mark.parametrize("flow,elem,piece", CASES,
                         ids=["-".join(f) + "_" + "-".join(e) + ("_piece" + p if p else "") for f, e, p in CASES])
def test_rollup_equals_a_handle_fed_the_packets(five, monkeypatch, flow, elem, piece):
    if piece:
        monkeypatch.setenv("GNS_SPREAD_ROLLUP_PIECE", piece)
        assert five.dict_stats()["slots"] // int(piece) >= 16
    t, ipver, ts = plain_stream()
    spread, pairs = truth(t, ipver, ts, flow, elem)
    direct = new_spread(flow, elem)
    feed(direct, t, ipver, ts)
    got = new_spread(flow, elem)
    view = five.view()
    with untouched(five):
        cursor, projected, new = got.rollup_from(five)
    assert (projected, new) == (five.n_flows, len(pairs))
    assert cursor == view.refresh() == N
    view.close()
    assert_equal_handles(got, direct, spread, pairs, f"{flow} / {elem}")
    c = got.counters()
    assert (c["inserted"], c["records"], c["batches"], c["new_pairs"]) == (0, 0, 0, len(pairs))
    if elem == FIVE:
        # "flows per source": an alias flow and the IPv4 flow of the same bytes are two flows of the
        # aggregator and one pair here
        assert new < projected
        # ... so a source none of whose bytes arrive in a 16-byte address has exactly the
        # aggregator's flow count (Summary.flows of gns_ex_aggregate filtered on it)
        from go2netspectra_amd import make_filter
        s16 = t["src16"]
        in16 = distinct(s16[ipver == 6])
        v4 = sorted((k for k in distinct(s16[ipver == 4]) - in16 if any(k)), key=lambda k: (-spread[k], k))[:6]
        v6 = sorted(k for k in distinct(s16[(ipver == 6) & (s16[:, 4:] != 0).any(1)]))[:3]
        assert len(v4) == 6 and len(v6) == 3 and spread[v4[0]] > 10
        sums = five.aggregate([make_filter(src_ip=k[:4]) for k in v4] + [make_filter(src_ip=k) for k in v6])
        assert [s.flows for s in sums] == [spread[k] for k in v4 + v6]
        assert np.array_equal(got.query_many(np.array([list(k) for k in v4 + v6], np.uint8)),
                              np.array([s.flows for s in sums], np.uint64))
    # ExactAggregator.spread / ExactTask.spread: the same table in a handle of their own
    from go2netspectra_amd import ExactTask
    again = ExactTask("five", FIVE, agg=five).spread(flow, elem, max_flows=1 << 12, max_pairs=1 << 13)
    assert again.flow_fields == list(flow) and again.elem_fields == list(elem) and again.device == five.device
    assert_same_flows(snap(again), spread, "ExactTask.spread")
    for h in (again, got, direct):
        h.close()


def test_projection_is_timed_as_a_stage_of_its_own(five):
    got = new_spread(["SrcIP"], ["DstIP"])
    got.set_timing(True)
    got.rollup_from(five)
    st = got.stage_times()
    assert st["project"][1] >= 1 and st["project"][0] > 0.0 and st["insert"][1] >= 1
    got.close()


# --- 2. IPv4-mapped arrivals: the documented deviation ---------------------------
def test_mapped_arrivals_count_with_their_ipv4_address(gpu, monkeypatch):
    monkeypatch.setenv("GNS_SPREAD_ROLLUP_PIECE", "512")
    raw, rewritten, ipver, ts = mapped_stream()
    flow, elem = ["SrcIP"], ["DstIP"]
    src = new_agg(FIVE)
    feed(src, raw, ipver, ts)
    got = new_spread(flow, elem)
    got.rollup_from(src)
    spread, pairs = truth(rewritten, ipver, ts, flow, elem)
    assert (spread, pairs) == truth(*plain_stream(), flow, elem)  # the added packets are copies once rewritten
    direct = new_spread(flow, elem)
    feed(direct, rewritten, ipver, ts)
    assert_equal_handles(got, direct, spread, pairs, "mapped arrivals rewritten")
    fed_raw = new_spread(flow, elem)
    feed(fed_raw, raw, ipver, ts)
    raw_spread, _ = truth(raw, ipver, ts, flow, elem)
    assert_same_flows(snap(fed_raw), raw_spread, "fed the raw packets")
    assert len(spread) < len(raw_spread)  # a mapped source is a key of its own when fed directly
    assert any(is_mapped(np.frombuffer(k, np.uint8)[None, :])[0] for k in raw_spread)
    assert not any(is_mapped(np.frombuffer(k, np.uint8)[None, :])[0] for k in snap(got))
    for h in (src, got, direct, fed_raw):
        h.close()


# --- 3. delta -------------------------------------------------------------------
def test_delta_rollup_keeps_dst_equal_to_a_full_one(gpu, monkeypatch):
    from go2netspectra_amd import GnsError, _lib
    monkeypatch.setenv("GNS_SPREAD_ROLLUP_PIECE", "512")
    t, ipver, ts = plain_stream()
    flow, elem = ["SrcIP"], ["DstIP"]
    A, B = slice(0, 40_000), slice(40_000, N)
    src = new_agg(FIVE)
    view = src.view()
    got = new_spread(flow, elem)
    feed(src, t, ipver, ts, A)
    c1, p1, n1 = got.rollup_from(src)
    in_a = distinct(to16_five(t, ipver, A))
    assert c1 == view.refresh() == 40_000 and p1 == len(in_a)
    assert n1 == len(truth(t, ipver, ts, flow, elem, A)[1])
    feed(src, t, ipver, ts, B)
    with untouched(src):
        c2, p2, n2 = got.rollup_from(src, since=c1)
    new_flows = distinct(to16_five(t, ipver, B)) - in_a
    assert c2 == view.refresh() == N
    assert p2 == len(new_flows) and 0 < p2 < src.counters()["flows"]
    spread, pairs = truth(t, ipver, ts, flow, elem)
    assert n1 + n2 == len(pairs) and n2 <= p2
    direct = new_spread(flow, elem)
    feed(direct, t, ipver, ts)
    assert_equal_handles(got, direct, spread, pairs, "A, then the delta of B")
    # nothing is new after the last cursor; a cursor beyond the position is refused, dst as it was
    assert got.rollup_from(src, since=c2) == (c2, 0, 0)
    before = (snap(got), got.counters(), got.export_pairs()[2])
    with pytest.raises(GnsError) as e:
        got.rollup_from(src, since=c2 + 1)
    assert e.value.code == _lib.GNS_E_ARG and "beyond" in str(e.value)
    assert (snap(got), got.counters(), got.export_pairs()[2]) == before
    view.close()
    for h in (src, got, direct):
        h.close()


# --- 4. union into a handle that holds pairs ----------------------------------------
def test_union_into_a_non_empty_handle(five, monkeypatch):
    monkeypatch.setenv("GNS_SPREAD_ROLLUP_PIECE", "512")
    t, ipver, ts = plain_stream()
    flow, elem = ["SrcIP", "DstIP"], ["DstPort"]
    own = slice(0, 30_000)
    got = new_spread(flow, elem)
    feed(got, t, ipver, ts, own)
    _, held = truth(t, ipver, ts, flow, elem, own)
    spread, pairs = truth(t, ipver, ts, flow, elem)
    assert 0 < len(held) < len(pairs)
    cur = got.export_pairs()[2]
    c0 = got.counters()
    with untouched(five):
        _, projected, new = got.rollup_from(five)
    assert projected == five.n_flows and new == len(pairs) - len(held)
    c1 = got.counters()
    assert {k for k in c1 if c1[k] != c0[k]} == {"new_pairs", "flows"}
    assert c1["new_pairs"] - c0["new_pairs"] == new and c1["flows"] == len(spread)
    assert_same_flows(snap(got), spread, "own ingest, then the roll-up")
    assert pair_set(got) == pairs
    f, e, nxt = got.export_pairs(since=cur)
    assert rows_set(f, e) == pairs - held  # merged pairs are stamped as inserted at the merge
    # a second roll-up of the same table adds nothing: a union is idempotent
    assert got.rollup_from(five)[1:] == (five.n_flows, 0)
    assert len(got.export_pairs(since=nxt)[0]) == 0
    got.close()


# --- 5. growth inside the call ---------------------------------------------------------
def test_both_tables_grow_inside_the_call(five, monkeypatch):
    monkeypatch.setenv("GNS_SPREAD_ROLLUP_PIECE", "512")  # many merges: the tables also grow while they hold pairs
    t, ipver, ts = plain_stream()
    flow, elem = ["SrcIP"], FIVE
    got = new_spread(flow, elem, max_flows=64, max_pairs=256, batch_packets=5000)
    ds = got.dict_stats()
    assert (ds["flow_slots"], ds["pair_slots"], ds["flow_growths"], ds["pair_growths"]) == (128, 512, 0, 0)
    _, projected, new = got.rollup_from(five)
    spread, pairs = truth(t, ipver, ts, flow, elem)
    assert projected == five.n_flows and new == len(pairs)
    ds = got.dict_stats()
    assert ds["flow_growths"] >= 2 and ds["pair_growths"] >= 2, ds
    assert ds["flows_claimed"] == len(spread) and ds["pairs_claimed"] == len(pairs)
    assert_same_flows(snap(got), spread, "grown inside the call")
    assert pair_set(got) == pairs
    got.close()


# --- 6. sources that are themselves derived -----------------------------------------
def test_derived_sources(five, monkeypatch):
    monkeypatch.setenv("GNS_SPREAD_ROLLUP_PIECE", "512")
    t, ipver, ts = plain_stream()
    flow, elem = ["DstIP"], ["SrcIP", "Protocol"]
    spread, pairs = truth(t, ipver, ts, flow, elem)
    # the destination of gns_ex_rollup, keyed so that both IP fields lie at odd offsets
    mid = five.rollup(["Protocol", "SrcIP", "DstIP"], max_flows=1 << 12)
    got = new_spread(flow, elem)
    with untouched(mid):
        _, projected, new = got.rollup_from(mid)
    assert (projected, new) == (mid.counters()["flows"], len(pairs)) and projected <= five.n_flows
    assert_same_flows(snap(got), spread, "from a rolled-up aggregator")
    assert pair_set(got) == pairs
    got.close()
    mid.close()
    # a table filled by gns_ex_merge (a restore): every flow is a merged row
    merged = new_agg(FIVE)
    merged.merge(*five.snapshot_arrays())
    got = new_spread(flow, elem)
    cursor, projected, new = got.rollup_from(merged)
    assert (cursor, projected, new) == (five.n_flows, five.n_flows, len(pairs))
    assert_same_flows(snap(got), spread, "from a merged table")
    assert pair_set(got) == pairs
    # a cursor from before a reset selects every flow of the new period; dst keeps the old pairs
    period = slice(5_000, 9_000)
    merged.reset()
    feed(merged, t, ipver, ts, period)
    fresh = new_spread(flow, elem)
    c2, projected, new = fresh.rollup_from(merged, since=cursor)
    want, want_pairs = truth(t, ipver, ts, flow, elem, period)
    assert c2 == cursor + 4_000
    assert (projected, new) == (len(distinct(to16_five(t, ipver, period))), len(want_pairs))
    assert_same_flows(snap(fresh), want, "only the new period")
    assert got.rollup_from(merged, since=cursor)[1:] == (projected, 0)  # (they are pairs of the whole stream)
    assert_same_flows(snap(got), spread, "a union keeps the earlier period")
    for h in (merged, got, fresh):
        h.close()


# --- 7. errors and leaves -----------------------------------------------------------------
def test_errors_and_an_empty_source_leave_dst_untouched(five):
    from go2netspectra_amd import ExactSpread, GnsError, _lib
    t, ipver, ts = plain_stream()
    L = _lib.load()
    out = (ct.c_uint64 * 2)(3, 4)
    cur = ct.c_uint64(5)
    got = new_spread(["SrcIP"], ["DstIP"])
    feed(got, t, ipver, ts, slice(0, 5_000), pieces=1)
    state = lambda h: (snap(h), h.counters(), h.dict_stats(), h.export_pairs()[2])
    before = state(got)
    # a field the source's key lacks: the library's own check, then the Python mirror of it
    by_src = new_agg(["SrcIP", "SrcPort"])
    feed(by_src, t, ipver, ts, slice(0, 5_000), pieces=1)
    assert L.gns_spread_rollup(got._h, by_src._h, 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"DstIP" in L.gns_last_error() and b"element" in L.gns_last_error()
    with pytest.raises(ValueError, match="DstIP"):
        got.rollup_from(by_src)
    with pytest.raises(ValueError, match="DstPort"):
        by_src.spread(["SrcIP"], ["DstPort"])
    # a handle made from key sizes alone
    sizes_only = ExactSpread(None, None, flow_bytes=16, elem_bytes=16, max_flows=64, max_pairs=64)
    assert L.gns_spread_rollup(sizes_only._h, five._h, 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"field layouts" in L.gns_last_error()
    with pytest.raises(ValueError, match="field lists"):
        sizes_only.rollup_from(five)
    assert sizes_only.counters()["flows"] == 0
    with pytest.raises(TypeError):
        got.rollup_from(got)
    assert (out[0], out[1], cur.value) == (3, 4, 5)
    assert state(got) == before
    # an empty source moves nothing, in an empty handle and in one that holds pairs
    empty = new_agg(FIVE)
    fresh = new_spread(["SrcIP"], ["DstIP"])
    assert fresh.rollup_from(empty) == (0, 0, 0) and fresh.counters()["flows"] == 0
    assert got.rollup_from(empty) == (0, 0, 0)
    assert (snap(got), got.counters(), got.dict_stats()) == before[:3]
    # ... and the handle still takes a roll-up afterwards
    spread, pairs = truth(t, ipver, ts, ["SrcIP"], ["DstIP"])
    got.rollup_from(five)
    assert_same_flows(snap(got), spread, "after the refused calls")
    for h in (by_src, sizes_only, empty, fresh, got):
        h.close()
