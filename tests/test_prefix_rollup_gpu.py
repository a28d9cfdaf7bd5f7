"""Prefix roll-up, prefix spread roll-up, CIDR filters and hierarchical heavy hitters on the GPU.

A resident flow table re-keyed onto a layout with its IP fields masked to a prefix
(gns_ex_rollup_prefix) equals oracle.Exact keyed on that layout and fed the same packets with
their addresses masked on the host -- keys, StartTime, EndTime, packets and bytes, with
timestamps that are not monotonic.  The stream and the packet-side mask are prefix_truth.py's;
every parity case first asserts that its prefix forms groups (1 < groups < flows // 2, or one
group per address class at /0), so a vacuous case fails loudly.  Device batches are 16K
packets: every table is built from several."""
import ctypes as ct

import numpy as np
import pytest

from exact_query_truth import (FIVE, batch_of, got_heavy, key_bytes_of, oracle_export, truth_heavy, truth_rows)
from helpers import assert_same_flows, assert_same_list
from prefix_truth import N, classes_present, is_mapped, mask_packets, network_of, pair_of, prefix_stream

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
PSD = ["Protocol", "SrcIP", "DstIP"]  # the IP fields at odd offsets
FULL = {"SrcIP": (32, 128), "DstIP": (32, 128)}
_CACHE = {}


def truth(oracle, fields, prefix=None, sel=slice(None), nflows=5000):
    """oracle.Exact keyed on ``fields`` over packets ``sel`` with their addresses masked by
    ``prefix``, as key bytes -> (start, end, packets, bytes)."""
    key = (tuple(fields), repr(sorted((prefix or {}).items())), sel.start, sel.stop, nflows)
    if key not in _CACHE:
        t, ipver, ts = prefix_stream(nflows)
        exp = oracle_export(oracle, fields, mask_packets(t, ipver, prefix), ipver, ts, sel)
        _CACHE[key] = {key_bytes_of(k, fields): v for k, v in exp.items()}
    return _CACHE[key]


def new_agg(fields, max_flows=1 << 12):
    from go2netspectra_amd import ExactAggregator
    return ExactAggregator(fields, max_flows=max_flows, batch_packets=16384)


def feed(agg, sel=slice(None), nflows=5000, pieces=3, stream=None):
    t, ipver, ts = stream or prefix_stream(nflows)
    idx = np.arange(len(ipver))[sel]
    for part in np.array_split(idx, pieces):
        agg.insert_tuples(batch_of(t, ipver, ts, part))
    agg.flush()


def as_dict(arrays):
    from go2netspectra_amd import apply_delta
    return apply_delta({}, arrays)


def same_arrays(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def assert_groups(want, n_src, prefix, fields):
    """The case is not vacuous: the prefix forms groups."""
    t, ipver, _ = prefix_stream()
    zero = [f for f in fields if f in ("SrcIP", "DstIP") and pair_of((prefix or {}).get(f)) == (0, 0)]
    if fields == zero and len(zero) == 1:
        assert len(want) == classes_present(t["src16" if zero[0] == "SrcIP" else "dst16"], ipver) == 2
    else:
        assert 1 < len(want) < n_src // 2, (len(want), n_src)


@pytest.fixture(scope="module")
def five(gpu, oracle):
    """The whole stream in a FIVE-keyed handle, three inserts of several device batches each."""
    src = new_agg(FIVE)
    feed(src)
    assert_same_flows(as_dict(src.snapshot_arrays()), truth(oracle, FIVE), "the source table itself")
    yield src
    src.close()


@pytest.fixture(scope="module")
def psd(gpu, oracle):
    src = new_agg(PSD)
    feed(src)
    assert_same_flows(as_dict(src.snapshot_arrays()), truth(oracle, PSD), "the Protocol-SrcIP-DstIP table itself")
    yield src
    src.close()


# --- 1. parity with a task keyed on the layout and fed the masked packets ---
PARITY = [("five", ["SrcIP"], {"SrcIP": p}) for p in ((24, 48), (8, 16), (0, 0), (1, 1), (17, 65), (31, 127))] + [
    ("five", ["DstIP", "SrcIP", "SrcPort"], {"SrcIP": (16, 32), "DstIP": (25, 97)}),
    ("psd", ["SrcIP", "DstIP"], {"SrcIP": (20, 56), "DstIP": (20, 56)}),
    ("five", FIVE, {"SrcIP": (24, 64), "DstIP": (24, 64)}),
]


def case_id(c):
    return f"{c[0]}_to_{'-'.join(c[1])}_" + "_".join(f"{k}{v[0]}.{v[1]}" for k, v in sorted(c[2].items()))


@pytest.mark.parametrize("case", PARITY, ids=case_id)
def test_prefix_rollup_equals_a_task_fed_the_masked_packets(request, oracle, case):
    which, fields, prefix = case
    src = request.getfixturevalue(which)
    want = truth(oracle, fields, prefix)
    n_src = src.counters()["flows"]
    assert n_src == len(truth(oracle, FIVE if which == "five" else PSD))
    assert_groups(want, n_src, prefix, fields)
    dst = new_agg(fields)
    projected, new = dst.rollup_from(src, prefix=prefix)
    assert (projected, new) == (n_src, len(want))
    assert_same_flows(as_dict(dst.snapshot_arrays()), want, f"roll-up to {fields} under {prefix}")
    assert dst.counters()["flows"] == len(want)
    dst.close()
    # ExactAggregator.rollup(prefix=...): the same table in a handle of its own
    again = src.rollup(fields, prefix=prefix, max_flows=1 << 12)
    assert again.key_fields == list(fields)
    assert_same_flows(as_dict(again.snapshot_arrays()), want, f"rollup({fields}, prefix={prefix})")
    again.close()


def test_a_prefix_for_a_field_the_layout_lacks_is_ignored(five, oracle):
    dst = five.rollup(["SrcIP", "DstPort"], prefix={"SrcIP": (8, 16), "DstIP": (3, 3)}, max_flows=1 << 12)
    assert_same_flows(as_dict(dst.snapshot_arrays()), truth(oracle, ["SrcIP", "DstPort"], {"SrcIP": (8, 16)}), "DstIP prefix ignored")
    dst.close()
    ports = five.rollup(["DstPort", "Protocol"], prefix={"SrcIP": 0, "DstIP": 0}, max_flows=1 << 12)
    assert_same_flows(as_dict(ports.snapshot_arrays()), truth(oracle, ["DstPort", "Protocol"]), "ports are never masked")
    ports.close()


def test_start_and_end_follow_stream_order_not_min_max(oracle):
    """At (8, 16) some group's StartTime is not the smallest start of its parts (nor its EndTime
    the largest end): the property a host group-by with min / max cannot give."""
    prefix = {"SrcIP": (8, 16)}
    want, parts = truth(oracle, ["SrcIP"], prefix), truth(oracle, FIVE)
    lo, hi = {}, {}
    for k, (st, en, _, _) in parts.items():
        g = network_of(k[:16], 8, 16)
        lo[g] = min(lo.get(g, st), st)
        hi[g] = max(hi.get(g, en), en)
    assert set(lo) == set(want)
    assert any(want[k][0] != lo[k] for k in want) and any(want[k][1] != hi[k] for k in want)


# --- 2. full prefixes are gns_ex_rollup ---
class Spy:
    """The library with the names of the functions fetched from it recorded."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("which,fields", [("five", ["SrcIP"]), ("five", ["DstIP", "SrcIP", "SrcPort"]), ("psd", ["SrcIP", "DstIP"]),
                                          ("five", FIVE)], ids=lambda v: "-".join(v) if isinstance(v, list) else v)
def test_full_prefixes_equal_the_plain_rollup_bit_for_bit(request, which, fields):
    from go2netspectra_amd import _lib
    src = request.getfixturevalue(which)
    L = _lib.load()
    plain, masked = new_agg(fields), new_agg(fields)
    o1, o2 = (ct.c_uint64 * 2)(), (ct.c_uint64 * 2)()
    px = _lib.Prefix(32, 128, 32, 128)
    assert L.gns_ex_rollup(plain._h, src._h, o1) == 0
    assert L.gns_ex_rollup_prefix(masked._h, src._h, ct.byref(px), o2) == 0
    assert (o1[0], o1[1]) == (o2[0], o2[1]) and o1[0] == src.counters()["flows"]
    a, b = plain.snapshot_arrays(), masked.snapshot_arrays()
    assert len(a[3]) == len(b[3]) == o1[1]
    # (two tables claim their slots in parallel, so rows are compared by key, every array of them)
    assert as_dict(a) == as_dict(b)
    assert plain.counters() == masked.counters()
    va, vb = plain.view(), masked.view()
    assert va.refresh() == vb.refresh()  # the same positions were spent
    for h in (va, vb, plain, masked):
        h.close()


def test_rollup_without_prefix_takes_the_old_entry_point(five, monkeypatch):
    from go2netspectra_amd import _lib
    spy = Spy(_lib.load())
    monkeypatch.setattr(five, "_L", spy)
    monkeypatch.setattr(_lib, "_lib", spy)  # the handle rollup() creates loads it from here
    dst = five.rollup(["SrcIP"], max_flows=64)
    assert "gns_ex_rollup" in spy.calls and "gns_ex_rollup_prefix" not in spy.calls
    dst.close()
    spy.calls.clear()
    dst = five.rollup(["SrcIP"], prefix=FULL, max_flows=64)
    assert "gns_ex_rollup_prefix" in spy.calls and "gns_ex_rollup" not in spy.calls
    dst.close()


# --- 3. pieces and growth ---
NFL = 12_000


@pytest.fixture(scope="module")
def grown(gpu):
    """A five-tuple handle that grew under the 12 000-flow stream from 2^12 slots: many pieces of 256."""
    src = new_agg(FIVE, max_flows=2048)
    feed(src, nflows=NFL)
    assert src.dict_stats()["growths"] >= 1 and src.dict_stats()["slots"] // 256 >= 64
    yield src
    src.close()


@pytest.mark.parametrize("prefix", [{"SrcIP": (0, 0)}, {"SrcIP": (24, 48)}, FULL], ids=["slash0", "24.48", "full"])
def test_pieces_and_growth(grown, oracle, monkeypatch, prefix):
    nfl, src = NFL, grown
    monkeypatch.setenv("GNS_EX_ROLLUP_PIECE", "256")
    n_src = src.counters()["flows"]
    assert n_src == len(truth(oracle, FIVE, nflows=nfl))
    want = truth(oracle, ["SrcIP"], prefix, nflows=nfl)
    if prefix["SrcIP"] == (0, 0):
        assert len(want) == 2  # every piece feeds the same two groups
    elif prefix is not FULL:
        assert 100 < len(want) < n_src // 2  # many groups spread over many pieces
    dst = new_agg(["SrcIP"], max_flows=1)  # the smallest table
    assert dst.rollup_from(src, prefix=prefix) == (n_src, len(want))
    if len(want) > 100:
        assert dst.dict_stats()["growths"] >= 1
    assert_same_flows(as_dict(dst.snapshot_arrays()), want, f"{prefix} over many pieces")
    dst.close()


# --- 4. u64 wrap inside a group ---
def test_counts_that_wrap_inside_a_group(gpu):
    """Three merged rows of one /24 with 2^63, 2^63 and 5 packets: the first two sum to exactly
    0, the group's total does not, so the group is a flow with 5 packets, the bytes of all
    three, the start of the first row and the end of the last.  Two rows of another /24 summing
    to exactly 0: not a flow (a flow exists iff it has packets)."""
    from go2netspectra_amd.exact import ip_to16
    src = new_agg(["SrcIP", "SrcPort"], max_flows=64)
    rows = [("10.9.8.1", 1, 100, 200, 1 << 63, 7), ("10.9.8.77", 2, -50, 900, 1 << 63, M64 - 2), ("10.9.8.200", 3, 300, -7, 5, 11),
            ("10.9.9.1", 4, 1, 2, 1 << 63, 1), ("10.9.9.2", 5, 3, 4, 1 << 63, 2), ("2001:db8::1", 6, 5, 6, 9, 9)]
    keys = np.array([list(ip_to16(ip) + bytes([0, port])) for ip, port, *_ in rows], np.uint8)
    src.merge(keys, [r[2] for r in rows], [r[3] for r in rows], np.array([r[4] for r in rows], np.uint64),
              np.array([r[5] for r in rows], np.uint64))
    assert src.counters()["flows"] == 6
    dst = src.rollup(["SrcIP"], prefix={"SrcIP": (24, 64)}, max_flows=64)
    got = as_dict(dst.snapshot_arrays())
    assert got == {ip_to16("10.9.8.0"): (100, -7, 5, (7 + M64 - 2 + 11) & M64), ip_to16("2001:db8::"): (5, 6, 9, 9)}
    assert dst.counters()["flows"] == 2
    dst.close()
    src.close()


# --- 5. chain ---
def test_chained_prefixes_equal_direct_and_take_further_packets(five, oracle):
    levels = [(24, 64), (16, 48), (8, 32)]
    cur, made = five, []
    for lv in levels:
        cur = cur.rollup(["SrcIP"], prefix={"SrcIP": lv}, max_flows=64)
        made.append(cur)
        direct = five.rollup(["SrcIP"], prefix={"SrcIP": lv}, max_flows=64)
        want = truth(oracle, ["SrcIP"], {"SrcIP": lv})
        assert 1 < len(want) < five.counters()["flows"] // 2
        assert_same_flows(as_dict(direct.snapshot_arrays()), want, f"direct to {lv}")
        assert_same_flows(as_dict(cur.snapshot_arrays()), want, f"chained to {lv}")
        direct.close()
    # the /16 handle takes packets: the oracle fed the masked stream, then those packets as they are
    t, ipver, ts = prefix_stream()
    extra = slice(0, 9_000)
    mt = mask_packets(t, ipver, {"SrcIP": (16, 48)})
    both = {k: np.concatenate([mt[k], t[k][extra]]) for k in t}
    exp = oracle_export(oracle, ["SrcIP"], both, np.concatenate([ipver, ipver[extra]]), np.concatenate([ts, ts[extra]]))
    want = {key_bytes_of(k, ["SrcIP"]): v for k, v in exp.items()}
    assert len(want) > len(truth(oracle, ["SrcIP"], {"SrcIP": (16, 48)}))  # hosts joined the prefixes
    feed(made[1], extra)
    assert_same_flows(as_dict(made[1].snapshot_arrays()), want, "the /16 table, then packets")
    for h in made:
        h.close()


# --- 6. the result is a first-class handle ---
def test_result_is_a_first_class_handle(five, oracle, tmp_path):
    from go2netspectra_amd import ExactTask, checkpoint
    t, ipver, ts = prefix_stream()
    fields, prefix = ["SrcIP", "DstIP"], {"SrcIP": (16, 48), "DstIP": (16, 48)}
    task = ExactTask("five", FIVE, agg=five).rollup("nets", fields, 64, prefix=prefix, max_flows=1 << 12)
    assert isinstance(task, ExactTask) and task.key_fields == fields
    export = oracle_export(oracle, fields, mask_packets(t, ipver, prefix), ipver, ts)
    want = truth(oracle, fields, prefix)
    assert 1 < len(want) < five.counters()["flows"] // 2
    for metric in (0, 1):
        assert_same_list(got_heavy(*task.agg.heavy_hitters(metric, 0, 10)), truth_heavy(export, fields, metric, 0, 10),
                         f"top 10 by metric {metric}")
    rows = truth_rows(export, fields)
    nets = sorted({k[:16] for k in want})[:4]
    got = task.agg.aggregate([{}] + [dict(src_ip=n) for n in nets] + [dict(src_ip="203.0.113.0")])
    exp = [cidr_summary(rows, fields, {})] + [cidr_summary(rows, fields, {"SrcIP": (n, 128)}) for n in nets]
    assert got[:-1] == exp and got[-1].flows == 0 and exp[0].flows == len(want) and max(e.flows for e in exp[1:]) > 1
    assert {f.Key: (f.StartTime, f.EndTime, f.PacketCount, f.ByteCount) for f in task.flows()} == export
    view = task.view()
    view.refresh()
    assert same_arrays(view.snapshot_arrays(), task.agg.snapshot_arrays())
    assert view.aggregate([{}]) == [exp[0]]
    view.close()
    path = tmp_path / "nets.ckpt"
    task.save(path)
    back = ExactTask("back", fields, max_flows=64)
    back.restore(path)
    assert_same_flows(as_dict(back.agg.snapshot_arrays()), want, "checkpoint of a prefix table")
    checkpoint.save(back.agg, tmp_path / "again.ckpt")
    back.agg.close()
    task.agg.close()


# --- 7. spread ---
def new_spread(flow, elem, **kw):
    from go2netspectra_amd import ExactSpread
    kw.setdefault("max_flows", 1 << 12)
    kw.setdefault("max_pairs", 1 << 13)
    kw.setdefault("batch_packets", 16384)
    return ExactSpread(flow, elem, **kw)


def snap(ex):
    f, v = ex.snapshot_arrays()
    d = {bytes(f[i]): int(v[i]) for i in range(len(v))}
    assert len(d) == len(v), "snapshot lists a flow twice"
    return d


def pair_set(ex):
    f, e, _ = ex.export_pairs()
    rows = np.concatenate([np.asarray(f), np.asarray(e)], axis=1)
    out = set(map(bytes, rows))
    assert len(out) == len(rows), "a pair is listed twice"
    return out


def spread_truth(src_keys, src_fields, flow, elem, fpx, epx):
    """(flow bytes -> spread, pair set) of a source snapshot: distinct rows of the masked and
    converted flow bytes ‖ element bytes."""
    from go2netspectra_amd import mask_keys, rollup_plan, to16_to_encodeflow
    fk = to16_to_encodeflow(mask_keys(src_keys[:, rollup_plan(src_fields, flow)], flow, fpx), flow)
    ek = to16_to_encodeflow(mask_keys(src_keys[:, rollup_plan(src_fields, elem)], elem, epx), elem)
    pairs = set(map(bytes, np.concatenate([fk, ek], axis=1)))
    spread = {}
    for p in pairs:
        spread[p[:fk.shape[1]]] = spread.get(p[:fk.shape[1]], 0) + 1
    return spread, pairs


SPREADS = [
    ("hosts_per_24", ["SrcIP"], ["SrcIP"], {"SrcIP": (24, 48)}, None),
    ("nets_per_host", ["SrcIP"], ["DstIP"], None, {"DstIP": (24, 48)}),
    ("bytes_sized", ["SrcIP", "SrcPort"], ["Protocol"], {"SrcIP": (17, 65)}, None),       # 18 + 1 bytes: not word-sized
    ("ports_only", ["SrcPort"], ["Protocol"], {"SrcIP": (8, 8)}, {"DstIP": (8, 8)}),      # a 3-byte pair, nothing to mask
    ("widest", FIVE, FIVE, {"SrcIP": (24, 64), "DstIP": (24, 64)}, {"DstIP": (31, 127)}),  # 74 key bytes: a 20-word record
]


@pytest.fixture(scope="module")
def plain_five(gpu):
    """The stream without IPv4-mapped arrivals in a FIVE-keyed handle."""
    src = new_agg(FIVE)
    feed(src, stream=prefix_stream(mapped=False))
    yield src
    src.close()


@pytest.mark.parametrize("name,flow,elem,fpx,epx", SPREADS, ids=[s[0] for s in SPREADS])
def test_prefix_spread_rollup(five, plain_five, monkeypatch, name, flow, elem, fpx, epx):
    monkeypatch.setenv("GNS_SPREAD_ROLLUP_PIECE", "512")
    for src, mapped in ((five, True), (plain_five, False)):
        spread, pairs = spread_truth(src.snapshot_arrays()[0], FIVE, flow, elem, fpx, epx)
        n_src = src.counters()["flows"]
        if name not in ("ports_only",):
            assert 1 < len(spread) < n_src // 2 and max(spread.values()) > 1, (len(spread), n_src)
        got = new_spread(flow, elem)
        cursor, projected, new = got.rollup_from(src, flow_prefix=fpx, elem_prefix=epx)
        assert (cursor, projected, new) == (N, n_src, len(pairs))
        assert_same_flows(snap(got), spread, f"{name}: snapshot")
        assert pair_set(got) == pairs, f"{name}: pair set"
        if not mapped:  # an ExactSpread fed the masked packets (flow side and element side masked apart)
            t, ipver, ts = prefix_stream(mapped=False)
            fk = batch_of(mask_packets(t, ipver, fpx), ipver, ts).keys(flow)
            ek = batch_of(mask_packets(t, ipver, epx), ipver, ts).keys(elem)
            direct = new_spread(flow, elem)
            direct.insert_keys(fk, ek)
            direct.flush()
            assert_same_flows(snap(direct), spread, f"{name}: the handle fed the masked packets against the host truth")
            assert pair_set(direct) == pairs
            direct.close()
            again = src.spread(flow, elem, flow_prefix=fpx, elem_prefix=epx, max_flows=1 << 12, max_pairs=1 << 13)
            assert_same_flows(snap(again), spread, f"{name}: ExactAggregator.spread")
            again.close()
        got.close()


def test_prefix_spread_delta_chaining_equals_the_full_rollup(gpu, monkeypatch):
    monkeypatch.setenv("GNS_SPREAD_ROLLUP_PIECE", "512")
    flow, elem, fpx = ["SrcIP"], ["SrcIP"], {"SrcIP": (24, 48)}
    src = new_agg(FIVE)
    got = new_spread(flow, elem)
    feed(src, slice(0, 40_000))
    c1, p1, _ = got.rollup_from(src, flow_prefix=fpx)
    assert c1 == 40_000 and p1 == src.counters()["flows"]
    feed(src, slice(40_000, N))
    c2, p2, _ = got.rollup_from(src, since=c1, flow_prefix=fpx)
    assert c2 == N and 0 < p2 < src.counters()["flows"]
    full = new_spread(flow, elem)
    full.rollup_from(src, flow_prefix=fpx)
    spread, pairs = spread_truth(src.snapshot_arrays()[0], FIVE, flow, elem, fpx, None)
    assert_same_flows(snap(got), spread, "first part, then the delta")
    assert snap(full) == snap(got) and pair_set(full) == pair_set(got) == pairs
    assert got.rollup_from(src, since=c2, flow_prefix=fpx) == (c2, 0, 0)
    for h in (src, got, full):
        h.close()


# --- 8. CIDR filters ---
def cidr_summary(rows, fields, flt):
    """truth_summary restated with masks: ``flt`` = {field: value} with an IP value given as
    (address, bits of the 16-byte form); a row matches iff every field given is part of the key
    and equal -- an IP in its leading bits."""
    from go2netspectra_amd import Summary
    from go2netspectra_amd.exact import ip_to16
    if any(f not in fields for f in flt):
        return Summary()

    def top(ip, bits):
        return int.from_bytes(ip_to16(ip), "big") >> (128 - bits)

    def ok(parts):
        for f, v in flt.items():
            if f in ("SrcIP", "DstIP"):
                if top(parts[f], v[1]) != top(v[0], v[1]):
                    return False
            elif parts[f] != str(int(v)):
                return False
        return True
    hit = [r for r in rows if ok(r[0])]
    if not hit:
        return Summary()
    return Summary(len(hit), sum(r[3] for r in hit) & M64, sum(r[4] for r in hit) & M64, min(r[1] for r in hit),
                   max(r[2] for r in hit), max(r[3] for r in hit), max(r[4] for r in hit))


def cidr_filter(flt):
    from go2netspectra_amd import make_filter
    from go2netspectra_amd.exact import as_cidr
    arg = {"SrcIP": "src_ip", "DstIP": "dst_ip", "SrcPort": "src_port", "DstPort": "dst_port", "Protocol": "protocol"}
    plain = make_filter(**{arg[f]: (v[0] if f in ("SrcIP", "DstIP") else v) for f, v in flt.items()})
    return as_cidr(plain, flt.get("SrcIP", (0, 128))[1], flt.get("DstIP", (0, 128))[1])


def test_cidr_filters_on_handle_and_view(five, oracle):
    from go2netspectra_amd import _lib, make_filter
    t, ipver, ts = prefix_stream()
    rows = truth_rows(oracle_export(oracle, FIVE, t, ipver, ts), FIVE)
    s16 = t["src16"]
    four = bytes(s16[np.flatnonzero(ipver == 4)[0], :4])                                   # an IPv4 source, 4 bytes
    six = bytes(s16[np.flatnonzero((ipver == 6) & ~is_mapped(s16) & (s16[:, 4:] != 0).any(1))[0]])  # a genuine IPv6 source
    d4 = bytes(t["dst16"][np.flatnonzero(ipver == 4)[5], :4])
    flts = [{"SrcIP": (four, b)} for b in (0, 13, 96, 117, 120, 128)] + [{"SrcIP": (six, b)} for b in (0, 33, 64, 127)]
    flts += [{"DstIP": (d4, 120), "SrcIP": (four, 104)}, {"DstIP": (d4, 112), "DstPort": 53}, {"SrcIP": (six, 16), "Protocol": 6}]
    # low bits set in the filter's address are ignored
    noisy = bytes(four[:3]) + bytes([four[3] | 0x3F])
    flts.append({"SrcIP": (noisy, 120)})
    exp = [cidr_summary(rows, FIVE, f) for f in flts]
    assert exp[-1] == exp[4] and exp[-1].flows > 1
    assert exp[0].flows == exp[6].flows == len(rows)  # 0 bits: every flow whose key has the field
    assert exp[0].flows > exp[1].flows >= exp[2].flows > exp[3].flows >= exp[4].flows > exp[5].flows >= 1  # ... /0 of IPv4 ... the host
    assert exp[6].flows > exp[7].flows >= exp[8].flows >= exp[9].flows >= 1 and exp[7].flows > exp[9].flows
    got = five.aggregate([cidr_filter(f) for f in flts])
    assert got == exp
    view = five.view()
    view.refresh()
    assert view.aggregate([cidr_filter(f) for f in flts]) == exp
    # CIDR strings through make_filter, dicts through aggregate, a /24 string against the bits
    net = ".".join(str(b) for b in four[:3]) + ".0/24"
    assert five.aggregate([make_filter(src_ip=net), dict(src_ip=net)]) == [exp[4], exp[4]]
    # ... and through the task's querier calls: aggregate_flows[_many], trace_flow
    from go2netspectra_amd import ExactTask
    task = ExactTask("five", FIVE, agg=five)
    net6 = str(__import__("ipaddress").IPv6Address(six)) + "/33"
    e4, e6 = exp[4], exp[7]
    one = task.aggregate_flows(src_ip=net)
    assert (one.TaskName, one.FlowCount, one.TotalPackets, one.TotalBytes) == ("five", e4.flows, e4.packets, e4.bytes)
    many = task.aggregate_flows_many([dict(src_ip=net), dict(src_ip=net6), dict(src_ip=net, dst_port=53), {}])
    assert [(m.FlowCount, m.TotalPackets, m.TotalBytes) for m in many[:2]] == [(e.flows, e.packets, e.bytes) for e in (e4, e6)]
    with_port = cidr_summary(rows, FIVE, {"SrcIP": (four, 120), "DstPort": 53})
    assert 0 < with_port.flows < e4.flows and many[2].FlowCount == with_port.flows and many[3].FlowCount == len(rows)
    life = task.trace_flow({"SrcIP": net6})
    assert (life.FirstSeen, life.LastSeen, life.TotalPackets, life.TotalBytes) == (e6.first_ns, e6.last_ns, e6.max_packets, e6.max_bytes)
    life = task.trace_flow({"SrcIP": net, "DstPort": 53})
    assert (life.FirstSeen, life.LastSeen) == (with_port.first_ns, with_port.last_ns) and life.TotalPackets == with_port.max_packets
    task.agg = None  # (the fixture owns the handle)
    # a batch of 70 mixing both kinds: the wide path, two passes
    mixed, want = [], []
    for i in range(70):
        f = flts[i % len(flts)]
        if i % 3 == 0:  # equality filters, as the plain struct
            f = {k: ((v[0], 128) if k in ("SrcIP", "DstIP") else v) for k, v in f.items()}
            mixed.append(cidr_filter(f).f)
            assert isinstance(mixed[-1], _lib.ExFilter)
        else:
            mixed.append(cidr_filter(f))
        want.append(cidr_summary(rows, FIVE, f))
    assert five.aggregate(mixed) == want and view.aggregate(mixed) == want
    assert len({(s.flows, s.packets) for s in want}) > 8
    view.close()
    # a CIDR on a field outside the layout matches nothing; 0 bits on such a field too
    by_src = five.rollup(["SrcIP"], max_flows=1 << 12)
    src_rows = truth_rows(oracle_export(oracle, ["SrcIP"], t, ipver, ts), ["SrcIP"])
    probe = [{"DstIP": (d4, 120)}, {"DstIP": (d4, 0)}, {"SrcIP": (four, 120)}, {"SrcIP": (four, 120), "DstIP": (d4, 0)}]
    exp = [cidr_summary(src_rows, ["SrcIP"], f) for f in probe]
    assert [e.flows for e in exp[:2]] == [0, 0] and exp[2].flows > 1 and exp[3].flows == 0
    assert by_src.aggregate([cidr_filter(f) for f in probe]) == exp
    by_src.close()


# --- 9. hierarchical heavy hitters ---
def brute_hhh(leaves, levels, threshold):
    """From the per-address totals: level by level, finest first, a prefix's conditioned count is
    the sum of the addresses under it that lie under no prefix reported before."""
    reported, out = [], []  # reported: (level index, prefix bytes)
    for li, (v4, v6) in enumerate(levels):
        total, cond = {}, {}
        for ip, val in leaves.items():
            p = network_of(ip, v4, v6)
            total[p] = total.get(p, 0) + val
            if not any(network_of(ip, *levels[lj]) == q for lj, q in reported):
                cond[p] = cond.get(p, 0) + val
        rows = sorted(((p, total[p], cond.get(p, 0)) for p in total if cond.get(p, 0) >= threshold), key=lambda r: (-r[1], r[0]))
        out.append(rows)
        reported += [(li, p) for p, _, _ in rows]
    return out


@pytest.mark.parametrize("metric", [0, 1], ids=["packets", "bytes"])
def test_hierarchical_heavy_hitters(five, oracle, metric):
    from go2netspectra_amd import ExactTask
    levels = [(32, 128), (24, 64), (16, 48), (8, 32)]
    leaves = {k: v[3] if metric else v[2] for k, v in truth(oracle, ["SrcIP"]).items()}
    assert max(leaves.values()) < 1 << 63 and sum(leaves.values()) < 1 << 64
    threshold = sum(leaves.values()) // 40
    want = brute_hhh(leaves, levels, threshold)
    # a coarse prefix is reported, and some prefix heavy by its total is discounted away
    assert want[0] and any(want[li] for li in (1, 2, 3))
    heavy_by_total = 0
    for li, (v4, v6) in enumerate(levels[1:], 1):
        total = {}
        for ip, val in leaves.items():
            p = network_of(ip, v4, v6)
            total[p] = total.get(p, 0) + val
        heavy_by_total += sum(1 for p, tv in total.items() if tv >= threshold) - len(want[li])
    assert heavy_by_total >= 1
    got = five.hierarchical_heavy_hitters("SrcIP", levels, metric, threshold)
    assert got == want
    assert all(isinstance(v, int) for lv in got for row in lv for v in row[1:])
    assert ExactTask("five", FIVE, agg=five).hierarchical_heavy_hitters("SrcIP", levels, metric, threshold) == want
    with pytest.raises(ValueError):
        five.hierarchical_heavy_hitters("SrcPort", levels, metric, threshold)
    with pytest.raises(ValueError):
        five.hierarchical_heavy_hitters("SrcIP", levels[::-1], metric, threshold)
    with pytest.raises(ValueError):
        five.hierarchical_heavy_hitters("SrcIP", levels, metric, 0)


# --- 10. errors ---
def test_errors_leave_dst_untouched(gpu):
    from go2netspectra_amd import GnsError, _lib
    by_src, by_dst = new_agg(["SrcIP"]), new_agg(["DstIP"])
    feed(by_src, slice(0, 5_000), pieces=1)
    feed(by_dst, slice(0, 5_000), pieces=1)
    L = _lib.load()
    out = (ct.c_uint64 * 2)(3, 4)
    full = _lib.Prefix(32, 128, 32, 128)
    snap0, cnt0 = by_dst.snapshot_arrays(), by_dst.counters()
    # bits out of range, a null prefix
    for bad in ((33, 128, 32, 128), (32, 129, 32, 128), (32, 128, 33, 128), (32, 128, 32, 129)):
        px = _lib.Prefix(*bad)
        assert L.gns_ex_rollup_prefix(by_dst._h, by_src._h, ct.byref(px), out) == _lib.GNS_E_ARG
        assert b"prefix" in L.gns_last_error()
    assert L.gns_ex_rollup_prefix(by_dst._h, by_src._h, None, out) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()
    for bad in ({"SrcIP": 33}, {"SrcIP": (8, 129)}, {"Protocol": 3}):
        with pytest.raises(ValueError):
            by_dst.rollup_from(by_src, prefix=bad)
    # the GNS_E_ARG cases of the plain call: dst is src, a field the source lacks
    assert L.gns_ex_rollup_prefix(by_dst._h, by_dst._h, ct.byref(full), out) == _lib.GNS_E_ARG
    assert b"same handle" in L.gns_last_error()
    with pytest.raises(GnsError) as e:
        by_dst.rollup_from(by_dst, prefix={"DstIP": 8})
    assert e.value.code == _lib.GNS_E_ARG
    assert L.gns_ex_rollup_prefix(by_dst._h, by_src._h, ct.byref(full), out) == _lib.GNS_E_ARG
    assert b"DstIP" in L.gns_last_error()
    with pytest.raises(ValueError, match="DstIP"):
        by_dst.rollup_from(by_src, prefix={"DstIP": 8})
    with pytest.raises(ValueError, match="DstIP"):
        by_src.rollup(["DstIP"], prefix={"DstIP": 8})
    assert same_arrays(by_dst.snapshot_arrays(), snap0) and by_dst.counters() == cnt0
    assert (out[0], out[1]) == (3, 4)
    view = by_dst.view()
    assert view.refresh() == 5_000  # no positions were spent
    view.close()
    # the spread call, every case through the library itself against a handle that holds pairs:
    # prefixes out of range or null (either side), a cursor beyond the position, a field src's
    # key lacks, a dst created from key sizes alone
    from go2netspectra_amd import ExactSpread
    sp = new_spread(["SrcIP"], ["SrcIP"])
    sp.rollup_from(by_src, flow_prefix={"SrcIP": 24})
    state = lambda h: (snap(h), h.counters(), h.dict_stats(), pair_set(h))
    before = state(sp)
    assert before[1]["flows"] > 1
    bad = _lib.Prefix(40, 128, 32, 128)
    cur = ct.c_uint64(5)
    call = L.gns_spread_rollup_prefix
    assert call(sp._h, by_src._h, ct.byref(bad), ct.byref(full), 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"prefix" in L.gns_last_error()
    assert call(sp._h, by_src._h, ct.byref(full), ct.byref(_lib.Prefix(32, 128, 32, 129)), 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"prefix" in L.gns_last_error()
    assert call(sp._h, by_src._h, None, ct.byref(full), 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()
    assert call(sp._h, by_src._h, ct.byref(full), None, 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()
    assert call(sp._h, by_src._h, ct.byref(full), ct.byref(full), 5_001, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"since" in L.gns_last_error()
    with pytest.raises(GnsError):
        sp.rollup_from(by_src, since=5_001, flow_prefix={"SrcIP": 24})
    # a field the source's key lacks: the library's own check on each side, then the Python mirror of it
    to_dst = new_spread(["SrcIP"], ["DstIP"])
    from_dst = new_spread(["DstIP"], ["SrcIP"])
    px24 = _lib.Prefix(24, 64, 24, 64)
    assert call(to_dst._h, by_src._h, ct.byref(px24), ct.byref(px24), 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"DstIP" in L.gns_last_error() and b"element" in L.gns_last_error()
    assert call(from_dst._h, by_src._h, ct.byref(px24), ct.byref(px24), 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"DstIP" in L.gns_last_error() and b"flow" in L.gns_last_error()
    assert to_dst.counters()["flows"] == from_dst.counters()["flows"] == 0
    with pytest.raises(ValueError, match="DstIP"):
        to_dst.rollup_from(by_src, elem_prefix={"DstIP": 24})
    with pytest.raises(ValueError, match="DstIP"):
        by_src.spread(["DstIP"], ["SrcIP"], flow_prefix={"DstIP": 24})
    # a handle made from key sizes alone
    sizes_only = ExactSpread(None, None, flow_bytes=16, elem_bytes=16, max_flows=64, max_pairs=64)
    assert call(sizes_only._h, by_src._h, ct.byref(px24), ct.byref(full), 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"field layouts" in L.gns_last_error()
    with pytest.raises(ValueError, match="field lists"):
        sizes_only.rollup_from(by_src, flow_prefix={"SrcIP": 24})
    assert sizes_only.counters()["flows"] == 0
    assert state(sp) == before and (out[0], out[1], cur.value) == (3, 4, 5)
    # ... and the handle still takes a roll-up afterwards
    assert sp.rollup_from(by_src, flow_prefix={"SrcIP": 24})[2] == 0 and state(sp)[0] == before[0]
    for h in (to_dst, from_dst, sizes_only):
        h.close()
    # an empty source moves nothing
    empty, dst = new_agg(FIVE), new_agg(["DstIP"])
    assert dst.rollup_from(empty, prefix={"DstIP": 8}) == (0, 0) and dst.counters()["flows"] == 0
    for h in (by_src, by_dst, sp, empty, dst):
        h.close()
