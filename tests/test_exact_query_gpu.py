"""The exact engine's query plane on the GPU (gns_ex_aggregate / gns_ex_heavy_hitters and
the Querier shapes of ExactTask) against the ClickHouse comparison restated on the oracle's
export (exact_query_truth.py): filtered aggregates, flow trace, ordered heavy hitters."""
import ctypes as ct
import ipaddress

import numpy as np
import pytest

from exact_query_truth import (FIVE, batch_of, got_heavy, oracle_export, packet_value, to_filter, tricky_stream,
                               truth_heavy, truth_rows, truth_summary)
from helpers import assert_same_list

pytestmark = pytest.mark.gpu

LAYOUTS = [FIVE, ["SrcIP"], ["Protocol", "SrcIP"], ["SrcPort", "Protocol", "DstIP", "DstPort"]]
N, NFLOWS = 60_000, 2500
_STREAM = {}


def stream():
    if "s" not in _STREAM:
        _STREAM["s"] = tricky_stream(7, N, NFLOWS)
    return _STREAM["s"]


def respell(value, how: int):
    """Another spelling of the same IP (4 / 16 net.IP bytes in)."""
    value = bytes(value)
    if len(value) == 4:
        dotted = str(ipaddress.IPv4Address(value))
        return [dotted, "::ffff:" + dotted, "0:0:0:0:0:FFFF:" + dotted][how % 3]
    a = ipaddress.IPv6Address(value)
    if a.ipv4_mapped is not None:  # arrived mapped: ask through the dotted quad
        return [str(a.ipv4_mapped), value][how % 2]
    return [a.compressed, a.exploded, a.exploded.upper()][how % 3]


def filter_set(fields, t, ipver, rng, n_each=6):
    """Filters drawn from the stream: none, one field (present or absent in the key), every
    key field (one flow of a five-tuple key), near misses, IPs in other spellings."""
    out = [{}]
    pick = rng.integers(0, len(ipver), n_each)
    for f in FIVE:  # single-field filters, also on fields the key does not have
        for j, i in enumerate(pick):
            v = packet_value(t, ipver, i, f)
            out.append({f: respell(v, j) if f.endswith("IP") else v})
    for j, i in enumerate(rng.integers(0, len(ipver), 3 * n_each)):  # all key fields: that packet's flow
        flt = {f: packet_value(t, ipver, i, f) for f in fields}
        out.append({f: respell(v, j) if f.endswith("IP") else v for f, v in flt.items()})
        miss = dict(flt)  # one field off: matches another flow or none
        g = fields[j % len(fields)]
        if g.endswith("IP"):
            b = bytearray(miss[g])
            b[-1] ^= 0x55
            miss[g] = bytes(b)
        else:
            miss[g] = (miss[g] + 1) % (256 if g == "Protocol" else 65536)
        out.append(miss)
    out.append({f: packet_value(t, ipver, int(pick[0]), f) for f in FIVE})  # all five, whatever the key
    out.append({"Protocol": 6})
    out.append({"Protocol": 200})  # not in the stream
    return out


@pytest.fixture(scope="module", params=LAYOUTS, ids=lambda f: "-".join(f))
def loaded(request, gpu, oracle):
    from go2netspectra_amd import ExactTask
    fields = request.param
    t, ipver, ts = stream()
    task = ExactTask("q", fields, batch_packets=16384, max_flows=1 << 12)
    task.process_packets(batch_of(t, ipver, ts))
    task.flush()
    want = oracle_export(oracle, fields, t, ipver, ts)
    yield task, fields, want
    task.agg.close()


def check_filters(task, fields, want, filters):
    rows = truth_rows(want, fields)
    got = task.agg.aggregate([to_filter(f) for f in filters])
    exp = [truth_summary(rows, fields, f) for f in filters]
    for f, g, e in zip(filters, got, exp):
        assert g == e, f"{fields} filter {f}: got {g} want {e}"
    return exp


def test_filters_equal_the_clickhouse_comparison(loaded):
    task, fields, want = loaded
    t, ipver, ts = stream()
    filters = filter_set(fields, t, ipver, np.random.default_rng(len(fields)))
    exp = check_filters(task, fields, want, filters)
    counts = [e.flows for e in exp]
    assert exp[0].flows == len(want)  # mask == 0: the totals
    assert 0 in counts and 1 in counts  # filters that match no flow, one flow ...
    if len(fields) > 1:  # ... and many (a one-field key has one flow per value)
        assert max(counts[1:]) > 1
    absent = [f for f in FIVE if f not in fields]
    for f in absent:  # a field outside the key is a NULL column
        assert task.agg.aggregate([to_filter({f: packet_value(t, ipver, 0, f)})])[0].flows == 0


def test_wide_sums_and_signed_times(loaded):
    task, fields, want = loaded
    tot = task.agg.aggregate([to_filter({})])[0]
    assert tot == truth_summary(truth_rows(want, fields), fields, {})
    assert tot.bytes > 1 << 33 and tot.max_bytes > 1 << 32 and tot.first_ns < 0 < tot.last_ns


@pytest.mark.parametrize("nf", [1, 2, 63, 64, 65, 200])
def test_batch_equals_one_by_one(loaded, nf):
    task, fields, want = loaded
    t, ipver, ts = stream()
    pool = _STREAM.setdefault(("pool", tuple(fields)), filter_set(fields, t, ipver, np.random.default_rng(99), n_each=12))
    filters = [pool[(3 * i) % len(pool)] for i in range(nf)]
    singles = _STREAM.setdefault(("singles", tuple(fields)), {})
    for i in {(3 * i) % len(pool) for i in range(nf)}:
        if i not in singles:
            singles[i] = task.agg.aggregate([to_filter(pool[i])])[0]
    got = task.agg.aggregate([to_filter(f) for f in filters])
    assert got == [singles[(3 * i) % len(pool)] for i in range(nf)]
    rows = truth_rows(want, fields)
    assert got[-1] == truth_summary(rows, fields, filters[-1])


def probe_filters(fields, t, ipver, idx):
    out = [{}]
    for i in idx:
        out += [{f: packet_value(t, ipver, i, f)} for f in fields]
        out.append({f: packet_value(t, ipver, i, f) for f in fields})
    return out


def check_all(task, fields, want, t, ipver, idx):
    check_filters(task, fields, want, probe_filters(fields, t, ipver, idx))
    for metric in (0, 1):
        assert_same_list(got_heavy(*task.agg.heavy_hitters(metric)), truth_heavy(want, fields, metric), "all flows")
        assert_same_list(got_heavy(*task.agg.heavy_hitters(metric, 0, 10)), truth_heavy(want, fields, metric, 0, 10),
                         "top 10")


def test_empty_one_packet_reset_and_refill(gpu, oracle):
    from go2netspectra_amd import ExactTask, Summary
    t, ipver, ts = stream()
    task = ExactTask("s", FIVE, max_flows=1 << 12)
    probes = probe_filters(FIVE, t, ipver, [0, 1])
    assert task.agg.aggregate([to_filter(f) for f in probes]) == [Summary()] * len(probes)
    for metric in (0, 1):
        keys, vals = task.agg.heavy_hitters(metric, 0, 5)
        assert len(keys) == 0 and len(vals) == 0
    task.process_packets(batch_of(t, ipver, ts, slice(0, 1)))
    check_all(task, FIVE, oracle_export(oracle, FIVE, t, ipver, ts, slice(0, 1)), t, ipver, [0, 1])
    task.process_packets(batch_of(t, ipver, ts, slice(1, 30_000)))
    check_all(task, FIVE, oracle_export(oracle, FIVE, t, ipver, ts, slice(0, 30_000)), t, ipver, [0, 5, 29_999, 40_000])
    task.reset()
    assert task.agg.aggregate([to_filter({})]) == [Summary()]
    sel = slice(50_000, 52_000)  # a smaller refill: nothing of the first period may be seen
    task.process_packets(batch_of(t, ipver, ts, sel))
    check_all(task, FIVE, oracle_export(oracle, FIVE, t, ipver, ts, sel), t, ipver, [0, 50_000, 51_999])


@pytest.mark.parametrize("touched_list", [False, True])
def test_grown_table_between_batches(gpu, oracle, monkeypatch, touched_list):
    """A table of 32 flows grows several times under the stream; queries between the calls of
    a multi-batch insert (16K-packet device batches) see exactly the packets inserted so far,
    also when T / D run over the touched-flow list."""
    from go2netspectra_amd import ExactTask
    if touched_list:
        monkeypatch.setenv("GNS_EX_LIST", "1")
    t, ipver, ts = stream()
    fields = ["SrcPort", "Protocol", "DstIP", "DstPort"]
    task = ExactTask("g", fields, max_flows=32, batch_packets=16384)
    for end in (20_000, 60_000):
        start = 0 if end == 20_000 else 20_000
        task.process_packets(batch_of(t, ipver, ts, slice(start, end)))
        check_all(task, fields, oracle_export(oracle, fields, t, ipver, ts, slice(0, end)), t, ipver, [3, end - 1])
    assert task.agg.dict_stats()["growths"] >= 2


def tie_stream(rng):
    """400 five-tuple flows: 50 heavy ones with distinct counts, then 50 / 150 / 150 flows with
    exactly 9 / 5 / 1 packets; lengths near 2^32 on the 9-packet flows, so their byte counts
    pass 2^32 and order differently by their low 32 bits."""
    nfl = 400
    src, dst = np.zeros((nfl, 16), np.uint8), np.zeros((nfl, 16), np.uint8)
    src[:, :4] = rng.integers(0, 256, (nfl, 4))
    dst[:, :4] = rng.integers(0, 256, (nfl, 4))
    sport = np.arange(nfl).astype(np.uint16)  # distinct flows whatever the addresses
    counts = np.concatenate([100 + 3 * np.arange(50), np.full(50, 9), np.full(150, 5), np.full(150, 1)])
    idx = rng.permutation(np.repeat(np.arange(nfl), counts))
    n = len(idx)
    length = rng.integers(64, 1500, n).astype(np.uint32)
    nine = (idx >= 50) & (idx < 100)
    length[nine] = rng.integers(1 << 31, 1 << 32, int(nine.sum()), dtype=np.uint64).astype(np.uint32)
    tt = dict(src16=src[idx], dst16=dst[idx], sport=sport[idx], dport=np.full(n, 443, np.uint16),
              proto=np.full(n, 6, np.uint8), length=length)
    return tt, np.full(n, 4, np.uint8), rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)


def test_heavy_hitters_order_ties_and_cuts(gpu, oracle):
    from go2netspectra_amd import ExactTask
    t, ipver, ts = tie_stream(np.random.default_rng(5))
    task = ExactTask("hh", FIVE, max_flows=1 << 10)
    task.process_packets(batch_of(t, ipver, ts))
    want = oracle_export(oracle, FIVE, t, ipver, ts)
    assert len(want) == 400
    full = [truth_heavy(want, FIVE, m) for m in (0, 1)]
    by = [v for _, v in full[1]]
    assert any(a > b > 1 << 32 and (a & 0xFFFFFFFF) < (b & 0xFFFFFFFF) for a, b in zip(by, by[1:]))
    for metric in (0, 1):
        top = full[metric][0][1]
        some = full[metric][120][1]
        for thr in (top + 1, top, some, 1, 0):  # 0, 1, some and all flows
            exp = truth_heavy(want, FIVE, metric, thr)
            assert_same_list(got_heavy(*task.agg.heavy_hitters(metric, thr)), exp, f"metric {metric} thr {thr}")
        assert len(truth_heavy(want, FIVE, metric, top + 1)) == 0 and len(truth_heavy(want, FIVE, metric, top)) == 1
        # limits below, inside a run of equal values (75: the 9-packet flows; 180: the 5-packet
        # ones), at and above the list length
        for limit in (1, 49, 50, 75, 180, 399, 400, 401, 100_000):
            exp = truth_heavy(want, FIVE, metric, 0, limit)
            assert_same_list(got_heavy(*task.agg.heavy_hitters(metric, 0, limit)), exp, f"metric {metric} limit {limit}")
        assert_same_list(got_heavy(*task.agg.heavy_hitters(metric, some, 60)), truth_heavy(want, FIVE, metric, some, 60),
                         "threshold and limit")
    assert full[0][74][1] == full[0][75][1] == 9  # the cut at 75 falls between equal counts
    # a capacity smaller than the list: the length is reported, nothing is written
    L = task.agg._L
    keys, vals = np.full((399, 37), 0xAB, np.uint8), np.full(399, 0xABAB, np.uint64)
    n = ct.c_uint64(399)
    assert L.gns_ex_heavy_hitters(task.agg._h, 0, 0, 0, keys.ctypes.data, vals.ctypes.data, ct.byref(n)) == 0
    assert n.value == 400 and (keys == 0xAB).all() and (vals == 0xABAB).all()
    n = ct.c_uint64(399)
    assert L.gns_ex_heavy_hitters(task.agg._h, 1, 0, 399, keys.ctypes.data, vals.ctypes.data, ct.byref(n)) == 0
    assert n.value == 399 and got_heavy(keys, vals) == full[1][:399]


def test_c_abi_argument_errors(gpu):
    from go2netspectra_amd import ExactTask, _lib, make_filter
    task = ExactTask("e", ["SrcIP"], max_flows=64)
    L = task.agg._L
    f = (_lib.ExFilter * 1)(make_filter(protocol=6))
    out = (_lib.ExSummary * 1)()
    assert L.gns_ex_aggregate(task.agg._h, f, 0, out) == 0  # nf == 0: a no-op
    assert L.gns_ex_aggregate(task.agg._h, None, 0, None) == 0
    assert L.gns_ex_aggregate(task.agg._h, None, 1, out) == _lib.GNS_E_ARG
    assert L.gns_ex_aggregate(task.agg._h, f, 1, None) == _lib.GNS_E_ARG
    assert L.gns_ex_aggregate(None, f, 1, out) == _lib.GNS_E_ARG
    f[0].mask = 1 << 6
    assert L.gns_ex_aggregate(task.agg._h, f, 1, out) == _lib.GNS_E_ARG
    f[0].mask = 1  # GNS_F_NONE is not a field
    assert L.gns_ex_aggregate(task.agg._h, f, 1, out) == _lib.GNS_E_ARG
    n = ct.c_uint64(0)
    assert L.gns_ex_heavy_hitters(task.agg._h, 2, 0, 0, None, None, ct.byref(n)) == _lib.GNS_E_ARG
    assert L.gns_ex_heavy_hitters(task.agg._h, 0, 0, 0, None, None, None) == _lib.GNS_E_ARG


def test_tasks_through_the_manager(gpu, oracle):
    from go2netspectra_amd import FlowLifecycle, HeavyHitter, Manager, TaskSummary, parse_config
    from go2netspectra_amd.exact import key_string
    cfg = parse_config("""
aggregator:
  types: ["exact"]
  exact:
    tasks:
      - name: "per_five_tuple"
        key_fields: ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
        num_shards: 128
      - name: "per_dst"
        key_fields: ["DstIP", "DstPort"]
""")
    t, ipver, ts = stream()
    mgr = Manager(cfg, max_flows=1 << 12)
    mgr.start()
    mgr.process(batch_of(t, ipver, ts))
    for task in mgr.tasks():
        fields = task.key_fields
        want = oracle_export(oracle, fields, t, ipver, ts)
        rows = truth_rows(want, fields)
        for i in (0, 17, 59_999):
            dip, dport = respell(packet_value(t, ipver, i, "DstIP"), i), packet_value(t, ipver, i, "DstPort")
            e = truth_summary(rows, fields, {"DstIP": dip, "DstPort": dport})
            assert task.aggregate_flows(dst_ip=dip, dst_port=dport) == TaskSummary(task.name(), e.bytes, e.packets, e.flows)
            assert task.trace_flow({"DstIP": dip, "DstPort": str(dport)}) == \
                FlowLifecycle(e.first_ns, e.last_ns, e.max_packets, e.max_bytes)
            e = truth_summary(rows, fields, {"SrcIP": packet_value(t, ipver, i, "SrcIP")})
            assert task.aggregate_flows(src_ip=packet_value(t, ipver, i, "SrcIP")).FlowCount == e.flows
        reqs = [dict(), dict(protocol=6), dict(dst_port=int(t["dport"][5])), dict(dst_ip="203.0.113.9")]
        names = [{}, {"Protocol": 6}, {"DstPort": int(t["dport"][5])}, {"DstIP": "203.0.113.9"}]
        exp = [truth_summary(rows, fields, f) for f in names]
        assert task.aggregate_flows_many(reqs) == [TaskSummary(task.name(), e.bytes, e.packets, e.flows) for e in exp]
        for type_ in (0, 1):
            exp = [HeavyHitter(key_string(k, fields)[0], v) for k, v in truth_heavy(want, fields, type_, 0, 25)]
            assert_same_list(task.heavy_hitters(type_, 25), exp, "QueryHeavyHitters")
        assert task.heavy_hitters(0, 0) == [] and task.heavy_hitters(7, 10) == []
        # AlerterMsg from the device totals == the message built from the snapshot totals
        keys, st, en, pk, by = task.agg.snapshot_arrays()
        rules = [{"name": "r", "task_name": task.name(), "metric": m, "operator": ">", "threshold": 1}
                 for m in ("total_packets", "total_bytes", "total_flows", "other")]
        msg = task.alerter_msg(rules)
        for metric, value, unit in (("total_packets", int(pk.sum()), "packets"), ("total_bytes", int(by.sum()), "bytes"),
                                    ("total_flows", len(pk), "flows")):
            assert (f"<li><b>Metric:</b> <code>{metric}</code></li><li><b>Condition:</b> <code>> 1.00</code></li>"
                    f"<li><b>Observed Value:</b> <code>{float(value):.0f} {unit}</code></li></ul>") in msg
        assert msg.count("<h3>Alert: r</h3>") == 3
    mgr.stop()
