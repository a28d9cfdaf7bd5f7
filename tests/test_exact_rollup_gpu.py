"""Roll-up of the exact aggregator on the GPU (gns_ex_rollup): a resident flow table re-keyed
onto a coarser (or permuted, or equal) layout equals oracle.Exact keyed on that layout and fed
the same packets -- keys, StartTime, EndTime, packets and bytes, with timestamps that are not
monotonic, so that start / end must follow stream order and not min / max.

Inputs: the tricky stream of exact_query_truth.py (IPv4, IPv4-mapped and IPv6 aliases of the
same flows, random timestamps in [-2^40, 2^40), wire lengths near 2^32), with the IPv4 source
addresses folded onto 256 values so that a source address groups many flows whose packets
interleave in the stream.  Device batches are 16K packets: every table is built from several."""
import numpy as np
import pytest

from exact_query_truth import (FIVE, batch_of, got_heavy, key_bytes_of, oracle_export, packet_value, to_filter,
                               tricky_stream, truth_heavy, truth_rows, truth_summary)
from helpers import assert_same_flows, assert_same_list

pytestmark = pytest.mark.gpu

N = 60_000
M64 = (1 << 64) - 1
_CACHE = {}


def fold_sources(t):
    """IPv4 sources a.b.c.d -> a.0.0.0 in each of the three forms a packet carries one in (the
    4-byte slot, the IPv4-mapped 16 bytes, and the 16-byte IPv6 alias of the slot bytes): plain
    and mapped arrivals still print the same string, the alias still another one."""
    s = t["src16"]
    mapped = (s[:, :10] == 0).all(1) & (s[:, 10:12] == 0xFF).all(1)
    slot = (s[:, 4:] == 0).all(1) & ~mapped
    s[mapped, 13:16] = 0
    s[slot, 1:4] = 0


def stream(nflows=5000, seed=17):
    if (nflows, seed) not in _CACHE:
        t, ipver, ts = tricky_stream(seed, N, nflows)
        fold_sources(t)
        _CACHE[nflows, seed] = (t, ipver, ts)
    return _CACHE[nflows, seed]


def truth(oracle, fields, sel=slice(None), nflows=5000):
    """oracle.Exact keyed on ``fields`` over packets ``sel``, as key bytes -> (start, end, packets, bytes)."""
    key = (tuple(fields), sel.start, sel.stop, nflows)
    if key not in _CACHE:
        t, ipver, ts = stream(nflows)
        _CACHE[key] = {key_bytes_of(k, fields): v for k, v in oracle_export(oracle, fields, t, ipver, ts, sel).items()}
    return _CACHE[key]


def new_agg(fields, max_flows=1 << 12):
    from go2netspectra_amd import ExactAggregator
    return ExactAggregator(fields, max_flows=max_flows, batch_packets=16384)


def feed(agg, sel=slice(None), nflows=5000, pieces=3):
    t, ipver, ts = stream(nflows)
    idx = np.arange(N)[sel]
    for part in np.array_split(idx, pieces):
        agg.insert_tuples(batch_of(t, ipver, ts, part))
    agg.flush()


def as_dict(arrays):
    from go2netspectra_amd import apply_delta
    return apply_delta({}, arrays)


def merge_truth(state, rows):
    """gns_ex_merge restated on a key -> (start, end, packets, bytes) map; rows in order."""
    out = dict(state)
    keys, st, en, pk, by = rows
    for i in range(len(pk)):
        if int(pk[i]) == 0:
            continue
        k = bytes(keys[i])
        if k in out:
            s, _, p, b = out[k]
            out[k] = (s, int(en[i]), (p + int(pk[i])) & M64, (b + int(by[i])) & M64)
        else:
            out[k] = (int(st[i]), int(en[i]), int(pk[i]), int(by[i]))
    return out


def rows_of(d):
    """A key -> state map as merge rows (any order: the keys are distinct)."""
    ks = list(d)
    return (np.array([list(k) for k in ks], np.uint8), np.array([d[k][0] for k in ks], np.int64),
            np.array([d[k][1] for k in ks], np.int64), np.array([d[k][2] for k in ks], np.uint64),
            np.array([d[k][3] for k in ks], np.uint64))


def same_arrays(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def five(gpu, oracle):
    """The whole stream in a FIVE-keyed handle, three inserts of several device batches each."""
    src = new_agg(FIVE)
    feed(src)
    assert_same_flows(as_dict(src.snapshot_arrays()), truth(oracle, FIVE), "the source table itself")
    yield src
    src.close()


# --- 1. parity with a task keyed on the coarser layout ---
LAYOUTS = [["SrcIP"], ["DstPort", "Protocol"], ["DstIP", "SrcIP", "SrcPort"], ["Protocol"], FIVE]


@pytest.mark.parametrize("fields", LAYOUTS, ids=lambda f: "-".join(f))
def test_rollup_equals_a_task_keyed_on_the_layout(five, oracle, fields):
    want = truth(oracle, fields)
    n_src = five.counters()["flows"]
    assert n_src == len(truth(oracle, FIVE))
    dst = new_agg(fields)
    projected, new = dst.rollup_from(five)
    assert (projected, new) == (n_src, len(want))
    got = as_dict(dst.snapshot_arrays())
    assert_same_flows(got, want, f"roll-up to {fields}")
    assert dst.counters()["flows"] == len(want)
    if fields == ["SrcIP"]:  # the groups are groups: far fewer keys than flows, times not min / max of the parts
        assert len(want) < n_src // 2
    dst.close()
    # ExactAggregator.rollup: the same table in a handle of its own
    again = five.rollup(fields, max_flows=1 << 12)
    assert again.key_fields == list(fields)
    assert_same_flows(as_dict(again.snapshot_arrays()), want, f"rollup({fields})")
    again.close()


def test_start_and_end_follow_stream_order_not_min_max(oracle):
    """The property the host route cannot give: for some source address the group's StartTime
    is not the smallest start of its flows (nor EndTime the largest end)."""
    want, parts = truth(oracle, ["SrcIP"]), truth(oracle, FIVE)
    lo, hi = {}, {}
    for k, (st, en, _, _) in parts.items():
        lo[k[:16]] = min(lo.get(k[:16], st), st)
        hi[k[:16]] = max(hi.get(k[:16], en), en)
    assert any(want[k][0] != lo[k] for k in want) and any(want[k][1] != hi[k] for k in want)


# --- 2. pieces and growth ---
def test_pieces_and_growth(gpu, oracle, monkeypatch):
    nfl = 12_000
    monkeypatch.setenv("GNS_EX_ROLLUP_PIECE", "256")
    src = new_agg(FIVE, max_flows=2048)  # 2^12 slots: grows under the stream
    feed(src, nflows=nfl)
    assert src.dict_stats()["growths"] >= 1
    n_src = src.counters()["flows"]
    fields = ["DstPort", "Protocol"]
    want = truth(oracle, fields, nflows=nfl)
    assert 5000 <= len(want) < n_src - 500  # hundreds of groups with flows in different pieces
    dst = new_agg(fields, max_flows=1)  # the smallest table
    projected, new = dst.rollup_from(src)
    assert (projected, new) == (n_src, len(want))
    assert dst.dict_stats()["growths"] >= 1
    assert src.dict_stats()["slots"] // 256 >= 64  # many pieces
    assert_same_flows(as_dict(dst.snapshot_arrays()), want, "many groups over many pieces")
    dst.close()
    # few groups, every one of them fed by every piece
    for fields in (["Protocol"], ["SrcIP"]):
        want = truth(oracle, fields, nflows=nfl)
        assert len(want) < n_src // 2
        dst = new_agg(fields, max_flows=1)
        assert dst.rollup_from(src) == (n_src, len(want))
        assert_same_flows(as_dict(dst.snapshot_arrays()), want, f"{fields} over many pieces")
        dst.close()
    src.close()


# --- 3. two sources, then packets ---
def test_two_sources_and_further_ingest(gpu, oracle):
    fields = ["SrcIP"]
    a_sel, b_sel, c_sel = slice(0, 25_000), slice(25_000, 50_000), slice(50_000, N)
    A, B = new_agg(FIVE), new_agg(FIVE)
    feed(A, a_sel)
    feed(B, b_sel)
    dst = new_agg(fields, max_flows=64)
    view = dst.view()
    dst.rollup_from(A)
    assert_same_flows(as_dict(dst.snapshot_arrays()), truth(oracle, fields, a_sel), "after the first source")
    cur = view.refresh()
    assert cur == 25_000  # dst's stream advanced by A's length
    projected, new = dst.rollup_from(B)
    want_ab = truth(oracle, fields, slice(0, 50_000))
    assert projected == B.counters()["flows"] and new == len(want_ab) - len(truth(oracle, fields, a_sel))
    assert_same_flows(as_dict(dst.snapshot_arrays()), want_ab, "after the second source")
    nxt = view.refresh(cur)
    assert nxt == 50_000
    delta = view.snapshot_arrays()
    touched = set(truth(oracle, fields, b_sel))
    assert len(delta[3]) == len(touched) and set(map(bytes, delta[0])) == touched
    assert_same_flows(as_dict(delta), {k: want_ab[k] for k in touched}, "the delta's rows are cumulative")
    feed(dst, c_sel)  # packets after the roll-ups come after every rolled-up flow
    assert_same_flows(as_dict(dst.snapshot_arrays()), truth(oracle, fields, slice(0, N)), "whole stream")
    assert view.refresh(nxt) == N
    assert set(map(bytes, view.snapshot_arrays()[0])) == set(truth(oracle, fields, c_sel))
    view.close()
    for h in (A, B, dst):
        h.close()


# --- 4. the source is untouched; of dst's counters only flows moves ---
def test_source_untouched_and_counters(five, oracle):
    fields = ["DstPort", "Protocol"]
    dst = new_agg(fields)
    feed(dst, slice(0, 10_000))
    snap0, c0, d0 = five.snapshot_arrays(), five.counters(), five.dict_stats()
    before = dst.counters()
    dst.rollup_from(five)
    assert same_arrays(five.snapshot_arrays(), snap0) and five.counters() == c0 and five.dict_stats() == d0
    after = dst.counters()
    assert {k for k in after if after[k] != before[k]} == {"flows"}
    want = merge_truth(truth(oracle, fields, slice(0, 10_000)), rows_of(truth(oracle, fields)))
    assert after["flows"] == len(want) > before["flows"]
    assert_same_flows(as_dict(dst.snapshot_arrays()), want, "existing keys keep start, take end, counts add")
    dst.close()


# --- 5. positions of merged rows, u64 wrap, reset ---
def test_merged_rows_wrap_and_reset(gpu, oracle):
    from go2netspectra_amd import rollup_plan
    fields = ["SrcIP"]
    s0, s1, s2 = slice(0, 20_000), slice(20_000, 40_000), slice(40_000, N)
    other, src = new_agg(FIVE), new_agg(FIVE)
    feed(other, s1)
    feed(src, s0)
    rows = [a.copy() for a in other.snapshot_arrays()]
    # one more row: a 5-tuple outside the stream under the busiest source address, 2^64 - 1 packets
    by_src = truth(oracle, fields, s0)
    busy = max(by_src, key=lambda k: by_src[k][2])
    assert by_src[busy][2] >= 3
    extra = bytearray(next(k for k in truth(oracle, FIVE, s0) if k[:16] == busy))
    seen = set(truth(oracle, FIVE))
    while bytes(extra) in seen:
        extra[32] ^= 0x5A
        extra[33] = (extra[33] + 1) & 0xFF
    rows[0] = np.concatenate([rows[0], np.frombuffer(bytes(extra), np.uint8)[None, :]])
    rows[1] = np.append(rows[1], np.int64(-77))
    rows[2] = np.append(rows[2], np.int64(1 << 41))
    rows[3] = np.append(rows[3], np.uint64(M64))
    rows[4] = np.append(rows[4], np.uint64(M64 - 4))
    src.merge(*rows)
    feed(src, s2)
    # a SrcIP-keyed handle fed the same inserts and merges: the rows projected, in their order
    plan = rollup_plan(FIVE, fields)
    want = merge_truth(by_src, (rows[0][:, plan],) + tuple(rows[1:]))
    want = merge_truth(want, rows_of(truth(oracle, fields, s2)))
    wrapped = want[busy]
    assert 0 < wrapped[2] < 1 << 40 and wrapped[3] < 1 << 63  # both sums went round
    dst = src.rollup(fields, max_flows=64)
    assert_same_flows(as_dict(dst.snapshot_arrays()), want, "inserts, merged rows, inserts")
    dst.close()
    # a new period of the source
    src.reset()
    feed(src, slice(5_000, 9_000))
    dst = src.rollup(fields, max_flows=64)
    assert_same_flows(as_dict(dst.snapshot_arrays()), truth(oracle, fields, slice(5_000, 9_000)), "only the new period")
    for h in (dst, src, other):
        h.close()


# --- 6. the result is a first-class handle ---
def test_result_is_a_first_class_task(five, oracle, tmp_path):
    from go2netspectra_amd import ExactTask, checkpoint
    t, ipver, ts = stream()
    fields = ["SrcIP", "DstIP"]
    base = ExactTask("five", FIVE, agg=five)
    task = base.rollup("pairs", fields, 64, max_flows=1 << 12)
    assert isinstance(task, ExactTask) and task.name() == "pairs" and task.shard_count == 64
    assert task.key_fields == fields
    export = oracle_export(oracle, fields, t, ipver, ts)
    want = truth(oracle, fields)
    # the query plane, restated on the oracle's export as test_exact_query_gpu.py does
    for metric in (0, 1):
        assert_same_list(got_heavy(*task.agg.heavy_hitters(metric, 0, 10)), truth_heavy(export, fields, metric, 0, 10),
                         f"top 10 by metric {metric}")
    rows = truth_rows(export, fields)
    probes = (0, 1, 777, 31_000, int(np.flatnonzero(ipver == 4)[0]))  # (the last: a folded source, many flows)
    filters = [{}] + [{"SrcIP": packet_value(t, ipver, i, "SrcIP")} for i in probes]
    filters.append({"SrcIP": bytes([203, 0, 113, 9])})  # no such source
    got = task.agg.aggregate([to_filter(f) for f in filters])
    exp = [truth_summary(rows, fields, f) for f in filters]
    assert got == exp
    assert exp[0].flows == len(want) and max(e.flows for e in exp[1:]) > 1 and exp[-1].flows == 0
    # flows(), snapshot(), query, a view
    assert {f.Key: (f.StartTime, f.EndTime, f.PacketCount, f.ByteCount) for f in task.flows()} == export
    assert sum(len(s.Flows) for s in task.snapshot().Shards) == len(want)
    k = next(iter(want))
    assert task.query(k) == ((want[k][2] << 32) | want[k][3]) & M64
    view = task.view()
    view.refresh()
    assert same_arrays(view.snapshot_arrays(), task.agg.snapshot_arrays())
    view.close()
    # checkpoint round trip
    path = tmp_path / "rolled.ckpt"
    task.save(path)
    back = ExactTask("back", fields, max_flows=64)
    back.restore(path)
    assert_same_flows(as_dict(back.agg.snapshot_arrays()), want, "checkpoint of a rolled-up table")
    checkpoint.save(back.agg, tmp_path / "again.ckpt")
    back.agg.close()
    # a roll-up of a roll-up: positions stay exact
    direct = five.rollup(["SrcIP"], max_flows=64)
    chained = task.agg.rollup(["SrcIP"], max_flows=64)
    assert_same_flows(as_dict(chained.snapshot_arrays()), truth(oracle, ["SrcIP"]), "FIVE -> SrcIP,DstIP -> SrcIP")
    assert_same_flows(as_dict(chained.snapshot_arrays()), as_dict(direct.snapshot_arrays()), "chained vs direct")
    for h in (direct, chained, task.agg):
        h.close()
    base.agg = None  # (the fixture owns the handle)


# --- 7. errors ---
def test_errors_leave_dst_untouched(gpu, oracle):
    import ctypes as ct
    from go2netspectra_amd import GnsError, _lib
    by_src, by_dst = new_agg(["SrcIP"]), new_agg(["DstIP"])
    feed(by_src, slice(0, 5_000), pieces=1)
    feed(by_dst, slice(0, 5_000), pieces=1)
    L = _lib.load()
    out = (ct.c_uint64 * 2)(3, 4)
    snap = by_dst.snapshot_arrays()
    cnt = by_dst.counters()
    # dst is src
    assert L.gns_ex_rollup(by_dst._h, by_dst._h, out) == _lib.GNS_E_ARG
    assert b"same handle" in L.gns_last_error()
    with pytest.raises(GnsError) as e:
        by_dst.rollup_from(by_dst)
    assert e.value.code == _lib.GNS_E_ARG
    # a field the source does not have: the library's own check, then the Python mirror of it
    assert L.gns_ex_rollup(by_dst._h, by_src._h, out) == _lib.GNS_E_ARG
    assert b"DstIP" in L.gns_last_error()
    with pytest.raises(ValueError, match="DstIP"):
        by_dst.rollup_from(by_src)
    with pytest.raises(ValueError, match="DstIP"):
        by_src.rollup(["DstIP"])
    assert same_arrays(by_dst.snapshot_arrays(), snap) and by_dst.counters() == cnt
    assert (out[0], out[1]) == (3, 4)
    view = by_dst.view()
    assert view.refresh() == 5_000  # no positions were spent
    view.close()
    # an empty source moves nothing
    empty = new_agg(FIVE)
    dst = new_agg(["DstIP"])
    assert dst.rollup_from(empty) == (0, 0)
    assert dst.counters()["flows"] == 0
    feed(dst, slice(0, 5_000), pieces=1)
    snap, cnt = dst.snapshot_arrays(), dst.counters()
    assert dst.rollup_from(empty) == (0, 0)
    assert same_arrays(dst.snapshot_arrays(), snap) and dst.counters() == cnt
    for h in (by_src, by_dst, empty, dst):
        h.close()
