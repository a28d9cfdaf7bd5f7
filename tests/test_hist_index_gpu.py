"""The seams of the key index both histories share (HistIndex, gns_histindex.hip), at the
smallest shapes that can break them: ids an append has already resolved survive an index growth
that a later list of the same append causes, and an append that is refused for a duplicate after
the index has grown leaves nothing behind.  Every answer is compared with the truth helpers of
the history tests (heavy_history_truth.py, history_truth.py: the reference's SQL restated over
the appended rows), never with the code under test.  The rollback of a trim's index rebuild is
not reachable without a failing device call and is not tested here."""
import numpy as np
import pytest

from exact_query_truth import key_bytes_of, to_filter
from go2netspectra_amd import ExactHistory, GnsError, HeavyHistory, _lib
from heavy_history_truth import HeavyTruth
from history_truth import HistoryTruth
from test_exact_history_gpu import assert_history_equals_truth
from test_heavy_history_gpu import assert_history_is, entries
from test_heavy_history_trim_gpu import assert_points

pytestmark = pytest.mark.gpu


def flow_pool(K, n, seed):
    """n distinct K-byte flows in a seeded random order."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 256, (4 * n, K), dtype=np.uint8), axis=0)
    assert len(pool) >= n
    return pool[rng.permutation(len(pool))[:n]]


# --- 1. ids of earlier lists survive a growth caused by a later list ---
@pytest.mark.parametrize("K", [4, 37])
def test_earlier_lists_survive_a_growth_in_a_later_list(gpu, K):
    """64 slots.  Snapshot 10 lists flows 0..7 (type 0).  Snapshot 20 is one append of three lists of
    40 rows: flows 0..39 (type 0), 30..69 (type 1), 60..99 (type 2), 100 distinct flows.  List 0
    fits (40 claimed slots, under the cap of 48); when list 1 starts the load has reached 1/2 and
    the index doubles with list 0's 40 ids resolved; when list 2 starts, 70 of 128 slots are
    claimed and it doubles again with 80 ids resolved."""
    rng = np.random.default_rng(K)
    pool = flow_pool(K, 110, 11 + K)
    hist = HeavyHistory(K, max_rows=64, max_flows=32)
    tr = HeavyTruth(decode=bytes.hex)
    assert hist.stats()["index_slots"] == 64
    v0 = rng.integers(1, 1000, 8).astype(np.uint32)
    assert hist.append(10, {0: (pool[:8], v0)}) == (8, 8)
    tr.record(10, {0: entries(pool[:8], v0)})
    lists = {ty: (pool[lo:lo + 40][rng.permutation(40)], rng.integers(0, 1000, 40).astype(np.uint32))
             for ty, lo in ((0, 0), (1, 30), (2, 60))}
    grown = hist.stats()["index_growths"]
    assert hist.append(20, lists) == (120, 112)
    tr.record(20, {ty: entries(f, v) for ty, (f, v) in lists.items()})
    st = hist.stats()
    assert st["index_growths"] >= grown + 1 and st["keys"] == 120 and st["rows"] == 128
    assert tr.probe_times()[:4] == [9, 10, 15, 20]  # (as of the one-list snapshot and as of the three lists)
    assert_history_is(hist, tr, (0, 1, 2), f"K {K}", thresholds=(500,))
    assert_points(hist, tr, (0, 1, 2), pool, f"K {K}")
    hist.close()


# --- 2. a duplicate found after a growth leaves nothing behind ---
def test_exact_duplicate_after_a_growth_leaves_nothing(gpu):
    """64 slots.  200 distinct keys and a repeat of key 3 as the last row: the resolve grows the
    index, then the call is refused.  20 of the keys are in the first snapshot."""
    fields = ["SrcIP", "DstPort"]
    rng = np.random.default_rng(2)
    names = [f"10.1.{i // 200}.{i % 200 + 1}-{1000 + i}" for i in range(220)]
    keys = np.frombuffer(b"".join(key_bytes_of(s, fields) for s in names), np.uint8).reshape(220, 18)
    start, end = rng.integers(-(1 << 40), 0, 220), rng.integers(0, 1 << 40, 220)
    pkts, nbytes = rng.integers(1, 1000, 220).astype(np.uint64), rng.integers(64, 1 << 20, 220).astype(np.uint64)

    def rows(sel, scale=1):
        return keys[sel], start[sel], end[sel], pkts[sel] * scale, nbytes[sel] * scale

    def export(sel, scale=1):
        return {names[i]: (int(start[i]), int(end[i]), int(pkts[i]) * scale, int(nbytes[i]) * scale) for i in sel}

    hist = ExactHistory(fields, max_rows=64, max_flows=32)
    tr = HistoryTruth(fields)
    assert hist.stats()["index_slots"] == 64
    first = np.arange(190, 210)
    assert hist.append_rows(*rows(first), 10) == (20, 20)
    tr.record(10, export(first))
    filters = [{}, {"SrcIP": "10.1.0.4"}, {"DstPort": 1195}, {"SrcIP": "10.1.0.0/24"}, {"SrcIP": "10.9.9.9"}]
    engine_filters = [to_filter(f) for f in filters]

    def check(what):
        matches = [tr.matches(f) for f in filters]
        for T in (9, 10, 15, 20, None):
            assert_history_equals_truth(hist, tr, filters, engine_filters, matches, T, what)

    def state():
        return (hist.times(), hist.stats()["keys"], hist.stats()["rows"], hist.aggregate(engine_filters),
                [a.tobytes() for a in hist.snapshot_arrays()], [a.tobytes() for a in hist.export_log()])
    check("one snapshot")
    before, grown = state(), hist.stats()["index_growths"]
    sel = np.concatenate([np.arange(200), [3]])
    with pytest.raises(GnsError, match="history append: two rows of the call have the same key") as e:
        hist.append_rows(*rows(sel, 2), 20)
    assert e.value.code == _lib.GNS_E_ARG
    assert hist.stats()["index_growths"] >= grown + 1  # (the duplicate was found in the grown index)
    assert state() == before
    check("after the refused call")
    assert hist.append_rows(*rows(np.arange(200), 2), 20) == (200, 190)
    tr.record(20, export(range(200), 2))
    assert hist.times() == [10, 20] and hist.stats()["keys"] == 210 and hist.stats()["rows"] == 220
    check("after the good call")
    hist.close()


@pytest.mark.parametrize("K", [4, 37])
def test_heavy_duplicate_after_a_growth_leaves_nothing(gpu, K):
    """The same on the heavy-hitter history, with one list."""
    rng = np.random.default_rng(30 + K)
    pool = flow_pool(K, 220, 31 + K)
    hist = HeavyHistory(K, max_rows=64, max_flows=32)
    tr = HeavyTruth(decode=bytes.hex)
    v0 = rng.integers(0, 1000, 20).astype(np.uint32)
    assert hist.append(10, {1: (pool[190:210], v0)}) == (20, 20)
    tr.record(10, {1: entries(pool[190:210], v0)})

    def state():
        return (hist.times(), hist.stats()["keys"], hist.stats()["rows"], [a.tobytes() for a in hist.export_log()])
    before, grown = state(), hist.stats()["index_growths"]
    vals = rng.integers(0, 1000, 201).astype(np.uint32)
    flows = np.concatenate([pool[:200], pool[3:4]])
    with pytest.raises(GnsError, match="heavy history append: two rows of a list name the same flow") as e:
        hist.append(20, {1: (flows, vals)})
    assert e.value.code == _lib.GNS_E_ARG
    assert hist.stats()["index_growths"] >= grown + 1
    assert state() == before
    assert_history_is(hist, tr, (1, 0), f"K {K} after the refused call", thresholds=(500,))
    assert_points(hist, tr, (1, 0), pool, f"K {K} after the refused call")
    assert hist.append(20, {1: (flows[:200], vals[:200])}) == (200, 190)
    tr.record(20, {1: entries(flows[:200], vals[:200])})
    assert hist.stats()["keys"] == 210 and hist.stats()["rows"] == 220
    assert_history_is(hist, tr, (1, 0), f"K {K} after the good call", thresholds=(500,))
    assert_points(hist, tr, (1, 0), pool, f"K {K} after the good call")
    hist.close()
