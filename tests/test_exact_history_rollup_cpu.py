"""CPU side of the history roll-up (gns_ex_hist_rollup): the truth module against a brute-force
restatement and against the oracle fed a monotone stream, and the header / binding of the call."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from exact_query_truth import FIVE
from history_rollup_truth import RowLog, combine, group_by, offsets, project, rollup_rows, rollup_truth
from history_truth import HistoryTruth
from prefix_truth import mask_packets, prefix_stream

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "gns_sketch.h")
M64 = (1 << 64) - 1
I64 = np.iinfo(np.int64)


def mapped(a, b, c, d):
    return bytes(10) + b"\xff\xff" + bytes([a, b, c, d])


def random_rows(rng, n):
    """n distinct (SrcIP, SrcPort, Protocol) rows over few addresses, ports and protocols, times
    of both signs and at the int64 extremes, one pair of rows whose packets sum to 2^64."""
    seen, keys = set(), []
    while len(keys) < n:
        if rng.random() < 0.5:
            ip = mapped(10, int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 20)))
        else:
            ip = bytes([0x20, 0x01]) + bytes(5) + bytes([int(rng.integers(0, 2))]) + bytes(7) + bytes([int(rng.integers(0, 20))])
        k = ip + int(rng.integers(0, 4)).to_bytes(2, "big") + bytes([int(rng.integers(0, 3))])
        if k not in seen:
            seen.add(k)
            keys.append(k)
    keys = np.frombuffer(b"".join(keys), np.uint8).reshape(n, 19).copy()
    st = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
    en = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
    st[:4] = [I64.min, I64.max, -1, 0]
    en[:4] = [I64.max, I64.min, 0, -1]
    pk = rng.integers(1, 1 << 40, n).astype(np.uint64)
    by = rng.integers(1, 1 << 63, n).astype(np.uint64) * np.uint64(2)  # sums wrap
    return keys, st, en, pk, by


def brute(keys, st, en, pk, by, src, dst, prefix):
    """The GROUP BY as a dict over Python ints, the mask through exact.mask_keys."""
    from go2netspectra_amd import mask_keys
    where = offsets(src)
    out = {}
    for i in range(len(keys)):
        k = b""
        for f in dst:
            o, n = where[f]
            part = keys[i:i + 1, o:o + n]
            if prefix and f in prefix:
                part = mask_keys(part, [f], {f: prefix[f]})
            k += part.tobytes()
        s0, e0, p0, b0 = out.get(k, (None, None, 0, 0))
        out[k] = (int(st[i]) if s0 is None else min(s0, int(st[i])), int(en[i]) if e0 is None else max(e0, int(en[i])),
                  (p0 + int(pk[i])) & M64, (b0 + int(by[i])) & M64)
    return sorted((k,) + v for k, v in out.items() if v[2] != 0)


@pytest.mark.parametrize("dst,prefix", [
    (["SrcIP"], None), (["Protocol"], None), (["Protocol", "SrcIP"], None), (["SrcIP", "SrcPort", "Protocol"], None),
    (["SrcIP"], {"SrcIP": (24, 64)}), (["SrcIP"], {"SrcIP": (0, 0)}), (["SrcPort", "SrcIP"], {"SrcIP": (17, 57)}),
], ids=lambda v: "-".join(v) if isinstance(v, list) else str(v))
def test_truth_equals_a_brute_force_group_by(dst, prefix):
    src = ["SrcIP", "SrcPort", "Protocol"]
    keys, st, en, pk, by = random_rows(np.random.default_rng(5), 300)
    # two rows with 2^63 packets each that share address and protocol (99, which no other row has) and
    # differ in the port: a group that vanishes wherever the port is dropped and the protocol kept
    keys[10, 18] = keys[11, 18] = 99
    keys[11, :16] = keys[10, :16]
    keys[11, 16:18] = keys[10, 16:18] ^ 0xFF
    pk[10] = pk[11] = np.uint64(1 << 63)
    got = rollup_rows(keys, st, en, pk, by, src, dst, prefix)
    want = brute(keys, st, en, pk, by, src, dst, prefix)
    assert got == want
    assert (st < 0).any() and (st > 0).any() and (en < 0).any() and (en > 0).any()
    assert any(r[1] < 0 for r in got) and (len(got) < 300 or "SrcPort" in dst)
    if dst[0] == "Protocol":  # rows 10 and 11 are the whole group of protocol 99 (and of 99 ‖ their address)
        assert not any(r[0][0] == 99 for r in got), "the zero-sum group is listed"
        assert sum(r[3] for r in got) & M64 == sum(int(x) for x in pk) & M64
    assert sum(int(x) for x in by) > M64, "the byte sums do not wrap"


def test_wrapped_sums_and_zero_sum_groups_by_hand():
    k = np.array([[6], [6], [17], [17], [1]], np.uint8)
    rows = group_by(k, [5, -7, 3, 9, -2], [-9, -8, 4, 1, -3],
                    np.array([1 << 63, 1 << 63, 1, 2, 7], np.uint64), np.array([1, 2, (1 << 64) - 1, 5, 0], np.uint64))
    assert rows == [(b"\x01", -2, -3, 7, 0), (b"\x11", 3, 4, 3, 4)]
    assert combine(rows, [(b"\x11", -1, 2, M64 - 2, 1), (b"\x02", 1, 1, 1, 1)]) == [(b"\x01", -2, -3, 7, 0), (b"\x02", 1, 1, 1, 1)]
    assert project(k, ["Protocol"], ["Protocol", "Protocol"]).tolist() == [[6, 6], [6, 6], [17, 17], [17, 17], [1, 1]]
    with pytest.raises(KeyError):
        project(k, ["Protocol"], ["SrcIP"])


def test_rowlog_takes_the_latest_row_per_key():
    log = RowLog(["Protocol"])
    log.append(10, [[6], [17]], [1, 2], [3, 4], [5, 6], [7, 8])
    log.append(20, [[6]], [-1], [-2], [1], [1])
    assert log.rollup(9, ["Protocol"]) == []
    assert log.rollup(10, ["Protocol"]) == [(b"\x06", 1, 3, 5, 7), (b"\x11", 2, 4, 6, 8)]
    assert log.rollup(None, ["Protocol"]) == [(b"\x06", -1, -2, 1, 1), (b"\x11", 2, 4, 6, 8)]


COARSE = [(["SrcIP"], None), (["DstIP", "DstPort"], None), (["Protocol"], None), (FIVE[::-1], None),
          (["SrcIP"], {"SrcIP": (24, 64)}), (["SrcIP", "DstIP"], {"SrcIP": (16, 48), "DstIP": (8, 32)})]


def test_truth_equals_the_oracle_fed_a_monotone_stream(oracle):
    """Timestamps monotone in arrival and no reset: a coarse task's start / end (first / last
    packet of the group) are the min / max over its flows' rows, so the GROUP BY over the latest
    rows as of each snapshot equals oracle.Exact(coarse fields) fed the packets up to it."""
    from exact_query_truth import key_bytes_of
    t, ipver, _ = prefix_stream(nflows=1500)
    n, cuts = 12_000, [3_000, 3_000, 7_500, 12_000]  # (the second snapshot stores the same table again)
    ts = (np.arange(n, dtype=np.int64) - 4_000) * 1_000  # negative, then positive
    feed = lambda o, tt, sel: o.insert_tuples(tt["src16"][sel], tt["dst16"][sel], tt["sport"][sel], tt["dport"][sel],
                                              tt["proto"][sel], ipver[sel], tt["length"][sel], ts[sel.start:sel.stop])
    fine, tr, done = oracle.Exact(FIVE), HistoryTruth(FIVE), 0
    for i, c in enumerate(cuts):
        if c > done:
            feed(fine, t, slice(done, c))
            done = c
        tr.record(100 + i, fine.export())
    for fields, prefix in COARSE:
        masked = mask_packets(t, ipver[:len(t["proto"])], prefix)
        for i, c in enumerate(cuts):
            o = oracle.Exact(fields)
            feed(o, masked, slice(0, c))
            want = sorted((key_bytes_of(k, fields), st, en, pk, by) for k, (st, en, pk, by) in o.export().items())
            got = rollup_truth(tr, 100 + i, fields, prefix)
            assert got == want, (fields, prefix, i)
            assert 0 < len(got) <= len(tr.latest(100 + i))
        assert rollup_truth(tr, 99, fields, prefix) == []
        assert rollup_truth(tr, None, fields, prefix) == rollup_truth(tr, 103, fields, prefix)


def test_header_declares_the_call_and_lib_binds_it():
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.findall(r"\bint\s+gns_ex_hist_rollup\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert len(m) == 1, "gns_ex_hist_rollup is not declared exactly once"
    args = [a.strip() for a in m[0].split(",") if a.strip()]
    assert len(args) == 5
    assert args[0].startswith("gns_ex *") and args[1].startswith("gns_ex_hist *") and "int64_t" in args[2]
    assert "gns_prefix" in args[3] and "uint64_t" in args[4]
    assert "Not offered: roll-ups\n * of a history" not in raw and "roll-ups of a history" not in raw
    assert "min(StartTime)" in raw and "stream-order rule" in raw
    from go2netspectra_amd import _lib
    assert "gns_ex_hist_rollup" in _lib.EXPORTED
    try:
        L = _lib.load()
    except OSError:
        pytest.skip("the library does not load on this machine")
    fn = L.gns_ex_hist_rollup
    assert fn.restype is ct.c_int and fn.argtypes == [ct.c_void_p] * 5
    # a null handle is an argument error before any device call
    out = (ct.c_uint64 * 2)(3, 4)
    assert fn(None, None, None, None, out) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()
    assert (out[0], out[1]) == (3, 4)


def test_python_surface_and_argument_errors_come_first():
    from go2netspectra_amd import ExactAggregator, ExactHistory, ExactTask
    import inspect
    for cls, name in ((ExactAggregator, "rollup_from_history"), (ExactHistory, "rollup"), (ExactHistory, "table"),
                      (ExactHistory, "spread"), (ExactHistory, "hierarchical_heavy_hitters")):
        assert callable(getattr(cls, name)), name
    for name in ("rollup", "spread", "hierarchical_heavy_hitters"):
        p = inspect.signature(getattr(ExactTask, name)).parameters
        assert "end_time" in p and p["end_time"].default is None, name
    # no handle and no library: the checks come before any call
    h = ExactHistory.__new__(ExactHistory)
    h._h, h._L, h.key_fields, h.key_bytes, h.device = None, None, ["SrcIP", "Protocol"], 17, 0
    with pytest.raises(ValueError, match="DstIP"):
        h.rollup(["DstIP"])
    with pytest.raises(ValueError):
        h.rollup(["SrcIP"], prefix={"SrcIP": 33})
    with pytest.raises(ValueError):
        h.rollup(["SrcIP"], prefix={"SrcIP": (8, 129)})
    with pytest.raises(ValueError):
        h.rollup(["SrcIP"], end_time=1 << 63)
    with pytest.raises(ValueError):
        h.spread(["SrcIP"], ["DstIP"])
    with pytest.raises(ValueError):
        h.hierarchical_heavy_hitters("SrcPort", [(32, 128)], 0, 1)
    with pytest.raises(ValueError):
        h.hierarchical_heavy_hitters("SrcIP", [(32, 128)], 0, 1, end_time=-(1 << 63) - 1)
    a = ExactAggregator.__new__(ExactAggregator)
    a._h, a._L, a.key_fields, a.key_bytes, a.device = None, None, ["SrcIP"], 16, 0
    with pytest.raises(TypeError):
        a.rollup_from_history(a)
    other = ExactHistory.__new__(ExactHistory)
    other._h, other._L, other.key_fields, other.key_bytes, other.device = None, None, ["SrcIP"], 16, 1
    with pytest.raises(ValueError, match="device"):
        a.rollup_from_history(other)
    task = ExactTask.__new__(ExactTask)
    task.name_, task.key_fields, task.agg = "t", ["SrcIP"], a
    for call in (lambda: task.rollup("r", ["SrcIP"], end_time=5), lambda: task.spread(["SrcIP"], ["SrcIP"], end_time=5),
                 lambda: task.hierarchical_heavy_hitters("SrcIP", [(32, 128)], 0, 1, end_time=5)):
        with pytest.raises(ValueError, match="end_time"):
            call()
