"""Truth side of the history roll-up tests: the reference's GROUP BY over the latest stored rows.

A roll-up of a history as of T is the SQL the reference would run over its flow_metrics rows:
per flow the row argMax(..., Timestamp) with Timestamp <= T (HistoryTruth.latest), its key
projected onto the destination's fields -- IP fields optionally masked to a prefix -- and then
GROUP BY the projected key with sum(PacketCount), sum(ByteCount) (u64 wrap), min(StartTime),
max(EndTime) (signed), as AggregateFlows and TraceFlow have it (querier.go:251-372).  A group
whose packets sum to exactly 0 is not a flow.  Key bytes come from key_bytes_of, fields are cut
at the offsets of the layout, masks are Python's ipaddress network arithmetic
(prefix_truth.network_of).  Nothing here comes from the engine.
"""
from __future__ import annotations

import numpy as np

from prefix_truth import network_of, pair_of

SIZE = {"SrcIP": 16, "DstIP": 16, "SrcPort": 2, "DstPort": 2, "Protocol": 1}


def offsets(fields) -> dict:
    """field -> (byte offset, size) in a key of this layout (the first occurrence of a field)."""
    out, o = {}, 0
    for f in fields:
        out.setdefault(f, (o, SIZE[f]))
        o += SIZE[f]
    return out


def project(keys, src_fields, dst_fields, prefix=None) -> np.ndarray:
    """[n, K_src] key bytes -> [n, K_dst]: every destination field copied from where the source
    holds it, an IP field with a prefix replaced by its network address."""
    keys = np.asarray(keys, np.uint8).reshape(len(keys), sum(SIZE[f] for f in src_fields))
    where = offsets(src_fields)
    cols = []
    for f in dst_fields:
        o, n = where[f]  # KeyError: a field the source lacks
        part = keys[:, o:o + n].copy()
        if prefix and f in prefix and f in ("SrcIP", "DstIP"):
            v4, v6 = pair_of(prefix[f])
            memo = {}
            for i in range(len(part)):
                b = part[i].tobytes()
                if b not in memo:
                    memo[b] = np.frombuffer(network_of(b, v4, v6), np.uint8)
                part[i] = memo[b]
        cols.append(part)
    return np.concatenate(cols, axis=1) if len(keys) else np.zeros((0, sum(SIZE[f] for f in dst_fields)), np.uint8)


def group_by(pkeys, start, end, pkts, bytes_) -> list:
    """GROUP BY the rows of pkeys: sorted [(key bytes, min start, max end, sum pkts, sum bytes)],
    sums in uint64 (wrapping), times in int64, zero-sum groups dropped."""
    n = len(pkeys)
    if n == 0:
        return []
    uniq, inv = np.unique(np.asarray(pkeys, np.uint8), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(n)
    g = len(uniq)
    pk, by = np.zeros(g, np.uint64), np.zeros(g, np.uint64)
    st = np.full(g, np.iinfo(np.int64).max, np.int64)
    en = np.full(g, np.iinfo(np.int64).min, np.int64)
    with np.errstate(over="ignore"):
        np.add.at(pk, inv, np.asarray(pkts, np.uint64))
        np.add.at(by, inv, np.asarray(bytes_, np.uint64))
    np.minimum.at(st, inv, np.asarray(start, np.int64))
    np.maximum.at(en, inv, np.asarray(end, np.int64))
    rows = [(uniq[i].tobytes(), int(st[i]), int(en[i]), int(pk[i]), int(by[i])) for i in range(g) if pk[i] != 0]
    return sorted(rows)


def rollup_rows(keys, start, end, pkts, bytes_, src_fields, dst_fields, prefix=None) -> list:
    return group_by(project(keys, src_fields, dst_fields, prefix), start, end, pkts, bytes_)


def latest_arrays(tr, T):
    """(keys [n, K], start, end, pkts, bytes) of HistoryTruth.latest(T)."""
    c = tr.cols()
    idx = tr.latest(T)
    K = sum(SIZE[f] for f in tr.fields)
    keys = np.frombuffer(b"".join(c["kb"][i] for i in idx), np.uint8).reshape(len(idx), K)
    return keys, c["start"][idx], c["end"][idx], c["pkts"][idx], c["bytes"][idx]


def rollup_truth(tr, T, dst_fields, prefix=None) -> list:
    """The roll-up of HistoryTruth ``tr`` as of T onto ``dst_fields``."""
    return rollup_rows(*latest_arrays(tr, T), tr.fields, dst_fields, prefix)


class RowLog:
    """Snapshots given as raw rows (ExactHistory.append_rows): the latest row per key as of T."""

    def __init__(self, fields):
        self.fields = list(fields)
        self.snaps = []  # (timestamp, keys [n, K], start, end, pkts, bytes)

    def append(self, timestamp, keys, start, end, pkts, bytes_) -> None:
        assert not self.snaps or timestamp > self.snaps[-1][0]
        keys = np.asarray(keys, np.uint8)
        assert len({k.tobytes() for k in keys}) == len(keys)
        self.snaps.append((timestamp, keys, np.asarray(start, np.int64), np.asarray(end, np.int64),
                           np.asarray(pkts, np.uint64), np.asarray(bytes_, np.uint64)))

    def latest(self, T):
        rows = {}
        for ts, keys, st, en, pk, by in self.snaps:
            if T is not None and ts > T:
                break
            for i in range(len(keys)):
                rows[keys[i].tobytes()] = (int(st[i]), int(en[i]), int(pk[i]), int(by[i]))
        K = sum(SIZE[f] for f in self.fields)
        keys = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), K)
        v = list(rows.values())
        col = lambda j, dt: np.array([r[j] for r in v], dt).reshape(len(v))
        return keys, col(0, np.int64), col(1, np.int64), col(2, np.uint64), col(3, np.uint64)

    def rollup(self, T, dst_fields, prefix=None) -> list:
        return rollup_rows(*self.latest(T), self.fields, dst_fields, prefix)


def combine(a: list, b: list) -> list:
    """Two roll-ups into one destination: counts add, min start, max end; zero sums are no flows."""
    out = {r[0]: r[1:] for r in a}
    for k, st, en, pk, by in b:
        if k in out:
            s0, e0, p0, b0 = out[k]
            out[k] = (min(s0, st), max(e0, en), (p0 + pk) & (2**64 - 1), (b0 + by) & (2**64 - 1))
        else:
            out[k] = (st, en, pk, by)
    return sorted((k,) + v for k, v in out.items() if v[2] != 0)
