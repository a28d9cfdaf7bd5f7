"""Truth side of the history delta tests: what changed between two times, over stored rows.

A window (T0, T1] of a history is two sets of stored rows.  L0 = the latest row of each flow as
of T0 (HistoryTruth.latest; empty for T0 = None, which here means "before everything") and L1 =
the same as of T1 (None: the newest).  The PLUS rows are L1 - L0, the rows current at T1 that
were stored in the window; the MINUS rows are L0 - L1, the rows current at T0 that were displaced
in it.  Both are projected (history_rollup_truth.project) and grouped by the projected key:
counts are sum(plus) - sum(minus) mod 2^64 -- the two's-complement signed change --, StartTime /
EndTime are the signed min / max over the group's PLUS rows only, and a group whose packet
change is exactly 0 is no flow.  Movers are a sort of those groups by (-|v|, key).

Which rows exist depends on how the history was stored: a whole view stores every flow again, a
delta view only the flows touched since the last one.  StoredTruth records an export the way the
task under test stores it (``full`` flags), so that row identities -- and with them the times of
coarser groups -- are those of the history compared against.  Nothing here comes from the engine.
"""
from __future__ import annotations

import numpy as np

from history_rollup_truth import SIZE, project
from history_truth import HistoryTruth

I64 = np.iinfo(np.int64)
M64 = (1 << 64) - 1


def signed(v: int) -> int:
    v &= M64
    return v - (1 << 64) if v >> 63 else v


class StoredTruth(HistoryTruth):
    """HistoryTruth whose i-th record stores what the i-th ``ExactTask.record(ts, full=full[i])``
    stores: the whole export, or the flows touched since the last record.  A flow was touched
    when its value differs from the last export's (every packet raises PacketCount) or when the
    oracle object is a new one (a reset: every flow of the new table arrived after it)."""

    def __init__(self, fields, full):
        super().__init__(fields)
        self.full, self.n_rec, self.last, self.last_oracle = list(full), 0, {}, None

    def record(self, timestamp: int, export: dict) -> None:
        whole = self.full[self.n_rec] if self.n_rec < len(self.full) else False
        fresh = getattr(self, "oracle", None) is not self.last_oracle
        stored = export if whole or fresh else {k: v for k, v in export.items() if self.last.get(k) != v}
        self.n_rec += 1
        self.last, self.last_oracle = dict(export), getattr(self, "oracle", None)
        super().record(timestamp, stored)


def window_sets(tr, T0, T1):
    """(plus, minus): sorted indices of tr's stored rows.  T0 None: before every row."""
    l1 = set(int(i) for i in tr.latest(T1))
    l0 = set() if T0 is None else set(int(i) for i in tr.latest(T0))
    return sorted(l1 - l0), sorted(l0 - l1)


def group_signed(pkeys, start, end, pkts, bytes_, n_plus, keep_zero=False) -> list:
    """GROUP BY the projected keys; rows [0, n_plus) are plus rows, the rest minus rows.  Sorted
    [(key, min start, max end, packet change, byte change)]: changes mod 2^64, times over the
    plus rows (a group without one keeps int64 max / min), groups with packet change 0 dropped
    unless ``keep_zero`` (the slots a destination claims, for answers combined afterwards)."""
    groups = {}
    for i in range(len(pkeys)):
        k = pkeys[i].tobytes()
        st, en, pk, by = groups.get(k, (int(I64.max), int(I64.min), 0, 0))
        if i < n_plus:
            groups[k] = (min(st, int(start[i])), max(en, int(end[i])), (pk + int(pkts[i])) & M64, (by + int(bytes_[i])) & M64)
        else:
            groups[k] = (st, en, (pk - int(pkts[i])) & M64, (by - int(bytes_[i])) & M64)
    return sorted((k,) + v for k, v in groups.items() if keep_zero or v[2] != 0)


def delta_truth(tr, T0, T1, dst_fields, prefix=None, keep_zero=False):
    """(group_signed's rows, rows selected) of window (T0, T1] of HistoryTruth ``tr`` onto
    ``dst_fields``."""
    plus, minus = window_sets(tr, T0, T1)
    idx = np.array(plus + minus, np.int64)
    if len(idx) == 0:
        return [], 0
    c = tr.cols()
    K = sum(SIZE[f] for f in tr.fields)
    keys = np.frombuffer(b"".join(c["kb"][i] for i in idx), np.uint8).reshape(len(idx), K)
    return group_signed(project(keys, tr.fields, dst_fields, prefix), c["start"][idx], c["end"][idx], c["pkts"][idx],
                        c["bytes"][idx], len(plus), keep_zero), len(idx)


def rowlog_sets(log, T0, T1):
    """(plus, minus) of a history_rollup_truth.RowLog: lists of (snapshot, row) pairs."""
    def latest(T, none_is_empty):
        if T is None and none_is_empty:
            return {}
        out = {}
        for si, (ts, keys, *_rest) in enumerate(log.snaps):
            if T is not None and ts > T:
                break
            for i in range(len(keys)):
                out[keys[i].tobytes()] = (si, i)
        return out
    l0, l1 = set(latest(T0, True).values()), set(latest(T1, False).values())
    return sorted(l1 - l0), sorted(l0 - l1)


def rowlog_delta(log, T0, T1, dst_fields, prefix=None, keep_zero=False):
    """delta_truth over a RowLog."""
    plus, minus = rowlog_sets(log, T0, T1)
    ids = plus + minus
    if not ids:
        return [], 0
    K = sum(SIZE[f] for f in log.fields)
    keys = np.stack([log.snaps[si][1][i] for si, i in ids]).reshape(len(ids), K)
    col = lambda j, dt: np.array([log.snaps[si][j][i] for si, i in ids], dt)
    return group_signed(project(keys, log.fields, dst_fields, prefix), col(2, np.int64), col(3, np.int64),
                        col(4, np.uint64), col(5, np.uint64), len(plus), keep_zero), len(ids)


def movers_truth(rows, metric: int, direction: int = 0, threshold: int = 1, limit: int = 0):
    """[(key, signed change)] of delta rows: change != 0, sign as ``direction``, |change| >=
    max(threshold, 1), ordered by (-|change|, key), cut to ``limit`` when it is not 0."""
    out = []
    for r in rows:
        v = signed(r[4] if metric else r[3])
        if r[3] == 0 or v == 0 or abs(v) < max(threshold, 1):
            continue
        if direction and (v < 0) != (direction < 0):
            continue
        out.append((r[0], v))
    out.sort(key=lambda r: (-abs(r[1]), r[0]))
    return out[:limit] if limit else out
