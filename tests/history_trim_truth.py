"""Truth side of the history trim tests: what the stored snapshot rows look like after the
reference's store lost its old partitions (drop) or had them folded into one base snapshot.

Everything works on a HistoryTruth's row lists (history_truth.py) and an explicit list of the
snapshot times -- a snapshot without rows has a time and no row -- with nothing from the engine:
  drop  the rows with ts >= times[c], where c snapshots lie before ``before``;
  fold  the rows latest(times[c-1]) restamped times[c-1], followed by the rows with ts > times[c-1].
``delta_truth`` thins a truth that stored the whole table at every snapshot down to the rows a
delta ``record`` stores: those of flows touched in the interval.
"""
from __future__ import annotations

from history_truth import HistoryTruth

COLS = ("ts", "key", "parts", "start", "end", "pkts", "bytes")


class MemoTruth(HistoryTruth):
    """A HistoryTruth that answers a repeated question from memory: one trimmed truth is asked
    the same filters and times by every test case that trims to it.  (record() clears it.)"""

    def record(self, timestamp, export):
        super().record(timestamp, export)
        self._answers = {}

    def _memo_get(self, key, fn):
        memo = self.__dict__.setdefault("_answers", {})
        if memo.get("n") != len(self.ts):  # rows were added by hand
            memo.clear()
            memo["n"] = len(self.ts)
        if key not in memo:
            memo[key] = fn()
        return memo[key]

    def summary(self, flt, T, match=None):
        return self._memo_get(("s", tuple(sorted(flt.items())), T), lambda: HistoryTruth.summary(self, flt, T, match=match))

    def heavy(self, metric, threshold, limit, T):
        full = self._memo_get(("h", metric, T), lambda: HistoryTruth.heavy(self, metric, 0, 0, T))
        rows = [r for r in full if r[1] >= threshold]
        return rows[:limit] if limit else rows

    def rows_at(self, T):
        return self._memo_get(("r", T), lambda: HistoryTruth.rows_at(self, T))


def subset(tr: HistoryTruth, idx, restamp=None) -> HistoryTruth:
    """A truth of the rows ``idx`` of tr, in that order; restamp = (n, t): the first n get time t."""
    out = MemoTruth(tr.fields)
    for name in COLS:
        setattr(out, name, [getattr(tr, name)[i] for i in idx])
    if restamp:
        n, t = restamp
        out.ts[:n] = [t] * n
    return out


def joined(a: HistoryTruth, b: HistoryTruth) -> HistoryTruth:
    """The rows of a followed by those of b (b's times lie after a's)."""
    out = MemoTruth(a.fields)
    for name in COLS:
        setattr(out, name, list(getattr(a, name)) + list(getattr(b, name)))
    return out


def log_model(written, keys, c: int, fold: bool):
    """The kept set on an exported log, with numpy alone: ``written`` the snapshot number of each
    row, ``keys`` [n, K] its key bytes.  Returns (kept mask, the kept rows' new snapshot numbers).
    A row is superseded by the snapshot of the next row with its key; of the rows written
    before snapshot c, drop keeps none and fold those not superseded by snapshot c - 1."""
    import numpy as np
    w = np.asarray(written, np.int64)
    n = len(w)
    if c == 0 or (fold and c == 1):
        return np.ones(n, bool), w.copy()
    sup = np.full(n, 1 << 40, np.int64)
    if n:
        kid = np.unique(np.ascontiguousarray(keys), axis=0, return_inverse=True)[1].ravel()
        order = np.lexsort((np.arange(n), kid))  # by key, then log order
        same = kid[order][1:] == kid[order][:-1]
        sup[order[:-1][same]] = w[order[1:][same]]
    kept = (w >= c) | (fold & (sup > c - 1))
    d = c - 1 if fold else c
    return kept, np.maximum(w[kept], d) - d


def expired(times, before) -> int:
    """c: the snapshots with time < before (times are strictly increasing: a prefix)."""
    return sum(1 for t in times if t < before)


def trimmed_truth(tr: HistoryTruth, times, before, fold):
    """(truth, times) after a trim of the snapshots before ``before``."""
    times = list(times)
    c = expired(times, before)
    if c == 0:
        return subset(tr, range(len(tr.ts))), times
    if not fold:
        if c == len(times):
            return MemoTruth(tr.fields), []
        return subset(tr, [i for i, t in enumerate(tr.ts) if t >= times[c]]), times[c:]
    base = times[c - 1]
    live = [int(i) for i in tr.latest(base)]
    later = [i for i, t in enumerate(tr.ts) if t > base]
    return subset(tr, live + later, restamp=(len(live), base)), [base] + times[c:]


def delta_truth(tr: HistoryTruth, times, reset_after=None) -> HistoryTruth:
    """The rows a delta record stores: a flow's row of snapshot i unless the flow held the very
    same row at snapshot i - 1 (it was not touched in between).  Snapshot ``reset_after`` is the
    first of a new period: all its rows are stored.  Latest rows and min / max are those of tr."""
    times = list(times)
    at = {t: {} for t in times}
    row = lambda i: (tr.start[i], tr.end[i], tr.pkts[i], tr.bytes[i])
    for i, (t, k) in enumerate(zip(tr.ts, tr.key)):
        at[t][k] = row(i)
    keep = []
    for i, (t, k) in enumerate(zip(tr.ts, tr.key)):
        s = times.index(t)
        prev = at[times[s - 1]].get(k) if s > 0 and s != reset_after else None
        if prev != row(i):
            keep.append(i)
    return subset(tr, keep)


def counts(tr: HistoryTruth):
    """(rows, distinct keys) of the stored rows."""
    return len(tr.ts), len(set(tr.key))
