"""The truth side of the heavy-hitter history tests: the reference's heavy_hitters table as a
Python list of (timestamp, type, flow string, value) rows -- what the sketch writer appends,
one row per list entry of each interval's Snapshot() (writer_clickhouse.go:86-138) -- and
QueryHeavyHitters' SQL (querier.go:191-248) restated over it:

    SELECT Flow, argMax(Value, Timestamp) AS LatestValue FROM heavy_hitters
    WHERE TaskName = ? AND Type = ? [AND Timestamp <= ?]
    GROUP BY Flow ORDER BY LatestValue DESC LIMIT ?

Nothing here comes from the engine.  Rows group by the DECODED flow string, as the SQL does;
ClickHouse leaves ties unordered, the project's canonical order breaks them by key bytes."""
from go2netspectra_amd.task import decode_flow


class HeavyTruth:
    def __init__(self, flow_fields=None, decode=None):
        """decode: key bytes -> the Flow column's string (default: DecodeFlow of flow_fields)."""
        self.decode = decode or (lambda b: decode_flow(b, flow_fields))
        self.rows = []   # (timestamp, type, flow string, value)
        self.bytes = {}  # flow string -> key bytes (the tie order; DecodeFlow is injective)
        self.times = []
        self._latest = {}  # (type, end_time) -> latest(): the tests ask many limits per time

    def record(self, ts, lists):
        """One snapshot: lists = {type: [(key bytes, value), ...]} (an empty dict registers ts)."""
        assert not self.times or ts > self.times[-1]
        self.times.append(ts)
        self._latest.clear()
        for type, entries in lists.items():
            for key, value in entries:
                key = bytes(key)
                s = self.decode(key)
                assert self.bytes.setdefault(s, key) == key, "decode is not injective"
                self.rows.append((ts, type, s, int(value)))

    def record_cm(self, ts, orc):
        """A Count-Min oracle's lists now: Type 0 the count list, Type 1 the size list."""
        self.record(ts, {0: orc.heavy("count"), 1: orc.heavy("size")})

    def record_ss(self, ts, orc):
        """A SuperSpread oracle's list now: Type 2."""
        self.record(ts, {2: orc.heavy()})

    def latest(self, type, end_time=None):
        """flow string -> argMax(Value, Timestamp) over the rows of `type` with ts <= end_time."""
        if (type, end_time) in self._latest:
            return self._latest[type, end_time]
        best = {}
        for ts, ty, s, v in self.rows:
            if ty != type or (end_time is not None and ts > end_time):
                continue
            if s not in best or ts > best[s][0]:  # (timestamps are distinct per snapshot, one row per flow in each)
                best[s] = (ts, v)
        self._latest[type, end_time] = out = {s: v for s, (ts, v) in best.items()}
        return out

    def query(self, type, limit=0, threshold=0, end_time=None):
        """[(flow string, value)] ordered (-value, key bytes), value >= threshold, cut to limit != 0."""
        rows = [(s, v) for s, v in self.latest(type, end_time).items() if v >= threshold]
        rows.sort(key=lambda r: (-r[1], self.bytes[r[0]]))
        return rows[:limit] if limit else rows

    def query_bytes(self, type, limit=0, threshold=0, end_time=None):
        """query() with the key bytes in place of the string."""
        return [(self.bytes[s], v) for s, v in self.query(type, limit, threshold, end_time)]

    def probe_times(self):
        """Every snapshot time, a time between each two, one before the first, and None."""
        ts = self.times
        out = [ts[0] - 1] if ts else [0]
        for i, t in enumerate(ts):
            out.append(t)
            if i + 1 < len(ts) and ts[i + 1] - t > 1:
                out.append(t + (ts[i + 1] - t) // 2)
        return out + [None]
