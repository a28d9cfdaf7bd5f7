"""Truth side of the exact history tests: the reference's SQL over stored snapshot rows.

The reference's writer stores every flow of a task under one Timestamp per interval
(manager.go:139-159) and the Querier filters `Timestamp <= ?` (querier.go:211-213, 271-273,
344-346).  AggregateFlows and QueryHeavyHitters then take argMax(..., Timestamp) per flow and
sum / order those latest rows; TraceFlow takes min(StartTime), max(EndTime), max(PacketCount),
max(ByteCount) over ALL the filtered rows.  This module is that, over a list of
(timestamp, key, start, end, packets, bytes) rows filled from oracle.Exact(fields).export() at
each snapshot point (a fresh oracle object after a reset).  Columns are compared as the
strings the reference stores (go_value); a CIDR is compared on the address bytes.  Nothing
here comes from the engine.
"""
from __future__ import annotations

import ipaddress

import numpy as np

from exact_query_truth import go_value, key_bytes_of, truth_rows

IP_FIELDS = ("SrcIP", "DstIP")


def _to16(ip) -> bytes:
    a = ipaddress.ip_address(ip)
    return (bytes(10) + b"\xff\xff" + a.packed) if a.version == 4 else a.packed


def parse_prefix(value):
    """(16 address bytes, leading bits that must match) of "a.b.c.d/len" / "x::/len": an IPv4
    prefix counts behind the 96 bits of ::ffff:0:0/96, as the stored 16-byte form has it."""
    a = ipaddress.ip_interface(value)
    return _to16(str(a.ip)), a.network.prefixlen + (96 if a.version == 4 else 0)


def is_prefix(field, value) -> bool:
    return field in IP_FIELDS and isinstance(value, str) and "/" in value


class HistoryTruth:
    def __init__(self, fields):
        self.fields = list(fields)
        self.ts, self.key, self.start, self.end, self.pkts, self.bytes = [], [], [], [], [], []
        self.parts = []
        self._np, self._memo = None, {}

    def record(self, timestamp: int, export: dict) -> None:
        """One snapshot: every flow of the export stored under ``timestamp``."""
        assert not self.ts or timestamp > self.ts[-1]
        for parts, st, en, pk, by, k in truth_rows(export, self.fields):
            self.ts.append(timestamp)
            self.key.append(k)
            self.parts.append(parts)
            self.start.append(st); self.end.append(en); self.pkts.append(pk); self.bytes.append(by)
        self._np, self._memo = None, {}

    # the stored rows as columns, built once per change
    def cols(self):
        if self._np is None:
            n = len(self.ts)
            ids = {}
            kid = np.array([ids.setdefault(k, len(ids)) for k in self.key], np.int64).reshape(n)
            kb = [key_bytes_of(k, self.fields) for k in self.key]
            ip = {}
            for f in self.fields:
                if f in IP_FIELDS:
                    ip[f] = np.frombuffer(b"".join(_to16(p[f]) for p in self.parts), np.uint8).reshape(n, 16)
            self._np = dict(
                ts=np.array(self.ts, np.int64).reshape(n), kid=kid, kb=kb, ip=ip,
                col={f: np.array([p[f] for p in self.parts], dtype=object).reshape(n) for f in self.fields},
                start=np.array(self.start, np.int64).reshape(n), end=np.array(self.end, np.int64).reshape(n),
                pkts=np.array(self.pkts, np.uint64).reshape(n), bytes=np.array(self.bytes, np.uint64).reshape(n))
        return self._np

    def seen(self, T) -> np.ndarray:
        """Indices of the rows with Timestamp <= T (None: every row), in stored order."""
        if ("seen", T) not in self._memo:
            c = self.cols()
            self._memo["seen", T] = np.arange(len(c["ts"])) if T is None else np.nonzero(c["ts"] <= T)[0]
        return self._memo["seen", T]

    def latest(self, T) -> np.ndarray:
        """argMax(..., Timestamp) per key among the seen rows: indices, in stored order."""
        if ("latest", T) not in self._memo:
            c = self.cols()
            idx = self.seen(T)
            if len(idx):
                rev = idx[::-1]  # rows are stored in timestamp order: the first of a key from the end is its latest
                _, first = np.unique(c["kid"][rev], return_index=True)
                idx = np.sort(rev[first])
            self._memo["latest", T] = idx
        return self._memo["latest", T]

    def matches(self, flt: dict) -> np.ndarray:
        """Row mask of a filter {field: value}; an IP value with "/len" is a prefix.  A field that
        is not a column of this layout is NULL in the store: `NULL = ?` selects nothing."""
        c = self.cols()
        n = len(c["ts"])
        if any(f not in self.fields for f in flt):
            return np.zeros(n, bool)
        m = np.ones(n, bool)
        for f, v in flt.items():
            if is_prefix(f, v):
                addr, bits = parse_prefix(v)
                full, rest = divmod(bits, 8)
                a = np.frombuffer(addr, np.uint8)
                ipb = c["ip"][f]
                if full:
                    m &= (ipb[:, :full] == a[:full]).all(1)
                if rest:
                    mask = (0xFF00 >> rest) & 0xFF
                    m &= (ipb[:, full] & mask) == (a[full] & mask)
            else:
                m &= c["col"][f] == go_value(f, v)
        return m

    def summary(self, flt: dict, T, match=None):
        from go2netspectra_amd import Summary
        c = self.cols()
        m = self.matches(flt) if match is None else match
        seen = self.seen(T)
        seen = seen[m[seen]]
        if len(seen) == 0:
            return Summary()
        live = self.latest(T)
        live = live[m[live]]
        return Summary(len(live), int(c["pkts"][live].sum(dtype=np.uint64)), int(c["bytes"][live].sum(dtype=np.uint64)),
                       int(c["start"][seen].min()), int(c["end"][seen].max()),
                       int(c["pkts"][seen].max()), int(c["bytes"][seen].max()))

    def export_at(self, T) -> dict:
        """key string -> (start, end, packets, bytes) of the latest rows as of T."""
        return {self.key[i]: (self.start[i], self.end[i], self.pkts[i], self.bytes[i]) for i in self.latest(T)}

    def heavy(self, metric: int, threshold: int, limit: int, T):
        c = self.cols()
        rows = [(c["kb"][i], self.bytes[i] if metric else self.pkts[i]) for i in self.latest(T)]
        rows = sorted((r for r in rows if r[1] >= threshold), key=lambda r: (-r[1], r[0]))
        return rows[:limit] if limit else rows

    def rows_at(self, T) -> set:
        c = self.cols()
        return {(c["kb"][i], self.start[i], self.end[i], self.pkts[i], self.bytes[i]) for i in self.latest(T)}
