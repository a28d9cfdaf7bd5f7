"""The store behind QueryHeavyHitters' EndTime for the sketch tasks (gns_hh_hist_*).

Reference: internal/query/querier.go:191-248 reads the ``heavy_hitters`` table that the sketch
writer fills (internal/engine/impl/sketch/writer_clickhouse.go:86-138): one row (Timestamp,
TaskName, Flow, Value, Type) per list entry of each interval's Snapshot(), Type 0 = Count-Min's
count list, 1 = its size list, 2 = SuperSpread's list.  The query keeps, per Flow, the value of
the latest row with ``Timestamp <= EndTime`` and orders by it.
"""
from __future__ import annotations

import ctypes as ct
from typing import Dict, List

import numpy as np

from . import _lib
from ._lib import check

TYPE_COUNT, TYPE_SIZE, TYPE_SPREAD = 0, 1, 2  # writer_clickhouse.go:95-135


def _int64_ns(what: str, t) -> int:
    t = int(t)
    if not -(1 << 63) <= t < (1 << 63):
        raise ValueError(f"{what} {t} is not an int64 of nanoseconds")
    return t


def _check_type(type) -> int:
    if isinstance(type, bool) or int(type) != type or not 0 <= int(type) <= 255:
        raise ValueError(f"type {type!r}: the reference's Type column is a UInt8 (0..255)")
    return int(type)


def _unsigned(what: str, v) -> int:
    v = int(v)
    if v < 0 or v >= (1 << 64):
        raise ValueError(f"{what} {v} is not an unsigned 64-bit number")
    return v


def pack_rows(flows, values, key_bytes: int) -> np.ndarray:
    """Host (flows [n, K], values [n]) -> packed rows uint8 [n, K + 4] ([flow | u32 LE value])."""
    values = np.ascontiguousarray(values)
    n = int(values.shape[0])
    if n and (values.min() < 0 or values.max() > 0xFFFFFFFF):
        raise ValueError("values are u32 in the log, as every producer emits them")
    flows = np.ascontiguousarray(flows, np.uint8).reshape(n, -1) if n else np.zeros((0, key_bytes), np.uint8)
    if n and flows.shape[1] != key_bytes:
        raise ValueError(f"flows must be [n, {key_bytes}]")
    rows = np.empty((n, key_bytes + 4), np.uint8)
    rows[:, :key_bytes] = flows
    rows[:, key_bytes:] = values.astype("<u4").reshape(n, 1).view(np.uint8)
    return rows


class HeavyHistory:
    """A device-resident history of one task's heavy-hitter lists, append-only but for ``trim``.  ``append`` is
    one snapshot under a strictly increasing timestamp (ns, signed): a dict type -> list, at most
    one list per type.  ``heavy_hitters(type, ..., end_time=T)`` answers as of the newest
    snapshot at or before T (``None``: the newest): per flow the value of its latest row of that
    type stored by then.  There are no tombstones -- a flow that left the list keeps its last
    listed value, and a flow listed again supersedes its old row even with a smaller value
    (after the sketch's reset) -- exactly as the reference's argMax(Value, Timestamp)."""

    def __init__(self, key_bytes: int, max_rows: int = 0, max_flows: int = 0, device: int = 0):
        if not 1 <= int(key_bytes) <= 37:
            raise ValueError(f"key_bytes {key_bytes}: 1..37")
        if max_rows < 0 or max_flows < 0:
            raise ValueError("max_rows and max_flows are unsigned (initial capacities; both grow)")
        self._L = _lib.load()
        self.key_bytes, self.device = int(key_bytes), device
        p = _lib.HhHistParams()
        p.key_bytes, p.max_rows, p.max_flows, p.device = self.key_bytes, max_rows, max_flows, device
        h = ct.c_void_p()
        check(self._L.gns_hh_hist_create(ct.byref(p), ct.byref(h)))
        self._h = h
        self._hint: Dict[int, int] = {}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.gns_hh_hist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- append ---
    def _lists(self, lists):
        """The checked arguments of an append, before any device call: (HhList array, where,
        the arrays the pointers name)."""
        W = self.key_bytes + 4
        items, keep, dev = [], [], []
        for type, rows in dict(lists).items():
            type = _check_type(type)
            if isinstance(rows, (tuple, list)) and len(rows) == 2 and not _lib.is_device(rows):
                rows = pack_rows(rows[0], rows[1], self.key_bytes)
            if _lib.is_device(rows):
                import torch
                if rows.dtype != torch.uint8:
                    raise TypeError(f"device rows must be uint8, not {rows.dtype}")
                if rows.dim() != 2 or int(rows.shape[1]) != W:
                    raise ValueError(f"rows of type {type} must be [n, {W}] (key_bytes + 4)")
                if rows.device.index != self.device:
                    raise ValueError(f"rows of type {type} are on device {rows.device.index}, the history on {self.device}")
                rows = rows.contiguous()
                dev.append(True)
                ptr = rows.data_ptr()
            else:
                rows = np.ascontiguousarray(rows, np.uint8)
                if rows.ndim != 2 or rows.shape[1] != W:
                    raise ValueError(f"rows of type {type} must be [n, {W}] (key_bytes + 4)")
                dev.append(False)
                ptr = rows.ctypes.data
            n = int(rows.shape[0])
            items.append((type, ptr if n else None, n))
            keep.append(rows)
        if any(dev) and not all(dev):
            raise ValueError("mix of host and device rows in one append")
        arr = (_lib.HhList * max(len(items), 1))()
        for i, (type, ptr, n) in enumerate(items):
            arr[i].type, arr[i].rows, arr[i].n = type, ptr, n
        return arr, len(items), (_lib.MEM_DEVICE if dev and all(dev) else _lib.MEM_HOST), keep

    def append(self, timestamp_ns: int, lists):
        """One snapshot: ``lists`` maps type -> a device uint8 [n, K + 4] tensor of packed rows
        (CountMin.heavy_hitters_rows_device and the views' give them) or host
        ``(flows [n, K], values [n])`` arrays (a packed host uint8 [n, K + 4] array is taken
        too).  Returns (rows appended, (type, flow) pairs new to the history).  A rejected
        append (GnsError) leaves every answer unchanged."""
        t = _int64_ns("timestamp_ns", timestamp_ns)
        arr, n, where, keep = self._lists(lists)
        if where == _lib.MEM_DEVICE:
            _lib.device_ready(*keep)
        out = (ct.c_uint64 * 2)()
        check(self._L.gns_hh_hist_append(self._h, t, arr, n, where, out))
        del keep
        return int(out[0]), int(out[1])

    # --- queries ---
    @staticmethod
    def _query_args(type, threshold, limit, end_time):
        type = _check_type(type)
        if int(limit) < 0:
            raise ValueError("negative limit")
        threshold, limit = _unsigned("threshold", threshold), _unsigned("limit", limit)
        if end_time is None:
            return type, threshold, limit, None, None
        c = ct.c_int64(_int64_ns("end_time", end_time))
        return type, threshold, limit, c, ct.byref(c)

    def heavy_hitters(self, type: int, threshold: int = 0, limit: int = 0, end_time=None):
        """(flows uint8 [n, K], values uint64 [n]): the flows whose latest row of ``type`` as of
        ``end_time`` has value >= threshold, value descending then flow bytes ascending, cut
        to ``limit`` rows when limit != 0."""
        type, threshold, limit, keep, end = self._query_args(type, threshold, limit, end_time)
        K = self.key_bytes
        cap = max(self._hint.get(type, 0), 1) if limit == 0 else max(min(limit, 1 << 20), 1)
        while True:
            flows, vals = np.empty((cap, K), np.uint8), np.empty(cap, np.uint64)
            n = ct.c_uint64(cap)
            check(self._L.gns_hh_hist_heavy_hitters(self._h, end, type, threshold, limit, flows.ctypes.data,
                                                    vals.ctypes.data, ct.byref(n)))
            if n.value <= cap:
                if limit == 0:
                    self._hint[type] = 2 * n.value + 64
                return flows[: n.value], vals[: n.value]
            cap = n.value

    def heavy_hitters_rows_device(self, type: int, threshold: int = 0, limit: int = 0, end_time=None):
        """The same list as one DEVICE tensor of packed rows uint8 [n, K + 4] in canonical
        order, e.g. for gns_hh_order_rows after an all-gather of flow-disjoint histories."""
        import torch
        type, threshold, limit, keep, end = self._query_args(type, threshold, limit, end_time)
        dev, W = torch.device("cuda", self.device), self.key_bytes + 4
        n = ct.c_uint64(0)
        check(self._L.gns_hh_hist_heavy_rows(self._h, end, type, threshold, limit, None, ct.byref(n)))
        while True:
            rows = torch.empty((max(n.value, 1), W), dtype=torch.uint8, device=dev)
            n2 = ct.c_uint64(rows.shape[0])
            check(self._L.gns_hh_hist_heavy_rows(self._h, end, type, threshold, limit, rows.data_ptr(), ct.byref(n2)))
            if n2.value <= rows.shape[0]:
                return rows[: n2.value]
            n = n2  # (another thread appended between the calls)

    def times(self) -> List[int]:
        n = ct.c_uint64(0)
        check(self._L.gns_hh_hist_times(self._h, None, ct.byref(n)))
        ts = np.zeros(max(n.value, 1), np.int64)
        n2 = ct.c_uint64(n.value)
        check(self._L.gns_hh_hist_times(self._h, ts.ctypes.data, ct.byref(n2)))
        return [int(t) for t in ts[:min(n.value, n2.value)]]

    STATS = ["snapshots", "rows", "keys", "lanes", "row_capacity", "index_slots", "index_growths", "log_growths"]

    def stats(self) -> dict:
        """snapshots, rows, keys (distinct (type, flow) pairs), lanes, row_capacity, index_slots,
        index_growths, log_growths."""
        s = (ct.c_uint64 * 8)()
        check(self._L.gns_hh_hist_stats(self._h, s))
        return {k: int(s[i]) for i, k in enumerate(self.STATS)}

    # --- per-flow queries as of T (gns_hh_hist_query) ---
    def _end(self, end_time):
        if end_time is None:
            return None, None
        c = ct.c_int64(_int64_ns("end_time", end_time))
        return c, ct.byref(c)

    def query(self, type: int, flows, end_time=None):
        """(values uint64 [n], found bool [n]): for each of the host ``flows`` (uint8 [n, K], or n
        bytes objects of K bytes) the value of its latest row of ``type`` as of ``end_time``,
        the sketch-side counterpart of trace_flow(..., end_time=T).  ``found`` is False, and the
        value 0, for a flow without such a row: never listed, listed only later, forgotten by a
        drop.  Duplicates are each answered; nothing is inserted."""
        type, K = _check_type(type), self.key_bytes
        if isinstance(flows, (list, tuple)) and flows and isinstance(flows[0], (bytes, bytearray)):
            if any(len(f) != K for f in flows):
                raise ValueError(f"flows must be {K} bytes each")
            flows = np.frombuffer(b"".join(bytes(f) for f in flows), np.uint8).reshape(-1, K)
        flows = np.ascontiguousarray(flows, np.uint8)
        if flows.size == 0:
            flows = flows.reshape(0, K)
        if flows.ndim != 2 or flows.shape[1] != K:
            raise ValueError(f"flows must be [n, {K}]")
        keep, end = self._end(end_time)
        n = int(flows.shape[0])
        values, found = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
        if n:
            check(self._L.gns_hh_hist_query(self._h, end, type, flows.ctypes.data, n, _lib.MEM_HOST,
                                            values.ctypes.data, found.ctypes.data))
        return values, found.astype(bool)

    def query_device(self, type: int, flows, end_time=None):
        """``query`` for a DEVICE uint8 tensor [n, K] on the history's GPU: (values, found) as
        device tensors, int64 [n] holding the uint64 answers and bool [n]; no host copy either way."""
        import torch
        type, K = _check_type(type), self.key_bytes
        if not _lib.is_device(flows):
            raise TypeError("query_device takes a device tensor (query takes host flows)")
        if flows.dtype != torch.uint8:
            raise TypeError(f"device flows must be uint8, not {flows.dtype}")
        if flows.dim() != 2 or int(flows.shape[1]) != K:
            raise ValueError(f"flows must be [n, {K}]")
        if flows.device.index != self.device:
            raise ValueError(f"flows are on device {flows.device.index}, the history on {self.device}")
        keep, end = self._end(end_time)
        n = int(flows.shape[0])
        values = torch.zeros((n,), dtype=torch.int64, device=flows.device)
        found = torch.zeros((n,), dtype=torch.uint8, device=flows.device)
        if n:
            flows = flows.contiguous()
            _lib.device_ready(flows, values, found)
            check(self._L.gns_hh_hist_query(self._h, end, type, flows.data_ptr(), n, _lib.MEM_DEVICE,
                                            values.data_ptr(), found.data_ptr()))
        return values, found.bool()

    # --- retention (gns_hh_hist_trim) ---
    TRIM = ["snapshots_removed", "rows_removed", "pairs_forgotten", "rows"]

    def trim(self, before_ns, fold: bool = False) -> dict:
        """Expire the snapshots with timestamp < ``before_ns``.  ``fold=False`` drops them with all
        their rows, as the reference drops a partition of its table: a (type, flow) pair listed
        only in them is forgotten, and the key index shrinks to the keys that are left.
        ``fold=True`` keeps of them, per type, each flow's latest row as one base snapshot under
        the last expired timestamp: every answer at or after it is unchanged, earlier end times
        answer empty.  A fold keeps one row per pair ever listed (the store has no tombstones)
        and never shrinks the index; only a drop bounds both.  Returns snapshots_removed,
        rows_removed, pairs_forgotten and the rows now held.  The kept rows move into new,
        smaller logs: the memory is returned."""
        if not isinstance(fold, (bool, np.bool_)) and fold not in (0, 1):
            raise ValueError(f"fold {fold!r}: False (drop) or True (fold)")
        before, out = _int64_ns("before_ns", before_ns), (ct.c_uint64 * 4)()
        check(self._L.gns_hh_hist_trim(self._h, before, int(bool(fold)), out))
        self._hint.clear()
        return {k: int(out[i]) for i, k in enumerate(self.TRIM)}

    def clear(self) -> dict:
        """Forget every snapshot: ``trim`` past the last timestamp with ``fold=False``.  The lanes
        stay; timestamps may start anew afterwards."""
        ts = self.times()
        if ts and ts[-1] == (1 << 63) - 1:
            raise ValueError("clear: no int64 lies past the last snapshot's timestamp")
        return self.trim(ts[-1] + 1 if ts else 0, fold=False)

    # --- the log as data ---
    def export_log(self):
        """(types uint8 [m], flows uint8 [m, K], values uint32 [m], written uint32 [m], times
        int64 [snapshots]): every log row in (type, log order), ``written[i]`` the number of the
        snapshot that stored row i."""
        L, K = self._L, self.key_bytes
        while True:
            ts = np.asarray(self.times(), np.int64)
            n = ct.c_uint64(0)
            check(L.gns_hh_hist_export(self._h, None, None, None, None, ct.byref(n)))
            m = n.value
            ty, fl = np.zeros(max(m, 1), np.uint8), np.zeros((max(m, 1), K), np.uint8)
            va, wr = np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32)
            n2 = ct.c_uint64(m)
            check(L.gns_hh_hist_export(self._h, ty.ctypes.data, fl.ctypes.data, va.ctypes.data, wr.ctypes.data,
                                       ct.byref(n2)))
            # (another thread appended between the calls: take the log again)
            if n2.value == m and self.times() == ts.tolist():
                return ty[:m], fl[:m], va[:m], wr[:m], ts

    def save(self, path) -> None:
        """The whole log as one .npz file."""
        ty, fl, va, wr, ts = self.export_log()
        with open(path, "wb") as f:
            np.savez(f, kind=np.array("heavy_history"), key_bytes=np.array(self.key_bytes, np.uint32),
                     types=ty, flows=fl, values=va, written=wr, times=ts)

    def restore(self, path) -> None:
        """Feed a saved log back, snapshot by snapshot, as host lists.  The history must be
        empty (``clear`` makes it so).  A trimmed history's file holds its base snapshot as an
        ordinary one."""
        with np.load(path, allow_pickle=False) as z:
            if str(z["kind"]) != "heavy_history":
                raise ValueError(f"{path}: not a heavy-history file")
            if int(z["key_bytes"]) != self.key_bytes:
                raise ValueError(f"{path}: saved with {int(z['key_bytes'])}-byte flows, this history has {self.key_bytes}")
            ty, fl, va, wr, ts = z["types"], z["flows"], z["values"], z["written"], z["times"]
        if self.times():
            raise ValueError("restore: the history is not empty")
        K = self.key_bytes
        fl = fl.reshape(-1, K)
        order = np.argsort(wr, kind="stable")  # by snapshot; (type, log order) within one
        bounds = np.searchsorted(wr[order], np.arange(len(ts) + 1))
        for s, t in enumerate(ts.tolist()):
            idx = order[bounds[s]:bounds[s + 1]]
            lists = {}
            for type in np.unique(ty[idx]).tolist():
                sel = idx[ty[idx] == type]
                lists[int(type)] = pack_rows(fl[sel], va[sel], K)
            self.append(t, lists)
