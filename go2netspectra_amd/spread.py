"""Exact distinct-element (spread) aggregator on the GPU: SuperSpread's ground truth.

Reference: the SuperSpread test keeps a map[flow]map[elem]bool of exact distinct
sets (ss_test.go:49-66) and compares the sketch against len(spreadMap[key])
(:86-136).  ExactSpread is that map on the device (csrc/gns_spread.hip, C ABI
gns_exs_*): spread(flow) = the number of distinct element keys inserted together
with the flow key since create / the last reset.

Keys are the EncodeFlow bytes SuperSpread uses for the same field lists
(task.go:265-300; IPv4 = 4 bytes + 12 zero bytes), so a flow key from here is a
key SuperSpread.query_many accepts -- not the exact aggregator's To16 form.  A
flow never seen answers 0 (SuperSpread.Query's minimum is 1,
super_spread.go:238-258).
"""
from __future__ import annotations

import ctypes as ct
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check
from .sketch import HeavyCount, HeavyRecord, _compact_args, _host, _is_device, _ptr, _where


class ExactSpread:
    """One exact spread table (gns_exs handle).  The ingest surface mirrors SuperSpread's."""

    def __init__(self, flow_fields: Optional[Sequence[str]], elem_fields: Optional[Sequence[str]],
                 max_flows: int = 0, max_pairs: int = 0, batch_packets: int = 0, device: int = 0,
                 flow_bytes: Optional[int] = None, elem_bytes: Optional[int] = None):
        """max_flows / max_pairs are initial capacities (both tables grow).  flow_bytes /
        elem_bytes give the key sizes of a handle without field lists (insert_keys only)."""
        self._L = _lib.load()
        self.flow_fields = list(flow_fields or [])
        self.elem_fields = list(elem_fields or [])
        fb = flow_bytes if flow_bytes is not None else _lib.layout_bytes(self.flow_fields)
        eb = elem_bytes if elem_bytes is not None else _lib.layout_bytes(self.elem_fields)
        p = _lib.ExsParams()
        p.flow, p.elem = _lib.Layout.of(self.flow_fields), _lib.Layout.of(self.elem_fields)
        p.flow_bytes, p.elem_bytes = fb, eb
        p.max_flows, p.max_pairs, p.batch_packets, p.device = max_flows, max_pairs, batch_packets, device
        h = ct.c_void_p()
        check(self._L.gns_exs_create(ct.byref(p), ct.byref(h)))
        self._h = h
        self.flow_bytes, self.elem_bytes = fb, eb
        self.device = device
        self._hh_cap = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.gns_exs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _on_device(self, *arrays) -> None:
        """A device tensor must live on the handle's GPU: the engine would read it there."""
        for a in arrays:
            if a is not None and _is_device(a) and a.device.index != self.device:
                raise ValueError(f"tensor on cuda:{a.device.index}, handle on cuda:{self.device}")

    # --- batched inserts ---
    def _rows(self, flows, elems):
        """(flows, elems, flow stride, elem stride, n, where) of key rows, host or device."""
        self._on_device(flows, elems)
        where = _where(flows, elems)
        if where == _lib.MEM_HOST:
            if len(flows) == 0:  # empty batch (numpy cannot infer -1 of a size-0 reshape)
                flows = np.zeros((0, self.flow_bytes), np.uint8)
                elems = np.zeros((0, self.elem_bytes), np.uint8)
            else:
                flows = _host(flows, np.uint8).reshape(len(flows), -1)
                elems = _host(elems, np.uint8).reshape(len(elems), -1)
        n = int(flows.shape[0])
        if int(elems.shape[0]) != n:
            raise ValueError("flows and elems lengths differ")
        fs = int(flows.shape[1]) if n else self.flow_bytes
        es = int(elems.shape[1]) if n else self.elem_bytes
        return flows, elems, fs, es, n, where

    def insert_keys(self, flows, elems) -> None:
        """flows [n, >= flow_bytes], elems [n, >= elem_bytes] uint8 (the leading bytes are the keys)."""
        flows, elems, fs, es, n, where = self._rows(flows, elems)
        check(self._L.gns_exs_insert_keys(self._h, _ptr(flows), fs, _ptr(elems), es, n, where))

    def insert_tuples(self, batch) -> None:
        """Task.ProcessPacket's key encoding for a PacketBatch (host or device arrays)."""
        self._on_device(batch.src16, batch.dst16, batch.sport, batch.dport, batch.proto)
        t, keep, where = batch.c_struct()
        check(self._L.gns_exs_insert_tuples(self._h, ct.byref(t), len(batch), where))
        del keep

    def insert_headers(self, hdr, wirelen) -> None:
        """64-byte header records [n, 64] uint8 + wire lengths [n] uint32, parsed as
        SuperSpread.insert_headers parses them."""
        self._on_device(hdr, wirelen)
        where = _where(hdr, wirelen)
        if where == _lib.MEM_HOST:
            hdr = _host(hdr, np.uint8)
            wirelen = _host(wirelen, np.uint32)
        check(self._L.gns_exs_insert_headers(self._h, _ptr(hdr), _ptr(wirelen), int(wirelen.shape[0]), where))

    def insert_compact(self, rec16, wirelen, side=None) -> None:
        """Compact records, as CountMin.insert_compact takes them: the same stream as
        insert_headers of the 64-byte records they were made from.  wirelen None: the
        16-byte form."""
        self._on_device(rec16, wirelen, side)
        (rec, wl, sd, _), n, ns, where, keep = _compact_args(rec16, wirelen, side)
        check(self._L.gns_spread_insert_compact(self._h, rec, wl, n, sd, ns, where))

    def flush(self) -> None:
        check(self._L.gns_exs_flush(self._h))

    def insert(self, flow: bytes, elem: bytes, size: int = 0) -> None:
        self.insert_keys(np.frombuffer(bytes(flow), np.uint8).reshape(1, -1),
                         np.frombuffer(bytes(elem), np.uint8).reshape(1, -1))

    # --- reads ---
    def query_many(self, flows):
        """Exact spread of n flows (0 = never seen); a device tensor in -> a device int64 tensor out."""
        if _lib.is_device(flows):
            self._on_device(flows)
            return _lib.query_device(self._L.gns_exs_query_device, self._h, flows)
        flows = _host(flows, np.uint8)
        n = flows.shape[0]
        out = np.zeros(n, dtype=np.uint64)
        if n:
            flows = flows.reshape(n, -1)
            check(self._L.gns_exs_query(self._h, flows.ctypes.data, flows.shape[1], n, out.ctypes.data))
        return out

    def query(self, flow: bytes) -> int:
        if len(flow) != self.flow_bytes:
            return 0
        return int(self.query_many(np.frombuffer(bytes(flow), np.uint8).reshape(1, -1))[0])

    def heavy_hitters_arrays(self, threshold: int, capacity: Optional[int] = None):
        """(flows [n, flow_bytes], spreads [n]) with spread >= threshold: spread descending,
        ties by flow bytes ascending.  ``capacity`` makes one call with buffers of that many
        rows and returns (flows, spreads, full length): a longer list is not written."""
        K = self.flow_bytes
        if capacity is not None:
            f = np.zeros((max(capacity, 1), K), np.uint8)
            v = np.zeros(max(capacity, 1), np.uint32)
            n = ct.c_uint64(capacity)
            check(self._L.gns_exs_heavy_hitters(self._h, threshold, f.ctypes.data, v.ctypes.data, ct.byref(n)))
            m = n.value if n.value <= capacity else 0
            return f[:m], v[:m], n.value
        hint = self._hh_cap
        while True:
            cap = max(hint, 1)
            f = np.empty((cap, K), np.uint8)
            v = np.empty(cap, np.uint32)
            n = ct.c_uint64(cap)
            check(self._L.gns_exs_heavy_hitters(self._h, threshold, f.ctypes.data, v.ctypes.data, ct.byref(n)))
            if n.value <= cap:
                self._hh_cap = 2 * n.value + 64
                return f[: n.value], v[: n.value]
            hint = n.value

    def heavy_hitters(self, threshold: int) -> HeavyRecord:
        """The true superspreaders as the HeavyRecord writers see from SuperSpread (Size = None)."""
        f, v = self.heavy_hitters_arrays(threshold)
        return HeavyRecord(Size=None, Count=[HeavyCount(bytes(f[i]), int(v[i])) for i in range(len(v))])

    def snapshot_arrays(self):
        """Every seen flow: (flows [n, flow_bytes] uint8, spreads [n] uint32), unspecified order."""
        n = ct.c_uint64(0)
        check(self._L.gns_exs_snapshot(self._h, None, None, ct.byref(n)))
        m = n.value
        f = np.zeros((max(m, 1), self.flow_bytes), np.uint8)
        v = np.zeros(max(m, 1), np.uint32)
        n2 = ct.c_uint64(m)
        check(self._L.gns_exs_snapshot(self._h, f.ctypes.data, v.ctypes.data, ct.byref(n2)))
        m = min(m, n2.value)
        return f[:m], v[:m]

    def reset(self) -> None:
        """Empties the tables; cursors taken before are refused afterwards."""
        check(self._L.gns_exs_reset(self._h))

    # --- the pair set: export, delta export, union (gns_pairs_*) ---
    def export_pairs(self, since: int = 0, device: bool = False):
        """(flows [n, flow_bytes], elems [n, elem_bytes], cursor): every distinct pair held, or
        with ``since`` (a cursor this handle returned) only the pairs first inserted or merged
        after that point.  numpy arrays, or with ``device`` torch tensors on the handle's GPU.
        Unspecified order, no row twice.  ``cursor`` names the point the export was taken at."""
        n = ct.c_uint64(0)
        check(self._L.gns_pairs_export(self._h, since, None, None, ct.byref(n), None, _lib.MEM_HOST))
        while True:
            cap = n.value
            if device:
                import torch
                dev = torch.device("cuda", self.device)
                f = torch.empty((max(cap, 1), self.flow_bytes), dtype=torch.uint8, device=dev)
                e = torch.empty((max(cap, 1), self.elem_bytes), dtype=torch.uint8, device=dev)
                _lib.device_ready(f, e)
                where = _lib.MEM_DEVICE
            else:
                f = np.zeros((max(cap, 1), self.flow_bytes), np.uint8)
                e = np.zeros((max(cap, 1), self.elem_bytes), np.uint8)
                where = _lib.MEM_HOST
            n = ct.c_uint64(cap)
            cur = ct.c_uint64(0)
            check(self._L.gns_pairs_export(self._h, since, _ptr(f), _ptr(e), ct.byref(n), ct.byref(cur), where))
            if n.value <= cap:  # only another thread's insert between the two calls makes it larger
                return f[: n.value], e[: n.value], int(cur.value)

    def merge_pairs(self, flows, elems) -> None:
        """Union with the given pairs (rows as insert_keys takes them, host or device): not
        traffic, so inserted / records / batches stay; new_pairs rises by the pairs added."""
        flows, elems, fs, es, n, where = self._rows(flows, elems)
        check(self._L.gns_pairs_merge(self._h, _ptr(flows), fs, _ptr(elems), es, n, where))

    def merge_from(self, other: "ExactSpread", since: int = 0) -> int:
        """Union with ``other``'s pairs (those after ``since``, a cursor of ``other``) on the
        device; ``other`` is not modified.  Returns ``other``'s cursor for the next delta."""
        cur = ct.c_uint64(0)
        check(self._L.gns_pairs_merge_from(self._h, other._h, since, ct.byref(cur)))
        return int(cur.value)

    def rollup_from(self, src, since: int = 0, flow_prefix=None, elem_prefix=None):
        """gns_spread_rollup: union with the (flow, element) pairs of the flows an
        ExactAggregator holds, projected onto this handle's layouts on the device and converted
        from its To16 keys to EncodeFlow form.  Into an empty handle the result equals a handle of
        these layouts fed src's packets (an IPv4-mapped arrival counted with its IPv4 address).
        ``since`` (a cursor this call or ``ExactView.refresh`` returned for src) projects only the
        flows first seen after that point; chained into the same handle that keeps it equal to a
        full roll-up.  src is only read.  Returns (src's cursor, flows projected, pairs new here).

        ``flow_prefix`` / ``elem_prefix`` (gns_spread_rollup_prefix; ``ExactAggregator.rollup_from``'s
        ``prefix``) mask the IP fields of the flow row / the element row to their leading bits, on
        the To16 bytes src stores and before the conversion.  Both None: the unmasked entry point."""
        from .exact import ExactAggregator, make_prefix, spread_rollup_plan
        if not isinstance(src, ExactAggregator):
            raise TypeError("rollup_from takes an ExactAggregator")
        if since < 0:
            raise ValueError("since is a stream position (unsigned)")
        spread_rollup_plan(src.key_fields, self.flow_fields, self.elem_fields)
        cur = ct.c_uint64(0)
        out = (ct.c_uint64 * 2)()
        if flow_prefix is None and elem_prefix is None:
            check(self._L.gns_spread_rollup(self._h, src._h, since, ct.byref(cur), out))
        else:
            fpx, epx = make_prefix(flow_prefix), make_prefix(elem_prefix)
            check(self._L.gns_spread_rollup_prefix(self._h, src._h, ct.byref(fpx), ct.byref(epx), since, ct.byref(cur),
                                                   out))
        return int(cur.value), int(out[0]), int(out[1])

    def save(self, path) -> None:
        """The whole pair set into one checkpoint file (checkpoint.save)."""
        from . import checkpoint
        checkpoint.save(self, path)

    def restore(self, path) -> None:
        """Replace the pair set by a file's (checkpoint.restore); the key layout must be equal."""
        from . import checkpoint
        checkpoint.restore(self, path)

    Insert = insert
    Query = query
    Reset = reset

    # --- observability ---
    def counters(self) -> dict:
        s = (ct.c_uint64 * 8)()
        check(self._L.gns_exs_counters(self._h, s))
        names = ["inserted", "dropped", "unsupported", "probe_full", "new_pairs", "flows", "records", "batches"]
        return {k: int(s[i]) for i, k in enumerate(names)}

    def dict_stats(self) -> dict:
        s = (ct.c_uint64 * 8)()
        check(self._L.gns_exs_dict_stats(self._h, s))
        names = ["flow_growths", "pair_growths", "flow_slots", "flows_claimed", "pair_slots", "pairs_claimed",
                 "grow_us"]
        return {k: int(s[i]) for i, k in enumerate(names)}

    STAGES = ["insert", "resolve", "grow", "project", "unused4", "total"]  # project: rollup_from's projection

    def set_timing(self, on: bool = True, stages=None) -> None:
        check(self._L.gns_exs_set_timing(self._h, _lib.timing_arg(on, stages, self.STAGES)))

    def stage_times(self, reset: bool = False) -> dict:
        ms = (ct.c_double * 8)()
        ln = (ct.c_uint64 * 8)()
        check(self._L.gns_exs_stage_times(self._h, ms, ln, 1 if reset else 0))
        return {name: (ms[i], ln[i]) for i, name in enumerate(self.STAGES)}
