"""sketch.Task mirror: the aggregator plugin the Manager drives.

Reference: internal/engine/impl/sketch/task.go (New :106-138, ProcessPacket
:156-169, Query :172, Snapshot :177, Reset :182, AlerterMsg :187-243, EncodeFlow
:279-300, DecodeFlow :303-325, fieldByteSize :327-338) behind model.Task
(internal/model/task.go:6-15).

GPU-first differences, by design:
  * process_packets(batch) is the hot entry point: one call per packet batch
    instead of one per packet from N worker goroutines.  process_packet(info)
    is kept for API parity and forwards a batch of one.
  * Row seeds (and SuperSpread's HLL seeds / RNG key) are injected so results
    are reproducible; the reference draws them from unseedable global RNGs.
"""
from __future__ import annotations

import ipaddress
import logging
import struct
from typing import List, Optional, Sequence

import numpy as np

from .config import SketchTaskDef
from .packets import CompactBatch, HeaderBatch, PacketBatch
from .sketch import CountMin, HeavyRecord, SuperSpread

log = logging.getLogger("go2netspectra_amd")

FIELD_SIZE = {"SrcIP": 16, "DstIP": 16, "SrcPort": 2, "DstPort": 2, "Protocol": 1}


def field_byte_size(f: str) -> int:  # task.go:327-338
    return FIELD_SIZE.get(f, 0)


def go_ip_string(b: bytes) -> str:
    """net.IP(b).String() for a 16-byte slot (Go prints IPv4-mapped as dotted quad)."""
    b = bytes(b)
    if len(b) == 16 and b[:10] == bytes(10) and b[10:12] == b"\xff\xff":
        return str(ipaddress.IPv4Address(b[12:]))
    if len(b) == 4:
        return str(ipaddress.IPv4Address(b))
    return ipaddress.IPv6Address(b).compressed


def decode_flow(flow: bytes, fields: Sequence[str]) -> str:
    """DecodeFlow (task.go:303-325)."""
    parts, off = [], 0
    for f in fields:
        if f in ("SrcIP", "DstIP"):
            parts.append(go_ip_string(flow[off:off + 16]))
            off += 16
        elif f in ("SrcPort", "DstPort"):
            parts.append(str(struct.unpack(">H", flow[off:off + 2])[0]))
            off += 2
        elif f == "Protocol":
            parts.append(str(flow[off]))
            off += 1
    return " ".join(parts)


def _check(value: float, threshold: float, op: str) -> bool:  # task.go:246-262
    if op == ">":
        return value > threshold
    if op == "<":
        return value < threshold
    if op == "=":
        return value == threshold
    if op == ">=":
        return value >= threshold
    if op == "<=":
        return value <= threshold
    log.warning("unknown operator '%s' in alerter rule", op)
    return False


def encode_flow(text: str, fields: Sequence[str]) -> bytes:
    """The key bytes ``decode_flow`` prints as ``text``: its inverse on a fixed field layout."""
    parts = text.split(" ")
    if len(parts) != len(fields):
        raise ValueError(f"flow {text!r}: {len(fields)} fields expected ({' '.join(fields)})")
    out = b""
    for f, p in zip(fields, parts):
        if f in ("SrcIP", "DstIP"):
            ip = ipaddress.ip_address(p)
            out += bytes(10) + b"\xff\xff" + ip.packed if ip.version == 4 else ip.packed
        elif f in ("SrcPort", "DstPort"):
            out += struct.pack(">H", int(p))
        elif f == "Protocol":
            out += bytes([int(p)])
    return out


class SketchTask:
    """model.Task implementation for skt_type 0 (CountMin) and 1 (SuperSpread)."""

    def __init__(self, cfg: SketchTaskDef, device: int = 0, seeds=None, max_flows: int = 0,
                 batch_packets: int = 0, hll_master: Optional[int] = None,
                 rng_seed: Optional[int] = None):
        self.name_ = cfg.Name
        self.flow_fields = list(cfg.FlowFields)
        self.element_fields = list(cfg.ElementFields)
        self.flow_size = sum(field_byte_size(f) for f in self.flow_fields)
        self.elem_size = sum(field_byte_size(f) for f in self.element_fields)
        if cfg.SketchType == 0:
            self.sketch = CountMin(cfg.Width, cfg.Depth, cfg.SizeThreshold, cfg.CountThreshold,
                                   flow_fields=self.flow_fields, seeds=seeds, max_flows=max_flows,
                                   batch_packets=batch_packets, device=device)
        elif cfg.SketchType == 1:
            kw = {}
            if hll_master is not None:
                kw["hll_master"] = hll_master
            if rng_seed is not None:
                kw["rng_seed"] = rng_seed
            self.sketch = SuperSpread(cfg.Width, cfg.Depth, cfg.CountThreshold, cfg.M, cfg.Size, cfg.Base,
                                      cfg.B, flow_fields=self.flow_fields, elem_fields=self.element_fields,
                                      seeds=seeds, batch_packets=batch_packets, device=device, **kw)
        else:  # task.go:126-127 log.Fatalf
            raise ValueError(f"Unknown sketch type: {cfg.SketchType} for task {cfg.Name}")

    # --- model.Task ---
    def name(self) -> str:
        return self.name_

    def fields(self) -> List[str]:
        return self.flow_fields

    def decode_flow(self, flow: bytes, fields: Sequence[str]) -> str:
        return decode_flow(flow, fields)

    def decode_flow_func(self):
        return self.decode_flow

    def process_packets(self, batch) -> None:
        """Batched ProcessPacket: PacketBatch, HeaderBatch or CompactBatch (or device equivalents)."""
        if isinstance(batch, HeaderBatch):
            self.sketch.insert_headers(batch.hdr, batch.wirelen)
        elif isinstance(batch, CompactBatch):
            self.sketch.insert_compact(batch.rec16, batch.wirelen, batch.side)
        else:
            self.sketch.insert_tuples(batch)

    def process_packet(self, info) -> None:
        """ProcessPacket(*PacketInfo); info = (src, dst, sport, dport, proto, length)."""
        self.process_packets(PacketBatch.from_packets([info]))

    def query(self, flow: bytes) -> int:
        return self.sketch.query(flow)

    def snapshot(self) -> HeavyRecord:
        return self.sketch.heavy_hitters()

    def reset(self) -> None:
        self.sketch.reset()

    def flush(self) -> None:
        self.sketch.flush()

    def save(self, path) -> None:
        """The sketch's whole state as one checkpoint file (checkpoint.save)."""
        from . import checkpoint
        checkpoint.save(self.sketch, path)

    def restore(self, path) -> None:
        """Replace the sketch's state by a checkpoint's (checkpoint.restore)."""
        from . import checkpoint
        checkpoint.restore(self.sketch, path)

    def view(self):
        """A snapshot view of the sketch (CountMinView / SuperSpreadView): refresh it on the
        ingest thread, then hand it to the snapshotter / alerter thread (snapshot_from,
        alerter_msg(rules, view=...), save_from)."""
        return self.sketch.view()

    def snapshot_from(self, view) -> HeavyRecord:
        """Snapshot from a view instead of the live sketch: what snapshot() gave at the view's
        refresh.  May run on another thread while the task keeps ingesting."""
        return view.heavy_hitters()

    def save_from(self, view, path) -> None:
        """save() from a SuperSpreadView refreshed with state=True, or from a CountMinView
        refreshed with detach=True: the checkpoint of the refresh point, written while the
        task keeps ingesting."""
        from . import checkpoint
        checkpoint.save(view, path)

    # --- the history behind QueryHeavyHitters' end_time (gns_hh_hist_*) ---
    def keep_heavy_history(self, retain=None, drop: bool = False, **kw):
        """Attach a HeavyHistory of this task's flow width (``kw``: its max_rows / max_flows) and
        a view of the sketch: ``record_heavy`` then stores an interval's lists, and
        ``query_heavy_hitters`` / ``query_heavy`` answer from it.  Returns the history (the one
        already attached, if any).

        ``retain=N`` (N >= 1; None: keep everything): after each ``record_heavy`` the history is
        trimmed down to the newest N snapshots.  ``drop=False`` folds the older ones into a base
        snapshot (the base counts as one of the N; answers at the kept times are unchanged, and a
        flow that left the lists keeps its last value); ``drop=True`` drops them, as the reference
        drops a partition: the history then answers over the N newest intervals' rows alone, and
        the key index stays bounded too."""
        if retain is not None:
            if isinstance(retain, bool) or int(retain) != retain or retain < 1:
                raise ValueError(f"retain {retain!r}: a number of snapshots >= 1, or None")
            retain = int(retain)
        if not isinstance(drop, bool):
            raise ValueError(f"drop {drop!r}: False (fold) or True (drop)")
        if getattr(self, "heavy_history", None) is None:
            from .heavy_history import HeavyHistory
            self._heavy_retain, self._heavy_drop = retain, drop
            kw.setdefault("device", self.sketch.device)
            self.heavy_history = HeavyHistory(self.flow_size, **kw)
            self._heavy_view = self.sketch.view()
        return self.heavy_history

    def _heavy(self, what: str):
        h = getattr(self, "heavy_history", None)
        if h is None:
            raise ValueError(f"{what}: no heavy history attached (keep_heavy_history first)")
        return h

    def record_heavy(self, timestamp_ns: int, view=None):
        """One interval of the sketch writer (writer_clickhouse.go:86-138): the lists as device
        rows, appended under ``timestamp_ns`` -- types 0 (count) and 1 (size) for Count-Min,
        type 2 for SuperSpread, the writer's branch on ``Size != nil``.  ``view``: a view the
        caller refreshed on the ingest thread (the call may then run on the snapshotter's
        thread while the task ingests); None refreshes a view of the task's own here.  Returns
        (rows appended, (type, flow) pairs new to the history)."""
        h = self._heavy("record_heavy")
        if view is None:
            view = self._heavy_view
            view.refresh()
        rows = view.heavy_hitters_rows_device()
        if isinstance(self.sketch, CountMin):
            out = h.append(timestamp_ns, {0: rows[0], 1: rows[1]})
        else:
            out = h.append(timestamp_ns, {2: rows})
        keep = getattr(self, "_heavy_retain", None)
        if keep is not None:
            ts = h.times()
            if len(ts) > keep:
                if self._heavy_drop:  # the newest keep snapshots stay
                    h.trim(ts[-keep], fold=False)
                else:  # all but the newest keep - 1 fold into the base
                    h.trim(ts[-(keep - 1)] if keep > 1 else ts[-1] + 1, fold=True)
        return out

    def query_heavy(self, flows, type: int, end_time=None):
        """What these flows read at T: per flow the value of its latest row of ``type`` with
        Timestamp <= ``end_time`` (None: no bound) in the attached history, the sketch-side
        counterpart of trace_flow(..., end_time=T).  ``flows``: key bytes as ``query`` takes them,
        or the decoded strings ``query_heavy_hitters`` returns, one or a list; a uint8 [n, K]
        array is taken too.  Returns a list of int, None for a flow without such a row."""
        h = self._heavy("query_heavy")
        one = isinstance(flows, (str, bytes, bytearray))
        if one:
            flows = [flows]
        if isinstance(flows, (list, tuple)):
            flows = [encode_flow(f, self.flow_fields) if isinstance(f, str) else bytes(f) for f in flows]
            if any(len(f) != self.flow_size for f in flows):
                raise ValueError(f"flows must be {self.flow_size} bytes each")
            flows = np.frombuffer(b"".join(flows), np.uint8).reshape(-1, self.flow_size)
        values, found = h.query(type, flows, end_time=end_time)
        out = [int(v) if f else None for v, f in zip(values, found)]
        return out[0] if one else out

    def query_heavy_hitters(self, type: int, limit: int, end_time=None):
        """QueryHeavyHitters (querier.go:191-248) from the attached history: per flow the value
        of its latest row of ``type`` with Timestamp <= ``end_time`` (None: no bound), ORDER BY
        value DESC LIMIT ``limit`` (ties by flow bytes).  LIMIT 0 and a Type without rows select
        nothing, as in the reference."""
        from .exact import HeavyHitter
        h = self._heavy("query_heavy_hitters")
        if limit < 0:
            raise ValueError("negative limit")
        if limit == 0:
            return []
        flows, vals = h.heavy_hitters(type, 0, limit, end_time=end_time)
        return [HeavyHitter(decode_flow(bytes(f), self.flow_fields), int(v)) for f, v in zip(flows, vals)]

    def save_heavy_history(self, path) -> None:
        """The attached heavy history's log as one file (HeavyHistory.save)."""
        self._heavy("save_heavy_history").save(path)

    def restore_heavy_history(self, path) -> None:
        """Feed a saved log into the attached, still empty heavy history (HeavyHistory.restore)."""
        self._heavy("restore_heavy_history").restore(path)

    def alerter_msg(self, rules, view=None) -> str:
        """AlerterMsg (task.go:187-243); rules: dicts with task_name/metric/operator/threshold/name.
        view: evaluate the rules on that view's snapshot instead of the live sketch's."""
        snap = self.snapshot() if view is None else self.snapshot_from(view)
        msgs = []
        for rule in rules:
            if rule.get("task_name") != self.name_:
                continue
            metric, op, thr = rule.get("metric"), rule.get("operator", ">"), float(rule.get("threshold", 0))
            hitters = []
            if metric == "heavy_hitter_count":
                for h in snap.Count:
                    if _check(float(h.Count), thr, op):
                        hitters.append(f"<tr><td><code>{decode_flow(h.Flow, self.flow_fields)}</code></td><td>{h.Count}</td></tr>")
            elif metric == "heavy_hitter_size":
                for h in snap.Size or []:
                    if _check(float(h.Size), thr, op):
                        hitters.append(f"<tr><td><code>{decode_flow(h.Flow, self.flow_fields)}</code></td><td>{h.Size} bytes</td></tr>")
            elif metric == "super_spreader_spread" and snap.Size is None:
                for h in snap.Count:
                    if _check(float(h.Count), thr, op):
                        hitters.append(f"<tr><td><code>{decode_flow(h.Flow, self.flow_fields)}</code></td><td>{h.Count}</td></tr>")
            if hitters:
                table = ("<table border=\"1\" cellpadding=\"5\" cellspacing=\"0\">"
                         "<tr><th>Flow/Source</th><th>Value</th></tr>" + "".join(hitters) + "</table>")
                msgs.append(f"<h3>Alert: {rule.get('name', '')}</h3><ul><li><b>Task:</b> <code>{rule.get('task_name')}</code></li>"
                            f"<li><b>Metric:</b> <code>{metric}</code></li><li><b>Condition:</b> <code>{op} {thr:.2f}</code></li>"
                            f"</ul><p><b>Triggering Items:</b></p>{table}")
        return "<br><hr><br>".join(msgs)

    # Go-style names
    Name = name
    Fields = fields
    DecodeFlow = decode_flow
    DecodeFlowFunc = decode_flow_func
    ProcessPacket = process_packet
    Query = query
    Snapshot = snapshot
    Reset = reset
    AlerterMsg = alerter_msg


def New(cfg: SketchTaskDef, **kw) -> SketchTask:  # task.go:106
    return SketchTask(cfg, **kw)
