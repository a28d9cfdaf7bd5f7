"""Exact aggregator on the GPU: the model.Task of internal/engine/impl/exact.

Reference: exact/task.go -- New (:83-103), ProcessPacket (:124-149), Snapshot
(:153-191), Reset (:194-210), AlerterMsg (:213-282), Query (:298-326),
generateKeyAndFields (:330-366); exact/statistic/flow.go (Flow, Shard,
SnapshotData); internal/query/querier.go (AggregateFlows, TraceFlow,
QueryHeavyHitters: answered from the device table, gns_ex_aggregate /
gns_ex_heavy_hitters).  The device engine (csrc/gns_exact.hip, C ABI gns_ex_*) keys
flows by canonical bytes (IP fields in 16-byte To16 form); the Go key string
and the Fields map are rebuilt here from those bytes for snapshots.
"""
from __future__ import annotations

import ctypes as ct
import ipaddress
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check
from .packets import CompactBatch, HeaderBatch, PacketBatch
from .task import _check, go_ip_string

DEFAULT_SHARDS = 256  # exact/task.go:72


@dataclass
class Flow:  # exact/statistic/flow.go:9-16
    Key: str
    Fields: Dict[str, object]
    StartTime: int  # ns since epoch (time.Time UnixNano)
    EndTime: int
    ByteCount: int
    PacketCount: int


@dataclass
class Shard:
    Flows: Dict[str, Flow] = field(default_factory=dict)


@dataclass
class SnapshotData:
    TaskName: str
    Shards: List[Shard]


@dataclass
class Summary:  # gns_ex_summary: one filter's answer
    flows: int = 0        # COUNT(*)
    packets: int = 0      # SUM(PacketCount) mod 2^64
    bytes: int = 0        # SUM(ByteCount) mod 2^64
    first_ns: int = 0     # min(StartTime), signed; 0 when flows == 0
    last_ns: int = 0      # max(EndTime)
    max_packets: int = 0  # max(PacketCount)
    max_bytes: int = 0    # max(ByteCount)


@dataclass
class Change:  # one filter's totals over a window: summary(T1) - summary(T0), signed
    flows: int = 0
    packets: int = 0  # the difference of the two u64 sums, read as int64
    bytes: int = 0


@dataclass
class TaskSummary:  # query.TaskSummary (querier.go:29-34)
    TaskName: str
    TotalBytes: int
    TotalPackets: int
    FlowCount: int


@dataclass
class FlowLifecycle:  # query.FlowLifecycle (querier.go:49-54); times in ns since the epoch
    FirstSeen: int
    LastSeen: int
    TotalPackets: int
    TotalBytes: int


@dataclass
class HeavyHitter:  # query.HeavyHitter (querier.go:65-68); Flow = the Go key string
    Flow: str
    Value: int


FLOW_KEYS = ("SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol")  # traceFlowKeys, querier.go:94-100
_FIELD_MASK = sum(1 << _lib.FIELD_IDS[f] for f in FLOW_KEYS)


def ip_to16(ip) -> bytes:
    """net.ParseIP(ip).To16(): the form the engine stores (IPv4 as ::ffff:a.b.c.d).
    "1.2.3.4" and "::ffff:1.2.3.4" give the same bytes, as does any spelling of an
    IPv6 address; 4 or 16 raw bytes are taken as a net.IP."""
    if isinstance(ip, (bytes, bytearray, np.ndarray)):
        ip = bytes(ip)
        if len(ip) not in (4, 16):
            raise ValueError(f"an IP of {len(ip)} bytes")
        return (bytes(10) + b"\xff\xff" + ip) if len(ip) == 4 else ip
    a = ipaddress.ip_address(ip)
    return (bytes(10) + b"\xff\xff" + a.packed) if a.version == 4 else a.packed


def to16_to_encodeflow(keys, fields: Sequence[str]) -> np.ndarray:
    """Key rows [n, K] laid out by ``fields`` with IPs in To16 form (this engine's keys) ->
    the same rows in EncodeFlow form (the keys of ExactSpread and SuperSpread), the conversion
    gns_spread_rollup applies: an IP field holding ::ffff:a.b.c.d becomes a.b.c.d + 12 zero
    bytes, every other IP value (genuine IPv6, :: included) and every port / protocol byte is
    copied.  The inverse of ``ip_to16`` on 4-byte addresses."""
    keys = np.ascontiguousarray(keys, np.uint8)
    K = sum(_lib.FIELD_SIZE.get(f, 0) for f in fields)
    keys = keys.reshape(-1, K) if K else keys.reshape(len(keys), 0)
    out = keys.copy()
    off = 0
    for f in fields:
        size = _lib.FIELD_SIZE.get(f, 0)
        if f in ("SrcIP", "DstIP"):
            ip = keys[:, off:off + 16]
            mapped = (ip[:, :10] == 0).all(1) & (ip[:, 10:12] == 0xFF).all(1)
            out[mapped, off:off + 4] = ip[mapped, 12:16]
            out[mapped, off + 4:off + 16] = 0
        off += size
    return out


def _prefix_bits(what: str, v):
    """(IPv4 bits, IPv6 bits) of one field's prefix: None keeps the field whole, a lone int is the
    IPv4 length with IPv6 kept whole, a pair gives both."""
    if v is None:
        return 32, 128
    if isinstance(v, (int, np.integer)):
        v = (v, 128)
    v = tuple(v)
    if len(v) != 2:
        raise ValueError(f"prefix of {what}: an IPv4 length or (IPv4 length, IPv6 length)")
    v4, v6 = int(v[0]), int(v[1])
    if not (0 <= v4 <= 32 and 0 <= v6 <= 128):
        raise ValueError(f"prefix of {what}: ({v4}, {v6}) outside (0..32, 0..128)")
    return v4, v6


def make_prefix(prefix) -> "_lib.Prefix":
    """gns_prefix of ``{"SrcIP": (24, 48), "DstIP": 16}``: per IP field the leading bits kept of an
    IPv4 and of an IPv6 value (``_prefix_bits``); a field left out, and None, keep everything."""
    prefix = dict(prefix or {})
    for k in prefix:
        if k not in ("SrcIP", "DstIP"):
            raise ValueError(f"prefix: {k!r} is not an IP field (SrcIP, DstIP)")
    px = _lib.Prefix()
    px.src_v4, px.src_v6 = _prefix_bits("SrcIP", prefix.get("SrcIP"))
    px.dst_v4, px.dst_v6 = _prefix_bits("DstIP", prefix.get("DstIP"))
    return px


def _prefix_byte(bits: int, b: int) -> int:
    """The mask byte of byte ``b`` of a value whose leading ``bits`` bits are kept."""
    k = min(max(bits - 8 * b, 0), 8)
    return (0xFF00 >> k) & 0xFF


def mask_prefix(keys16, v4_bits: int, v6_bits: int) -> np.ndarray:
    """The mask of gns_ex_rollup_prefix on IP values [n, 16] in To16 form: a value that is IPv4
    (bytes 0..9 zero, bytes 10, 11 ff ff) keeps bytes 0..11 and the leading ``v4_bits`` bits of
    bytes 12..15, every other value keeps its leading ``v6_bits`` bits; the rest are zeroed.  Only
    trailing bits are cleared: no value changes class, the mask is idempotent, and a coarser
    mask over a finer one is the coarser one."""
    v4_bits, v6_bits = _prefix_bits("mask_prefix", (v4_bits, v6_bits))
    keys = np.ascontiguousarray(keys16, np.uint8).reshape(-1, 16)
    m4 = np.array([0xFF] * 12 + [_prefix_byte(v4_bits, b) for b in range(4)], np.uint8)
    m6 = np.array([_prefix_byte(v6_bits, b) for b in range(16)], np.uint8)
    v4 = (keys[:, :10] == 0).all(1) & (keys[:, 10:12] == 0xFF).all(1)
    return keys & np.where(v4[:, None], m4[None, :], m6[None, :])


def mask_keys(keys, fields: Sequence[str], prefix) -> np.ndarray:
    """Key rows [n, K] laid out by ``fields`` (IPs in To16 form) with every IP field masked by
    ``prefix`` (``make_prefix``'s argument): ``mask_prefix`` per field, other bytes copied."""
    px = make_prefix(prefix)
    bits = {"SrcIP": (px.src_v4, px.src_v6), "DstIP": (px.dst_v4, px.dst_v6)}
    K = sum(_lib.FIELD_SIZE.get(f, 0) for f in fields)
    out = np.ascontiguousarray(keys, np.uint8).reshape(-1, K).copy()
    off = 0
    for f in fields:
        if f in bits:
            out[:, off:off + 16] = mask_prefix(out[:, off:off + 16], *bits[f])
        off += _lib.FIELD_SIZE.get(f, 0)
    return out


def prefix_plan(src_fields: Sequence[str], dst_fields: Sequence[str], prefix=None, encodeflow: bool = False):
    """The tables of a masked gather, as gns_ex_rollup_prefix builds them (``encodeflow``: as
    gns_spread_rollup_prefix builds them for one row): per byte j of the key laid out by
    ``dst_fields``, (g, field, m4, m6) -- ``rollup_plan``'s source offset, the IP field the byte
    belongs to (0 SrcIP, 1 DstIP, 2 none), and the mask byte applied when that field's value is
    IPv4 / is not.  Bytes outside IP fields carry 0xff in both.  For a To16 key m4 keeps bytes
    0..11 and counts the prefix in bytes 12..15; for an EncodeFlow row the IPv4 address sits in
    bytes 0..3 and the prefix is counted there."""
    g = rollup_plan(src_fields, dst_fields)
    px = make_prefix(prefix)
    bits = {"SrcIP": (0, px.src_v4, px.src_v6), "DstIP": (1, px.dst_v4, px.dst_v6)}
    field, m4, m6 = [], [], []
    for f in dst_fields:
        size = _lib.FIELD_SIZE.get(f, 0)
        if f not in bits:
            field += [2] * size
            m4 += [0xFF] * size
            m6 += [0xFF] * size
            continue
        i, v4, v6 = bits[f]
        field += [i] * 16
        if encodeflow:
            m4 += [_prefix_byte(v4, b) for b in range(4)] + [0xFF] * 12
        else:
            m4 += [0xFF] * 12 + [_prefix_byte(v4, b) for b in range(4)]
        m6 += [_prefix_byte(v6, b) for b in range(16)]
    return g, field, m4, m6


def spread_rollup_plan(src_fields: Sequence[str], flow_fields: Sequence[str], elem_fields: Sequence[str]):
    """The two byte gathers of a spread roll-up, as gns_spread_rollup builds them: (flow plan,
    element plan), each a ``rollup_plan`` from the key laid out by ``src_fields``.  ValueError
    naming the field when a flow or element field is not part of src, or when either layout
    is empty (a handle made from key sizes alone names no fields): GNS_E_ARG in C."""
    if not list(flow_fields or []) or not list(elem_fields or []):
        raise ValueError("spread rollup: the spread handle has no flow / element field lists (key sizes only)")
    plans = []
    for what, fields in (("flow", flow_fields), ("element", elem_fields)):
        try:
            plans.append(rollup_plan(src_fields, fields))
        except ValueError as e:
            raise ValueError(f"spread {e} ({what} layout)") from None
    return plans[0], plans[1]


def _small_int(name: str, v, hi: int) -> int:
    v = int(v)
    if not 0 <= v <= hi:
        raise ValueError(f"{name} {v} outside 0..{hi}")
    return v


def parse_cidr(ip):
    """(To16 bytes, leading bits of the 16-byte form that must match) of an address or a CIDR
    string: "10.1.0.0/16" -> 96 + 16 bits, "2001:db8::/32" -> 32, an address without a length ->
    128.  The address is kept as written: bits below the prefix are ignored by the filter."""
    if isinstance(ip, str) and "/" in ip:
        a = ipaddress.ip_interface(ip)
        return ip_to16(str(a.ip)), a.network.prefixlen + (96 if a.version == 4 else 0)
    return ip_to16(ip), 128


def make_filter(src_ip=None, dst_ip=None, src_port=None, dst_port=None, protocol=None):
    """gns_ex_filter of an AggregationRequest (querier.go:19-26, :143-170): every field
    given must equal the flow's; None (and "" for an IP, as the reference) leaves it open.
    An IP given as a CIDR string ("10.1.0.0/16", "2001:db8::/32") must match in its prefix only;
    the result is then a gns_ex_cidr (``_lib.ExCidr``), which every call that takes a filter
    accepts too."""
    f = _lib.ExFilter()
    bits = {"SrcIP": 128, "DstIP": 128}
    for name, ip, dst in (("SrcIP", src_ip, f.src16), ("DstIP", dst_ip, f.dst16)):
        if ip is None or (isinstance(ip, str) and ip == ""):
            continue
        b16, bits[name] = parse_cidr(ip)
        dst[:] = list(b16)
        f.mask |= 1 << _lib.FIELD_IDS[name]
    if src_port is not None:
        f.sport = _small_int("SrcPort", src_port, 0xFFFF)
        f.mask |= 1 << _lib.FIELD_IDS["SrcPort"]
    if dst_port is not None:
        f.dport = _small_int("DstPort", dst_port, 0xFFFF)
        f.mask |= 1 << _lib.FIELD_IDS["DstPort"]
    if protocol is not None:
        f.proto = _small_int("Protocol", protocol, 0xFF)
        f.mask |= 1 << _lib.FIELD_IDS["Protocol"]
    if bits["SrcIP"] != 128 or bits["DstIP"] != 128:
        return as_cidr(f, bits["SrcIP"], bits["DstIP"])
    return f


def as_cidr(f, src_bits: int = 128, dst_bits: int = 128) -> "_lib.ExCidr":
    """gns_ex_cidr of a filter: SrcIP / DstIP compared in their leading bits of the 16-byte form
    (an IPv4 /24 is 120; 128 is equality).  An ExCidr is returned as it is."""
    if isinstance(f, _lib.ExCidr):
        return f
    c = _lib.ExCidr()
    ct.memmove(ct.byref(c.f), ct.byref(f), ct.sizeof(_lib.ExFilter))
    c.src_bits, c.dst_bits = _small_int("SrcIP bits", src_bits, 128), _small_int("DstIP bits", dst_bits, 128)
    return c


def _filter_parts(f):
    """(gns_ex_filter, SrcIP bits, DstIP bits) of either kind of filter."""
    if isinstance(f, _lib.ExCidr):
        return f.f, int(f.src_bits), int(f.dst_bits)
    return f, 128, 128


_FLOW_KEY_ARG = {"SrcIP": "src_ip", "DstIP": "dst_ip", "SrcPort": "src_port", "DstPort": "dst_port",
                 "Protocol": "protocol"}


def filter_from_flow_keys(flow_keys):
    """gns_ex_filter of TraceFlowRequest.FlowKeys (appendTraceFlowFilters, querier.go:172-188)."""
    for k in sorted(flow_keys):
        if k not in _FLOW_KEY_ARG:
            raise ValueError(f"unsupported flow key: {k}")
    return make_filter(**{_FLOW_KEY_ARG[k]: v for k, v in flow_keys.items()})


def check_filter(f) -> None:
    f, sb, db = _filter_parts(f)
    if int(f.mask) & ~_FIELD_MASK:
        raise ValueError(f"filter mask {int(f.mask):#x} has bits outside the five key fields")
    if sb > 128 or db > 128:
        raise ValueError(f"filter prefix of {sb} / {db} bits (0..128 of the 16-byte form)")


def filter_fields(f) -> List[str]:
    """Names of the fields a filter constrains."""
    f = _filter_parts(f)[0]
    return [n for n in FLOW_KEYS if int(f.mask) >> _lib.FIELD_IDS[n] & 1]


def filter_key_bytes(f, key_fields: Sequence[str]):
    """(mask, value) uint8 arrays over the canonical key bytes of ``key_fields``: a flow
    matches iff key & mask == value.  None when the filter constrains a field that is not
    part of the key: such a column is NULL in the reference (writer_clickhouse.go:142-148)
    and `NULL = ?` selects nothing."""
    check_filter(f)
    want = set(filter_fields(f))
    if not want <= set(key_fields):
        return None
    f, sb, db = _filter_parts(f)
    bits = {"SrcIP": sb, "DstIP": db}
    vals = {"SrcIP": bytes(f.src16), "DstIP": bytes(f.dst16), "SrcPort": struct.pack(">H", f.sport),
            "DstPort": struct.pack(">H", f.dport), "Protocol": bytes([f.proto])}
    mask, value = bytearray(), bytearray()
    for name in key_fields:
        size = _lib.FIELD_SIZE.get(name, 0)
        m = bytes(_prefix_byte(bits.get(name, 8 * size), b) if name in want else 0 for b in range(size))
        mask += m
        value += bytes(v & k for v, k in zip(vals[name], m))  # address bits below a prefix are ignored
    return np.frombuffer(bytes(mask), np.uint8), np.frombuffer(bytes(value), np.uint8)


def merge_summaries(parts: Sequence[Summary]) -> Summary:
    """One Summary of shards that hold DISJOINT flows (the router's owner-key rule):
    sum, sum, sum (mod 2^64), min, max, max, max.  A shard without matching flows carries
    0 timestamps that are not observations and does not contribute them."""
    out = Summary()
    m64 = (1 << 64) - 1
    for p in parts:
        if p.flows == 0:
            continue
        first = p.first_ns if out.flows == 0 else min(out.first_ns, p.first_ns)
        last = p.last_ns if out.flows == 0 else max(out.last_ns, p.last_ns)
        out = Summary((out.flows + p.flows) & m64, (out.packets + p.packets) & m64, (out.bytes + p.bytes) & m64,
                      first, last, max(out.max_packets, p.max_packets), max(out.max_bytes, p.max_bytes))
    return out


def _no_end_time(end_time) -> None:
    if end_time is not None:
        raise ValueError("end_time is not supported: a live handle holds one point in time, no history of snapshots")


def signed(a):
    """The u64 count columns of a table of changes (``ExactHistory.delta(...).snapshot_arrays()``)
    as the int64 changes they store in two's complement; an int as a Python int."""
    if isinstance(a, (int, np.integer)):
        v = int(a) & ((1 << 64) - 1)
        return v - (1 << 64) if v >> 63 else v
    return np.asarray(a, np.uint64).view(np.int64)


def _ptr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _is_dev(a) -> bool:
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _snapshot_arrays(fn, h, key_bytes: int, retry: bool = False):
    """The two calls of a snapshot export (length, then rows) through gns_ex_snapshot or
    gns_ex_view_snapshot.  retry: a writer on another thread may add rows between the two calls
    (a history's newest snapshot); the rows are then taken again instead of cut at the first
    call's length."""
    while True:
        n = ct.c_uint64(0)
        check(fn(h, None, None, None, None, None, ct.byref(n)))
        m = n.value
        K = max(key_bytes, 1)
        keys = np.zeros((max(m, 1), K), np.uint8)
        st, en = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
        pk, by = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64)
        n2 = ct.c_uint64(m)
        check(fn(h, keys.ctypes.data, st.ctypes.data, en.ctypes.data, pk.ctypes.data, by.ctypes.data, ct.byref(n2)))
        if not retry or n2.value <= m:
            break
    m = min(m, n2.value)
    return keys[:m, :key_bytes], st[:m], en[:m], pk[:m], by[:m]


def _aggregate(fn, fn_cidr, h, filters) -> List[Summary]:
    """One batch through gns_ex[_view]_aggregate, or through its _cidr form when any filter of
    the batch is a gns_ex_cidr (the others enter it with 128 bits: equality)."""
    flt = [f if isinstance(f, (_lib.ExFilter, _lib.ExCidr)) else make_filter(**f) for f in filters]
    for f in flt:
        check_filter(f)
    n = len(flt)
    if n == 0:
        return []
    out = (_lib.ExSummary * n)()
    if any(isinstance(f, _lib.ExCidr) for f in flt):
        check(fn_cidr(h, (_lib.ExCidr * n)(*[as_cidr(f) for f in flt]), n, out))
    else:
        check(fn(h, (_lib.ExFilter * n)(*flt), n, out))
    return [Summary(int(o.flows), int(o.packets), int(o.bytes), int(o.first_ns), int(o.last_ns),
                    int(o.max_packets), int(o.max_bytes)) for o in out]


def _heavy_hitters(fn, h, key_bytes: int, metric: int, threshold: int, limit: int):
    if metric not in (0, 1):
        raise ValueError(f"metric {metric}: 0 (PacketCount) or 1 (ByteCount)")
    if threshold < 0 or limit < 0:
        raise ValueError("threshold and limit are unsigned")
    n = ct.c_uint64(limit if 0 < limit <= 1 << 16 else 0)
    if n.value == 0:  # the list's length first
        check(fn(h, metric, threshold, limit, None, None, ct.byref(n)))
    cap = n.value
    K = max(key_bytes, 1)
    keys, vals = np.zeros((max(cap, 1), K), np.uint8), np.zeros(max(cap, 1), np.uint64)
    if cap:
        check(fn(h, metric, threshold, limit, keys.ctypes.data, vals.ctypes.data, ct.byref(n)))
    m = min(cap, n.value)
    return keys[:m, :key_bytes], vals[:m]


def _movers(fn, h, key_bytes: int, metric: int, direction: int, threshold: int, limit: int):
    if metric not in (0, 1):
        raise ValueError(f"metric {metric}: 0 (PacketCount) or 1 (ByteCount)")
    if direction not in (-1, 0, 1):
        raise ValueError(f"direction {direction}: +1 (increases), -1 (decreases) or 0 (either)")
    if threshold < 0 or limit < 0 or threshold >= 1 << 64 or limit >= 1 << 64:
        raise ValueError("threshold and limit are unsigned 64-bit")
    keys, vals = _heavy_hitters(lambda hh, m, t, l, *a: fn(hh, m, direction, t, l, *a), h, key_bytes, metric, threshold, limit)
    return keys, vals.view(np.int64)


def apply_delta(state: dict, arrays) -> dict:
    """The consumer's rule for delta exports: fold the rows of one ``snapshot_arrays()`` (of a
    full or a delta view) into a map key bytes -> (start, end, packets, bytes) and return the
    new map.  Rows carry cumulative state, so a later row of a key replaces the earlier one
    (the store's argMax(..., Timestamp), querier.go:191-248); an empty delta changes nothing."""
    keys, st, en, pk, by = arrays
    out = dict(state)
    for i in range(len(pk)):
        out[bytes(keys[i])] = (int(st[i]), int(en[i]), int(pk[i]), int(by[i]))
    return out


def check_levels(levels):
    """The levels of hierarchical heavy hitters as a list of (IPv4 bits, IPv6 bits), finest
    first; ValueError unless each level is at most as long as the one before in both classes."""
    levels = [_prefix_bits("level", lv) for lv in levels]
    if not levels:
        raise ValueError("hierarchical heavy hitters: no levels")
    for a, b in zip(levels, levels[1:]):
        if b[0] > a[0] or b[1] > a[1]:
            raise ValueError(f"hierarchical heavy hitters: level {b} is not coarser than {a}")
    return levels


def discount_heavy_prefixes(lists, levels, threshold: int):
    """The host step of hierarchical heavy hitters.  ``lists[l]`` = (keys [n, 16] To16 bytes
    masked to ``levels[l]``, totals [n]) of the prefixes of level l whose total is >= threshold
    (``heavy_hitters`` of the level's table), finest level first.  From finest to coarsest, a
    prefix's conditioned count is its total minus the totals of the reported prefixes below it
    that have no reported prefix strictly between; it is reported iff that is >= threshold.  A
    prefix heavy by its total alone and discounted below the threshold is not reported and
    discounts nothing.  The lists suffice: a conditioned count never exceeds the total, so every
    reported prefix, and with it everything that discounts an ancestor, is in its level's list.
    Returns per level [(key bytes, total, conditioned), ...] in the list's order."""
    levels = check_levels(levels)
    if len(lists) != len(levels):
        raise ValueError("hierarchical heavy hitters: one list per level")
    open_, out = [], []  # open_: [key bytes, total] of reported prefixes no reported ancestor covers yet
    for (keys, totals), lv in zip(lists, levels):
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 16)
        below: Dict[bytes, List[int]] = {}
        if open_:
            up = mask_prefix(np.frombuffer(b"".join(k for k, _ in open_), np.uint8).reshape(-1, 16), *lv)
            for i, row in enumerate(up):
                below.setdefault(row.tobytes(), []).append(i)
        rows, covered = [], set()
        for k, t in zip(keys, totals):
            k, t = k.tobytes(), int(t)
            kids = below.get(k, [])
            cond = t - sum(open_[i][1] for i in kids)
            if cond >= threshold:
                rows.append((k, t, cond))
                covered.update(kids)
        open_ = [o for i, o in enumerate(open_) if i not in covered] + [[k, t] for k, t, _ in rows]
        out.append(rows)
    return out


def rollup_plan(src_fields: Sequence[str], dst_fields: Sequence[str]) -> List[int]:
    """The byte gather of a roll-up, as gns_ex_rollup builds it: for every byte of the key laid
    out by ``dst_fields``, the offset of that byte in the key laid out by ``src_fields`` (a
    field repeated in src is read at its first occurrence, one repeated in dst is copied once
    per occurrence).  ValueError when a field of dst is not part of src: GNS_E_ARG in C."""
    at, off = {}, 0
    for f in src_fields:
        size = _lib.FIELD_SIZE.get(f, 0)  # unknown names contribute no bytes (task.go:335-336)
        if size:
            at.setdefault(f, off)
        off += size
    plan: List[int] = []
    for f in dst_fields:
        size = _lib.FIELD_SIZE.get(f, 0)
        if size == 0:
            continue
        if f not in at:
            raise ValueError(f"rollup: key field {f} is not part of the source's layout")
        plan.extend(range(at[f], at[f] + size))
    return plan


class ExactView:
    """Snapshot view of an ExactAggregator (gns_ex_view_*): a dense copy of the table, or of
    the flows touched since a cursor, taken at a point of the insert stream (``refresh``) and
    exported or queried from any thread while the aggregator keeps ingesting.  The rows stay
    what they were at the refresh whatever the aggregator does afterwards, reset included."""

    def __init__(self, agg: "ExactAggregator"):
        self._L = agg._L
        self._agg = agg  # the handle outlives its views
        self.key_fields = list(agg.key_fields)
        self.key_bytes = agg.key_bytes
        h = ct.c_void_p()
        check(self._L.gns_ex_view_create(agg._h, ct.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.gns_ex_view_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def refresh(self, since: int = 0) -> int:
        """Ingest side, asynchronous: select the flows touched after ``since`` (0: every flow;
        else a cursor an earlier refresh returned) as of every insert and merge issued so far.
        Returns the cursor of this point."""
        if since < 0:
            raise ValueError("since is a stream position (unsigned)")
        cur = ct.c_uint64(0)
        check(self._L.gns_ex_view_refresh(self._h, since, ct.byref(cur)))
        return int(cur.value)

    def snapshot_arrays(self):
        """(keys [n,K] canonical bytes, start, end, packets, bytes) of the view's rows, dictionary
        slot order: after refresh(0), what ExactAggregator.snapshot_arrays() gave at that point."""
        return _snapshot_arrays(self._L.gns_ex_view_snapshot, self._h, self.key_bytes)

    def aggregate(self, filters) -> List[Summary]:
        """ExactAggregator.aggregate over the view's rows."""
        return _aggregate(self._L.gns_ex_view_aggregate, self._L.gns_ex_view_aggregate_cidr, self._h, filters)

    def heavy_hitters(self, metric: int, threshold: int = 0, limit: int = 0):
        """ExactAggregator.heavy_hitters over the view's rows."""
        return _heavy_hitters(self._L.gns_ex_view_heavy_hitters, self._h, self.key_bytes, metric, threshold, limit)


def _int64_ns(what: str, t) -> int:
    t = int(t)
    if not -(1 << 63) <= t < (1 << 63):
        raise ValueError(f"{what} {t} is not an int64 of nanoseconds")
    return t


def _end_ptr(end_time, what: str = "end_time"):
    """The end_ns argument of a gns_ex_hist_* query: NULL (the newest snapshot) or an int64."""
    if end_time is None:
        return None, None
    c = ct.c_int64(_int64_ns(what, end_time))
    return c, ct.byref(c)


def _window(start_time, end_time):
    """The (start_ns, end_ns) arguments of gns_ex_hist_rollup_between, checked: (keep, start
    pointer, end pointer)."""
    k0, p0 = _end_ptr(start_time, "start_time")
    k1, p1 = _end_ptr(end_time)
    if k0 is not None and k1 is not None and k0.value > k1.value:
        raise ValueError(f"start_time {k0.value} lies after end_time {k1.value}")
    return (k0, k1), p0, p1


class ExactHistory:
    """The store behind the Querier's EndTime (gns_ex_hist_*): an append-only, device-resident
    log of the rows of refreshed ExactViews, each ``append`` one snapshot under a strictly
    increasing timestamp (ns, signed).  A query with ``end_time=T`` answers as of the newest
    snapshot at or before T -- per flow the latest row stored by then, the reference's
    argMax(..., Timestamp) with `Timestamp <= ?` -- and as an empty table when there is none;
    ``end_time=None`` is the newest snapshot.  Whole views and delta views (refresh(cursor))
    give the same answers.  Flows are never forgotten by a reset: rows stored before a reset of
    the aggregator stay, and a flow that returns supersedes its old row.  ``trim`` expires old
    snapshots (dropped, or folded into one base snapshot), ``export_log`` / ``append_rows`` and
    ``save`` / ``restore`` carry the whole log to a file and back."""

    def __init__(self, key_fields: Sequence[str], max_rows: int = 0, max_flows: int = 0, device: int = 0):
        if max_rows < 0 or max_flows < 0:
            raise ValueError("max_rows and max_flows are unsigned (initial capacities; both grow)")
        self._L = _lib.load()
        self.key_fields = list(key_fields)
        self.key_bytes = sum(_lib.FIELD_SIZE.get(f, 0) for f in self.key_fields)
        self.device = device
        p = _lib.ExHistParams()
        p.key = _lib.Layout.of(self.key_fields)
        p.max_rows, p.max_flows, p.device = max_rows, max_flows, device
        h = ct.c_void_p()
        check(self._L.gns_ex_hist_create(ct.byref(p), ct.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.gns_ex_hist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, view: ExactView, timestamp_ns: int):
        """The rows of a refreshed view as the next snapshot; may run on the snapshotter's thread
        while the aggregator ingests.  Returns (rows appended, keys new to the history)."""
        if not isinstance(view, ExactView):
            raise TypeError("append takes an ExactView")
        out = (ct.c_uint64 * 2)()
        check(self._L.gns_ex_hist_append(self._h, view._h, _int64_ns("timestamp_ns", timestamp_ns), out))
        return int(out[0]), int(out[1])

    def times(self) -> List[int]:
        n = ct.c_uint64(0)
        check(self._L.gns_ex_hist_times(self._h, None, ct.byref(n)))
        ts = np.zeros(max(n.value, 1), np.int64)
        n2 = ct.c_uint64(n.value)
        check(self._L.gns_ex_hist_times(self._h, ts.ctypes.data, ct.byref(n2)))
        return [int(t) for t in ts[:min(n.value, n2.value)]]

    STATS = ["snapshots", "rows", "keys", "row_capacity", "index_slots", "index_growths", "log_growths",
             "rows_trimmed"]

    def stats(self) -> dict:
        s = (ct.c_uint64 * 8)()
        check(self._L.gns_ex_hist_stats(self._h, s))
        return {k: int(s[i]) for i, k in enumerate(self.STATS) if k != "_"}

    def _bind(self, name: str, end_time):
        """fn(h, ...) as the live calls have it from gns_ex_hist_<name>(h, end_ns, ...)."""
        keep, ptr = _end_ptr(end_time)
        return lambda h, *a: getattr(self._L, "gns_ex_hist_" + name)(h, ptr, *a)

    def aggregate(self, filters, end_time=None, start_time=None):
        """ExactAggregator.aggregate as of ``end_time``: flows / packets / bytes over each flow's
        latest row, first_ns / last_ns / max_packets / max_bytes over every row stored by then.
        With ``start_time``: one ``Change(flows, packets, bytes)`` per filter, summary(end_time) -
        summary(start_time) as signed ints -- two device scans and a subtraction here."""
        if start_time is None:
            return _aggregate(self._bind("aggregate", end_time), self._bind("aggregate_cidr", end_time), self._h, filters)
        _window(start_time, end_time)
        filters = list(filters)
        new, old = self.aggregate(filters, end_time=end_time), self.aggregate(filters, end_time=start_time)
        return [Change(a.flows - b.flows, signed(a.packets - b.packets), signed(a.bytes - b.bytes)) for a, b in zip(new, old)]

    def heavy_hitters(self, metric: int, threshold: int = 0, limit: int = 0, end_time=None):
        """ExactAggregator.heavy_hitters over each flow's latest row as of ``end_time``."""
        return _heavy_hitters(self._bind("heavy_hitters", end_time), self._h, self.key_bytes, metric, threshold, limit)

    def snapshot_arrays(self, end_time=None):
        """(keys, start, end, packets, bytes) of each flow's latest row as of ``end_time``, in
        log order (snapshot, then the view's row order)."""
        return _snapshot_arrays(self._bind("snapshot", end_time), self._h, self.key_bytes, retry=True)

    # --- the table as of end_time, re-keyed on the device (gns_ex_hist_rollup) ---
    def rollup(self, key_fields: Sequence[str], prefix=None, end_time=None, **kw) -> "ExactAggregator":
        """A new aggregator on the history's device keyed on ``key_fields`` (fields of the
        history's layout, in any order) and filled by ``rollup_from_history(self, end_time,
        prefix)``: "bytes per source /24 as of T" without the rows leaving the GPU.  Empty when
        no snapshot lies at or before ``end_time``.  ``kw`` as ExactAggregator's constructor."""
        rollup_plan(self.key_fields, key_fields)
        if prefix is not None:
            make_prefix(prefix)
        _end_ptr(end_time)
        kw.setdefault("device", self.device)
        dst = ExactAggregator(key_fields, **kw)
        try:
            dst.rollup_from_history(self, end_time=end_time, prefix=prefix)
        except Exception:
            dst.close()
            raise
        return dst

    # --- what changed in a window (gns_ex_hist_rollup_between, gns_ex_movers) ---
    def delta(self, key_fields=None, prefix=None, start_time=None, end_time=None, **kw) -> "ExactAggregator":
        """A new aggregator keyed on ``key_fields`` (None: the history's own layout) whose counts
        are the CHANGES between ``start_time`` and ``end_time``: per group sum(T1) - sum(T0) in
        two's complement (``signed`` reads the u64 columns), filled by
        ``rollup_from_history(self, end_time, prefix, start_time)`` from the rows that differ
        between the two snapshots only.  ``start_time=None``: from before the first snapshot, the
        table as of ``end_time``.  A group whose packet change is 0 is no flow and is not listed,
        whatever its byte change.  Times: min start / max end over the group's rows stored in the
        window and current at ``end_time``."""
        key_fields = self.key_fields if key_fields is None else list(key_fields)
        rollup_plan(self.key_fields, key_fields)
        if prefix is not None:
            make_prefix(prefix)
        _window(start_time, end_time)
        kw.setdefault("device", self.device)
        dst = ExactAggregator(key_fields, **kw)
        try:
            dst.rollup_from_history(self, end_time=end_time, prefix=prefix, start_time=start_time)
        except Exception:
            dst.close()
            raise
        return dst

    def movers(self, key_fields, metric: int, direction: int = 0, threshold: int = 1, limit: int = 0, start_time=None,
               end_time=None, prefix=None):
        """The groups whose count changed most in the window: ``delta(key_fields, ...)``, its
        ``ExactAggregator.movers`` list, and the table closed again."""
        if metric not in (0, 1):
            raise ValueError(f"metric {metric}: 0 (PacketCount) or 1 (ByteCount)")
        if direction not in (-1, 0, 1):
            raise ValueError(f"direction {direction}: +1 (increases), -1 (decreases) or 0 (either)")
        if threshold < 0 or limit < 0 or threshold >= 1 << 64 or limit >= 1 << 64:
            raise ValueError("threshold and limit are unsigned 64-bit")
        tab = self.delta(key_fields, prefix=prefix, start_time=start_time, end_time=end_time)
        try:
            return tab.movers(metric, direction, threshold, limit)
        finally:
            tab.close()

    def table(self, end_time=None, **kw) -> "ExactAggregator":
        """The table as of ``end_time`` as a live handle of the history's own layout: the rows of
        ``snapshot_arrays(end_time)``, ready for rollup / spread / views / queries / merge."""
        return self.rollup(self.key_fields, end_time=end_time, **kw)

    def spread(self, flow_fields: Sequence[str], elem_fields: Sequence[str], flow_prefix=None, elem_prefix=None,
               end_time=None, **kw):
        """ExactAggregator.spread of the table as of ``end_time``: through ``table(end_time)``,
        which is closed again (the log is not projected into a spread table directly)."""
        spread_rollup_plan(self.key_fields, flow_fields, elem_fields)
        for p in (flow_prefix, elem_prefix):
            if p is not None:
                make_prefix(p)
        tab = self.table(end_time=end_time)
        try:
            return tab.spread(flow_fields, elem_fields, flow_prefix=flow_prefix, elem_prefix=elem_prefix, **kw)
        finally:
            tab.close()

    def hierarchical_heavy_hitters(self, field: str, levels, metric: int, threshold: int, end_time=None):
        """ExactAggregator.hierarchical_heavy_hitters of the table as of ``end_time``.  The finest
        level is rolled straight from the history, each coarser level from the one before it
        (``ExactAggregator.rollup``); only counts are read, so the chain is exact."""
        if field not in ("SrcIP", "DstIP"):
            raise ValueError(f"hierarchical heavy hitters: {field!r} is not an IP field")
        levels = check_levels(levels)
        if threshold < 1:
            raise ValueError("hierarchical heavy hitters: threshold must be at least 1")
        _end_ptr(end_time)
        lists, made, cur = [], [], None
        try:
            for lv in levels:
                if cur is None:
                    cur = self.rollup([field], prefix={field: lv}, end_time=end_time)
                else:
                    cur = cur.rollup([field], prefix={field: lv})
                made.append(cur)
                lists.append(cur.heavy_hitters(metric, threshold))
        finally:
            for a in made:
                a.close()
        return discount_heavy_prefixes(lists, levels, threshold)

    # --- retention and the log as data (gns_ex_hist_trim / _export / _append_rows) ---
    TRIM = ["snapshots_removed", "rows_released", "keys_forgotten", "rows"]

    def trim(self, before, fold: bool = True) -> dict:
        """Expire the snapshots with timestamp < ``before`` (int64 ns).  ``fold=True`` keeps of
        them each flow's latest row as one base snapshot under the last expired timestamp, so
        every answer with end_time at or after it is unchanged (earlier end times then answer
        as an empty table, and first_ns / last_ns / max_* range over the rows that remain);
        ``fold=False`` drops them with all their rows, and a flow seen only in them is
        forgotten.  Returns snapshots_removed, rows_released, keys_forgotten and the rows now
        held.  The kept rows move into a new, smaller log: the memory is returned."""
        before, out = _int64_ns("before", before), (ct.c_uint64 * 4)()
        check(self._L.gns_ex_hist_trim(self._h, before, int(fold), out))
        return {k: int(out[i]) for i, k in enumerate(self.TRIM)}

    def clear(self) -> dict:
        """Forget every snapshot: ``trim`` past the last timestamp with ``fold=False``.  Timestamps
        may start anew afterwards."""
        ts = self.times()
        if ts and ts[-1] == (1 << 63) - 1:
            raise ValueError("clear: no int64 lies past the last snapshot's timestamp")
        return self.trim(ts[-1] + 1 if ts else 0, fold=False)

    def export_log(self):
        """(keys, start, end, packets, bytes, written, times): every log row in log order --
        ``written[i]`` the number of the snapshot that stored row i, ``times[j]`` snapshot j's
        timestamp (int64 array).  ``append_rows`` of each snapshot's rows into an empty history
        rebuilds this one."""
        L, K = self._L, max(self.key_bytes, 1)
        while True:
            ts = np.asarray(self.times(), np.int64)
            n = ct.c_uint64(0)
            check(L.gns_ex_hist_export(self._h, None, None, None, None, None, None, ct.byref(n)))
            m = n.value
            keys = np.zeros((max(m, 1), K), np.uint8)
            st, en = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
            pk, by = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64)
            wr = np.zeros(max(m, 1), np.uint32)
            n2 = ct.c_uint64(m)
            check(L.gns_ex_hist_export(self._h, keys.ctypes.data, st.ctypes.data, en.ctypes.data, pk.ctypes.data,
                                       by.ctypes.data, wr.ctypes.data, ct.byref(n2)))
            # (another thread appended or trimmed between the calls: take the log again)
            if n2.value == m and self.times() == ts.tolist():
                return keys[:m, :self.key_bytes], st[:m], en[:m], pk[:m], by[:m], wr[:m], ts

    def append_rows(self, keys, start, end, packets, bytes, timestamp_ns: int):
        """One snapshot from host arrays of the form ``snapshot_arrays`` / ``export_log`` give, as
        ``append`` takes it from a view.  Every row carries packets and no key occurs twice
        (GnsError otherwise, the history's answers unchanged); no rows register the timestamp.
        Returns (rows appended, keys new to the history)."""
        st, en = np.ascontiguousarray(start, np.int64), np.ascontiguousarray(end, np.int64)
        pk, by = np.ascontiguousarray(packets, np.uint64), np.ascontiguousarray(bytes, np.uint64)
        n = int(st.shape[0])
        keys = np.ascontiguousarray(keys, np.uint8).reshape(n, -1) if n else np.zeros((0, self.key_bytes), np.uint8)
        if n and keys.shape[1] != self.key_bytes:
            raise ValueError(f"append_rows: keys must be [n, {self.key_bytes}]")
        if not (en.shape[0] == pk.shape[0] == by.shape[0] == n):
            raise ValueError("append_rows: row arrays differ in length")
        out, t = (ct.c_uint64 * 2)(), _int64_ns("timestamp_ns", timestamp_ns)
        ptrs = [a.ctypes.data if n else None for a in (keys, st, en, pk, by)]
        check(self._L.gns_ex_hist_append_rows(self._h, *ptrs, n, t, out))
        return int(out[0]), int(out[1])

    def save(self, path) -> None:
        """The whole log as one checkpoint file (checkpoint.save)."""
        from . import checkpoint
        checkpoint.save(self, path)

    def restore(self, path) -> None:
        """Replace the log by a checkpoint's (checkpoint.restore): cleared, then one append_rows
        per saved snapshot."""
        from . import checkpoint
        checkpoint.restore(self, path)


class ExactAggregator:
    """One exact task's device state (gns_ex handle)."""

    def __init__(self, key_fields: Sequence[str], max_flows: int = 0, batch_packets: int = 0, device: int = 0):
        self._L = _lib.load()
        self.key_fields = list(key_fields)
        self.key_bytes = sum(_lib.FIELD_SIZE.get(f, 0) for f in self.key_fields)
        self.device = device
        p = _lib.ExParams()
        p.key = _lib.Layout.of(self.key_fields)
        p.max_flows, p.batch_packets, p.device = max_flows, batch_packets, device
        h = ct.c_void_p()
        check(self._L.gns_ex_create(ct.byref(p), ct.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            for v in list(getattr(self, "_views", ())):  # a view is destroyed before its handle
                v.close()
            self._L.gns_ex_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def insert_tuples(self, batch: PacketBatch) -> None:
        n = len(batch)
        t, keep, where = batch.c_struct()
        ipver, ts = batch.ipver, batch.ts
        if ts is None:
            raise ValueError("exact aggregation needs per-packet timestamps (PacketBatch.ts)")
        if where == _lib.MEM_HOST:
            ts = np.ascontiguousarray(ts, np.int64)
            ipver = None if ipver is None else np.ascontiguousarray(ipver, np.uint8)
        elif not _is_dev(ts) or (ipver is not None and not _is_dev(ipver)):
            raise ValueError("mix of host and device arrays")
        check(self._L.gns_ex_insert_tuples(self._h, ct.byref(t), None if ipver is None else _ptr(ipver), _ptr(ts),
                                           n, where))
        del keep

    def insert_headers(self, hdr, wirelen, ts) -> None:
        dev = [_is_dev(a) for a in (hdr, wirelen, ts)]
        if all(dev):
            _lib.device_ready(hdr, wirelen, ts)
            where = _lib.MEM_DEVICE
        elif any(dev):
            raise ValueError("mix of host and device arrays")
        else:
            where = _lib.MEM_HOST
            hdr = np.ascontiguousarray(hdr, np.uint8)
            wirelen = np.ascontiguousarray(wirelen, np.uint32)
            ts = np.ascontiguousarray(ts, np.int64)
        check(self._L.gns_ex_insert_headers(self._h, _ptr(hdr), _ptr(wirelen), _ptr(ts), int(wirelen.shape[0]),
                                            where))

    def insert_compact(self, rec16, wirelen, ts, side=None) -> None:
        """Compact records (packets.compact_headers / read_pcap_compact) + timestamps: the
        same stream as insert_headers of the 64-byte records they were made from.
        wirelen None: the 16-byte form (24 bytes per packet with the timestamps)."""
        from .sketch import _compact_args
        if ts is None:
            raise ValueError("the exact aggregator needs timestamps")
        (rec, wl, sd, tp), n, ns, where, keep = _compact_args(rec16, wirelen, side, ts)
        if n == 0:
            return
        check(self._L.gns_ex_insert_compact(self._h, rec, wl, tp, n, sd, ns, where))

    def flush(self) -> None:
        check(self._L.gns_ex_flush(self._h))

    def query_many(self, flows) -> np.ndarray:
        """PacketCount<<32 | ByteCount for n flows; a device tensor in -> a device int64 tensor out."""
        if _lib.is_device(flows):
            return _lib.query_device(self._L.gns_ex_query_device, self._h, flows)
        flows = np.ascontiguousarray(flows, np.uint8)
        n = flows.shape[0]
        out = np.zeros(n, np.uint64)
        if n:
            flows = flows.reshape(n, -1)
            check(self._L.gns_ex_query(self._h, flows.ctypes.data, flows.shape[1], n, out.ctypes.data))
        return out

    def snapshot_arrays(self):
        """(keys [n,K] canonical bytes, start, end, packets, bytes), dictionary slot order."""
        return _snapshot_arrays(self._L.gns_ex_snapshot, self._h, self.key_bytes)

    def view(self) -> ExactView:
        """A snapshot view of this aggregator (closed with it at the latest)."""
        import weakref
        v = ExactView(self)
        if not hasattr(self, "_views"):
            self._views = weakref.WeakSet()
        self._views.add(v)
        return v

    def merge(self, keys, start, end, pkts, bytes) -> None:
        """gns_ex_merge: add the rows of a snapshot_arrays() (this handle's or another shard's) to
        the table, each row one pseudo-record at the current end of the stream -- a restore when
        the table is empty, a union otherwise.  numpy arrays, or device tensors (keys uint8
        [n, key_bytes], the others int64 holding the 64-bit values)."""
        arrs = (keys, start, end, pkts, bytes)
        dev = [_is_dev(a) for a in arrs]
        if all(dev):
            n = int(start.shape[0])
            keys = keys.reshape(n, -1) if n else keys
            if n and (int(keys.shape[1]) != self.key_bytes or keys.element_size() != 1):
                raise ValueError(f"merge: keys must be uint8 [n, {self.key_bytes}]")
            if any(a.element_size() != 8 or int(a.shape[0]) != n for a in arrs[1:]):
                raise ValueError("merge: start / end / pkts / bytes must be 64-bit [n]")
            arrs = tuple(a.contiguous() for a in (keys,) + arrs[1:])
            _lib.device_ready(*arrs)
            where = _lib.MEM_DEVICE
        elif any(dev):
            raise ValueError("mix of host and device arrays")
        else:
            st, en = np.ascontiguousarray(start, np.int64), np.ascontiguousarray(end, np.int64)
            pk, by = np.ascontiguousarray(pkts, np.uint64), np.ascontiguousarray(bytes, np.uint64)
            n = int(st.shape[0])
            keys = np.ascontiguousarray(keys, np.uint8).reshape(n, -1) if n else np.zeros((0, self.key_bytes), np.uint8)
            if n and keys.shape[1] != self.key_bytes:
                raise ValueError(f"merge: keys must be [n, {self.key_bytes}]")
            if not (en.shape[0] == pk.shape[0] == by.shape[0] == n):
                raise ValueError("merge: row arrays differ in length")
            arrs = (keys, st, en, pk, by)
            where = _lib.MEM_HOST
        if n:
            check(self._L.gns_ex_merge(self._h, *[_ptr(a) for a in arrs], n, where))

    def rollup_from(self, src: "ExactAggregator", prefix=None):
        """gns_ex_rollup: re-key the flows of ``src`` onto this handle's layout, on the device.
        The flows that share one projected key enter as one pseudo-record under the rule of
        ``merge``: summed counts, the start of the constituent earliest and the end of the one
        latest in src's stream.  Into an empty handle the result equals an aggregator of this
        layout fed src's packets.  src is only read.  Returns (flows of src projected, flows
        new in this handle).

        ``prefix`` (gns_ex_rollup_prefix): ``{"SrcIP": (24, 48), "DstIP": 16}`` masks the projected
        key's IP fields to their leading bits -- (IPv4 bits, IPv6 bits), a lone int the IPv4
        length with IPv6 kept whole -- as ``mask_prefix`` does; the result then equals an
        aggregator of this layout fed src's packets with their addresses masked.  A prefix for
        a field this layout lacks is ignored.  None takes the unmasked entry point."""
        if not isinstance(src, ExactAggregator):
            raise TypeError("rollup_from takes an ExactAggregator")
        if src is not self:  # (dst is src: GNS_E_ARG from the library)
            rollup_plan(src.key_fields, self.key_fields)
        out = (ct.c_uint64 * 2)()
        if prefix is None:
            check(self._L.gns_ex_rollup(self._h, src._h, out))
        else:
            px = make_prefix(prefix)
            check(self._L.gns_ex_rollup_prefix(self._h, src._h, ct.byref(px), out))
        return int(out[0]), int(out[1])

    def rollup_from_history(self, hist: "ExactHistory", end_time=None, prefix=None, start_time=None):
        """gns_ex_hist_rollup: re-key the table ``hist`` holds as of ``end_time`` -- each flow's
        latest row stored by then, the rows ``hist.snapshot_arrays(end_time)`` lists -- onto this
        handle's layout, on the device.  The reference's GROUP BY over stored rows: the flows that
        share one projected key enter with summed counts (u64 wrap; a group whose packets sum to
        0 is no flow), the smallest start and the largest end (signed) -- not ``rollup_from``'s
        stream-order rule, log rows have no stream positions.  A key this handle already holds
        adds its counts and keeps the smaller start and the larger end.  ``prefix`` as
        ``rollup_from``'s.  hist is only read.  Returns (rows of hist projected, flows new in
        this handle); (0, 0) when no snapshot lies at or before ``end_time``.

        ``start_time`` (gns_ex_hist_rollup_between): only what changed after it enters -- the
        rows stored in the window that are current at ``end_time`` add, the rows current at
        ``start_time`` that were displaced in the window subtract (two's complement; ``signed``),
        and times are the min / max over the former.  Returns (rows selected, flows new in this
        handle); (0, 0) and no position spent when no snapshot lies in the window."""
        if not isinstance(hist, ExactHistory):
            raise TypeError("rollup_from_history takes an ExactHistory")
        rollup_plan(hist.key_fields, self.key_fields)
        px = make_prefix(prefix) if prefix is not None else None
        keep, sptr, ptr = _window(start_time, end_time)
        if hist.device != self.device:
            raise ValueError(f"rollup_from_history: this handle is on device {self.device}, "
                             f"the history on device {hist.device}")
        out = (ct.c_uint64 * 2)()
        pxp = ct.byref(px) if px is not None else None
        if start_time is None:  # (a NULL start is the same call, bit for bit)
            check(self._L.gns_ex_hist_rollup(self._h, hist._h, ptr, pxp, out))
        else:
            check(self._L.gns_ex_hist_rollup_between(self._h, hist._h, sptr, ptr, pxp, out))
        return int(out[0]), int(out[1])

    def rollup(self, key_fields: Sequence[str], prefix=None, **kw) -> "ExactAggregator":
        """A new aggregator on the same device keyed on ``key_fields`` (fields of this handle's
        layout, in any order) and filled by ``rollup_from(self, prefix)``; ``kw`` as the
        constructor's."""
        rollup_plan(self.key_fields, key_fields)
        if prefix is not None:
            make_prefix(prefix)
        kw.setdefault("device", self.device)
        dst = ExactAggregator(key_fields, **kw)
        try:
            dst.rollup_from(self, prefix)
        except Exception:
            dst.close()
            raise
        return dst

    def spread(self, flow_fields: Sequence[str], elem_fields: Sequence[str], flow_prefix=None, elem_prefix=None, **kw):
        """A new ExactSpread on the same device -- distinct ``elem_fields`` values per
        ``flow_fields`` value, both made of fields of this handle's key -- filled by
        ``ExactSpread.rollup_from(self)``: what a spread handle of those layouts fed the same
        packets holds (IPv4-mapped arrivals counted with their IPv4 address).  ``flow_prefix`` /
        ``elem_prefix`` (``rollup_from``'s ``prefix``) mask the IP fields of the flow / element
        row: hosts per source /24 is ``spread(["SrcIP"], ["SrcIP"], flow_prefix={"SrcIP": 24})``.
        ``kw`` as ExactSpread's constructor."""
        from .spread import ExactSpread
        spread_rollup_plan(self.key_fields, flow_fields, elem_fields)
        kw.setdefault("device", self.device)
        dst = ExactSpread(flow_fields, elem_fields, **kw)
        try:
            dst.rollup_from(self, flow_prefix=flow_prefix, elem_prefix=elem_prefix)
        except Exception:
            dst.close()
            raise
        return dst

    def aggregate(self, filters) -> List[Summary]:
        """gns_ex_aggregate: one Summary per filter (``make_filter`` values, equality or CIDR, or
        dicts of its arguments) from one device scan per 64 filters; nothing but the answers
        leaves the GPU."""
        return _aggregate(self._L.gns_ex_aggregate, self._L.gns_ex_aggregate_cidr, self._h, filters)

    def heavy_hitters(self, metric: int, threshold: int = 0, limit: int = 0):
        """gns_ex_heavy_hitters: (keys [n, K] canonical bytes, values uint64 [n]) of the flows
        with PacketCount (metric 0) / ByteCount (metric 1) >= threshold, value descending, ties
        by key bytes ascending, cut to ``limit`` rows when limit != 0."""
        return _heavy_hitters(self._L.gns_ex_heavy_hitters, self._h, self.key_bytes, metric, threshold, limit)

    def movers(self, metric: int, direction: int = 0, threshold: int = 1, limit: int = 0):
        """gns_ex_movers on a table of changes (``ExactHistory.delta``): (keys [n, K], values
        int64 [n]) of the groups whose packet (metric 0) / byte (metric 1) change v is not 0, has
        the sign of ``direction`` (+1 increases, -1 decreases, 0 either) and |v| >= max(threshold,
        1); |v| descending, ties by key bytes ascending, cut to ``limit`` rows when limit != 0."""
        return _movers(lambda *a: self._L.gns_ex_movers(*a), self._h, self.key_bytes, metric, direction, threshold, limit)

    def hierarchical_heavy_hitters(self, field: str, levels, metric: int, threshold: int):
        """Exact hierarchical heavy hitters of one IP field: ``levels`` is a list of (IPv4 bits,
        IPv6 bits) from finest to coarsest, e.g. [(32, 128), (24, 64), (16, 48), (8, 32)].  The
        table is rolled up to ``[field]`` at the finest level, each coarser level from the one
        before it, all on the device; ``heavy_hitters(metric, threshold)`` of every level is
        then discounted on the host (``discount_heavy_prefixes``).  Returns, per level, the list
        of (prefix key bytes, total, conditioned count) of the prefixes reported, in the
        canonical list order.  Counts are Python ints; totals are assumed below 2^64."""
        if field not in ("SrcIP", "DstIP"):
            raise ValueError(f"hierarchical heavy hitters: {field!r} is not an IP field")
        levels = check_levels(levels)
        if threshold < 1:
            raise ValueError("hierarchical heavy hitters: threshold must be at least 1")
        lists, made, cur = [], [], self
        try:
            for lv in levels:
                cur = cur.rollup([field], prefix={field: lv})
                made.append(cur)
                lists.append(cur.heavy_hitters(metric, threshold))
        finally:
            for a in made:
                a.close()
        return discount_heavy_prefixes(lists, levels, threshold)

    def reset(self) -> None:
        check(self._L.gns_ex_reset(self._h))

    def counters(self) -> dict:
        s = (ct.c_uint64 * 8)()
        check(self._L.gns_ex_counters(self._h, s))
        names = ["inserted", "dropped", "unsupported", "dict_full", "flows", "records", "batches", "_"]
        return {k: int(s[i]) for i, k in enumerate(names) if k != "_"}

    def dict_stats(self) -> dict:
        """Table growth counters (gns_ex_dict_stats): growths, -, slots, claimed, us, re-run batches."""
        d = _lib.dict_stats(self._L.gns_ex_dict_stats, self._h)
        return {"growths": d["reclaims"], "slots": d["live"], "claimed": d["claimed"], "grow_us": d["reclaim_us"],
                "retried_batches": d["retried_batches"]}

    def set_timing(self, on: bool = True, stages=None) -> None:
        check(self._L.gns_ex_set_timing(self._h, _lib.timing_arg(on, stages, self.STAGES)))

    STAGES = ["extract", "resolve", "partition", "aggregate", "hot", "total", "query", "view"]

    def stage_times(self, reset: bool = False) -> dict:
        ms = (ct.c_double * 8)()
        ln = (ct.c_uint64 * 8)()
        check(self._L.gns_ex_stage_times(self._h, ms, ln, 1 if reset else 0))
        return {name: (ms[i], ln[i]) for i, name in enumerate(self.STAGES)}


def key_string(key: bytes, fields: Sequence[str]):
    """Go key string and Fields map from canonical key bytes (task.go:330-366)."""
    parts, vals, off = [], {}, 0
    for f in fields:
        if f in ("SrcIP", "DstIP"):
            v = go_ip_string(key[off:off + 16])
            off += 16
        elif f in ("SrcPort", "DstPort"):
            v = struct.unpack(">H", key[off:off + 2])[0]
            off += 2
        elif f == "Protocol":
            v = key[off]
            off += 1
        else:
            raise ValueError(f"unknown key field: {f}")
        parts.append(str(v))
        vals[f] = v
    return "-".join(parts), vals


class ExactTask:
    """model.Task of the exact aggregator (exact/task.go)."""

    def __init__(self, name: str, key_fields: Sequence[str], num_shards: int = 0, device: int = 0,
                 max_flows: int = 0, batch_packets: int = 0, agg: Optional[ExactAggregator] = None):
        if num_shards == 0 or num_shards >= 32768:  # task.go:85-87
            num_shards = DEFAULT_SHARDS
        self.name_ = name
        self.key_fields = list(key_fields)
        self.shard_count = num_shards
        self.agg = agg if agg is not None else ExactAggregator(self.key_fields, max_flows=max_flows,
                                                               batch_packets=batch_packets, device=device)

    def name(self) -> str:
        return self.name_

    def fields(self):  # task.go:111-114: exact tasks serialize no field list
        return None

    def decode_flow_func(self):
        return lambda flow, fields: ""

    def process_packets(self, batch) -> None:
        if isinstance(batch, HeaderBatch):
            ts = batch.ts if batch.ts is not None else np.zeros(len(batch), np.int64)
            self.agg.insert_headers(batch.hdr, batch.wirelen, ts)
        elif isinstance(batch, CompactBatch):
            ts = batch.ts
            if ts is None and batch.is_device():
                import torch
                ts = torch.zeros(len(batch), dtype=torch.int64, device=batch.rec16.device)
            elif ts is None:
                ts = np.zeros(len(batch), np.int64)
            self.agg.insert_compact(batch.rec16, batch.wirelen, ts, batch.side)
        else:
            self.agg.insert_tuples(batch)

    def process_packet(self, info) -> None:
        """ProcessPacket(*PacketInfo); info = (src, dst, sport, dport, proto, length[, ts_ns])."""
        self.process_packets(PacketBatch.from_packets([info]))

    def query(self, flow: bytes) -> int:
        """Query (task.go:298-326): PacketCount<<32 | ByteCount, IP fields read as 16-byte IPs."""
        if len(flow) != self.agg.key_bytes:
            return 0
        return int(self.agg.query_many(np.frombuffer(bytes(flow), np.uint8).reshape(1, -1))[0])

    def flows(self, arrays=None) -> List[Flow]:
        keys, st, en, pk, by = self.agg.snapshot_arrays() if arrays is None else arrays
        out = []
        for i in range(len(pk)):
            k, vals = key_string(bytes(keys[i]), self.key_fields)
            out.append(Flow(k, vals, int(st[i]), int(en[i]), int(by[i]), int(pk[i])))
        return out

    def snapshot(self, arrays=None) -> SnapshotData:
        """Snapshot (task.go:153-191).  The reference spreads flows over shards by a
        randomly seeded maphash; here by a fixed hash of the key string."""
        import zlib
        shards = [Shard() for _ in range(self.shard_count)]
        for f in self.flows(arrays):
            shards[zlib.crc32(f.Key.encode()) % self.shard_count].Flows[f.Key] = f
        return SnapshotData(self.name_, shards)

    def view(self) -> ExactView:
        """A snapshot view of the task's table: refresh it on the ingest thread at the interval's
        end, then hand it to the snapshotter / alerter thread (snapshot_from, view.aggregate)."""
        return self.agg.view()

    def snapshot_from(self, view: ExactView) -> SnapshotData:
        """Snapshot built from a view's rows instead of the live table: the whole table after
        view.refresh(), the interval's changed flows after view.refresh(cursor).  May run on
        another thread while the task keeps ingesting."""
        return self.snapshot(view.snapshot_arrays())

    def rollup(self, name: str, key_fields: Sequence[str], num_shards: int = 0, prefix=None, end_time=None,
               start_time=None, **kw) -> "ExactTask":
        """A full task keyed on ``key_fields`` (fields of this task's key, in any order) holding
        this task's flows re-keyed on the device (ExactAggregator.rollup): what a task configured
        with that key and fed the same packets -- their addresses masked by ``prefix``, when one is
        given -- holds.  It takes packets, queries, views and checkpoints like any other task.
        ``end_time``: the table as of that time, from the attached history
        (ExactHistory.rollup; ValueError when none is attached) instead of the live one.
        ``start_time``: the changes from then to ``end_time`` (None: the newest snapshot) from the
        attached history (ExactHistory.delta) -- counts are signed changes."""
        if start_time is not None:
            agg = self._window_history(start_time).delta(key_fields, prefix=prefix, start_time=start_time,
                                                         end_time=end_time, **kw)
            return ExactTask(name, key_fields, num_shards, agg=agg)
        src = self.agg if end_time is None else self._as_of(end_time)
        extra = {} if end_time is None else {"end_time": end_time}
        return ExactTask(name, key_fields, num_shards, agg=src.rollup(key_fields, prefix=prefix, **extra, **kw))

    def spread(self, flow_fields: Sequence[str], elem_fields: Sequence[str], flow_prefix=None, elem_prefix=None,
               end_time=None, **kw):
        """The exact spread table of this task's flows (ExactAggregator.spread): SuperSpread's
        ground truth for those layouts without a spread engine on the ingest path.  ``end_time``:
        of the table as of that time, from the attached history (ExactHistory.spread)."""
        if end_time is not None:
            return self._as_of(end_time).spread(flow_fields, elem_fields, flow_prefix=flow_prefix,
                                                elem_prefix=elem_prefix, end_time=end_time, **kw)
        return self.agg.spread(flow_fields, elem_fields, flow_prefix=flow_prefix, elem_prefix=elem_prefix, **kw)

    def hierarchical_heavy_hitters(self, field: str, levels, metric: int, threshold: int, end_time=None):
        """ExactAggregator.hierarchical_heavy_hitters of this task's table, or with ``end_time``
        of the table as of that time (ExactHistory.hierarchical_heavy_hitters)."""
        if end_time is not None:
            return self._as_of(end_time).hierarchical_heavy_hitters(field, levels, metric, threshold, end_time=end_time)
        return self.agg.hierarchical_heavy_hitters(field, levels, metric, threshold)

    def reset(self) -> None:
        self.agg.reset()

    def flush(self) -> None:
        self.agg.flush()

    def save(self, path) -> None:
        """The flow table as one checkpoint file (checkpoint.save)."""
        from . import checkpoint
        checkpoint.save(self.agg, path)

    def restore(self, path) -> None:
        """Replace the flow table by a checkpoint's (checkpoint.restore)."""
        from . import checkpoint
        checkpoint.restore(self.agg, path)

    # --- the history behind end_time (gns_ex_hist_*) ---
    def keep_history(self, retain=None, **kw) -> ExactHistory:
        """Attach an ExactHistory of this task's layout (``kw``: its max_rows / max_flows), a view
        and a cursor: ``record`` then stores an interval, and the Querier calls below answer
        ``end_time`` from it.  Returns the history (the one already attached, if any).

        ``retain=N`` (N >= 1; None: keep everything): after each record the history is folded
        (``ExactHistory.trim(fold=True)``) down to at most N snapshots, the base included, so
        answers reach back N - 1 intervals and the log stops growing with time."""
        if retain is not None:
            if isinstance(retain, bool) or int(retain) != retain or retain < 1:
                raise ValueError(f"retain {retain!r}: a number of snapshots >= 1, or None")
            retain = int(retain)
        if getattr(self, "history", None) is None:
            self._hist_retain = retain
            kw.setdefault("device", self.agg.device)
            self.history = ExactHistory(self.key_fields, **kw)
            self._hist_view = self.agg.view()
            self._hist_cursor = 0
        return self.history

    def record(self, timestamp_ns: int, full: bool = False):
        """One interval of the snapshotter (manager.go:139-159): refresh the history's view -- the
        flows touched since the last record, or the whole table with ``full`` -- and append it
        under ``timestamp_ns``.  Returns (rows appended, keys new to the history)."""
        h = getattr(self, "history", None)
        if h is None:
            raise ValueError("record: no history attached (keep_history first)")
        cur = self._hist_view.refresh(0 if full else self._hist_cursor)
        out = h.append(self._hist_view, timestamp_ns)
        self._hist_cursor = cur  # (after the append: a rejected timestamp loses no interval)
        keep = getattr(self, "_hist_retain", None)
        if keep is not None:
            ts = h.times()
            if len(ts) > keep:  # fold all but the newest keep - 1 into the base
                h.trim(ts[-(keep - 1)] if keep > 1 else ts[-1] + 1, fold=True)
        return out

    def save_history(self, path) -> None:
        """The attached history's log as one checkpoint file (ExactHistory.save)."""
        self._history("save_history").save(path)

    def restore_history(self, path) -> None:
        """Replace the attached history's log by a checkpoint's (ExactHistory.restore).  The next
        delta ``record`` after a ``restore`` of the flow table stores every restored flow again
        -- the merge touched them all -- which is correct, only larger."""
        self._history("restore_history").restore(path)

    def _history(self, what: str) -> ExactHistory:
        h = getattr(self, "history", None)
        if h is None:
            raise ValueError(f"{what}: no history attached (keep_history first)")
        return h

    def _as_of(self, end_time):
        """The history an end_time query answers from; ValueError without one."""
        h = getattr(self, "history", None)
        if h is None:
            _no_end_time(end_time)
        return h

    def _window_history(self, start_time):
        """The history a start_time query answers from; ValueError without one."""
        h = getattr(self, "history", None)
        if h is None:
            raise ValueError("start_time is not supported: no history attached (keep_history first)")
        return h

    # --- query.Querier (internal/query/querier.go) on the live table, or as of end_time ---
    def aggregate_flows_many(self, requests) -> List[TaskSummary]:
        """AggregateFlows (querier.go:251-319) for a batch of AggregationRequests.  A request is a
        dict of src_ip / dst_ip / src_port / dst_port / protocol (absent or None: no constraint),
        end_time and start_time.  The requests without either are answered from the live table in
        ONE device call; those with an end_time from the attached history, one device call per
        distinct end_time (ValueError when no history is attached).  A request with start_time
        answers with the signed changes of the window (ExactHistory.aggregate's Change; end_time
        None: the newest snapshot), always from the history."""
        flt, at = [], []
        for req in requests:
            req = dict(req)
            t, t0 = req.pop("end_time", None), req.pop("start_time", None)
            if t0 is not None:
                self._window_history(t0)
                _window(t0, t)
            elif t is not None:
                self._as_of(t)
            at.append((t0, t))
            flt.append(make_filter(**req))
        out = [None] * len(flt)
        for t0, t in dict.fromkeys(at):  # distinct windows / end times, in order of appearance
            idx = [i for i, x in enumerate(at) if x == (t0, t)]
            sub = [flt[i] for i in idx]
            if t0 is not None:
                res = self.history.aggregate(sub, end_time=t, start_time=t0)
            else:
                res = self.agg.aggregate(sub) if t is None else self.history.aggregate(sub, end_time=t)
            for i, r in zip(idx, res):
                out[i] = r
        return [TaskSummary(self.name_, s.bytes, s.packets, s.flows) for s in out]

    def aggregate_flows(self, src_ip=None, dst_ip=None, src_port=None, dst_port=None, protocol=None,
                        end_time=None, start_time=None) -> TaskSummary:
        return self.aggregate_flows_many([dict(src_ip=src_ip, dst_ip=dst_ip, src_port=src_port, dst_port=dst_port,
                                               protocol=protocol, end_time=end_time, start_time=start_time)])[0]

    def trace_flow(self, flow_keys, end_time=None) -> FlowLifecycle:
        """TraceFlow (querier.go:322-372): min(StartTime), max(EndTime), max(PacketCount),
        max(ByteCount) of the flows equal to ``flow_keys`` on every key given (all zero when
        none is)."""
        flt = filter_from_flow_keys(flow_keys)
        if end_time is not None:
            s = self._as_of(end_time).aggregate([flt], end_time=end_time)[0]
        else:
            s = self.agg.aggregate([flt])[0]
        return FlowLifecycle(s.first_ns, s.last_ns, s.max_packets, s.max_bytes)

    def heavy_hitters(self, type: int, limit: int, end_time=None) -> List[HeavyHitter]:
        """QueryHeavyHitters (querier.go:191-248): Type 0 PacketCount, 1 ByteCount, ORDER BY value
        DESC LIMIT ``limit`` (ties by key bytes; LIMIT 0 and an unknown Type select no row, as
        in the reference)."""
        hist = self._as_of(end_time) if end_time is not None else None
        if limit < 0:
            raise ValueError("negative limit")
        if type not in (0, 1) or limit == 0:
            return []
        if hist is not None:
            keys, vals = hist.heavy_hitters(type, 0, limit, end_time=end_time)
        else:
            keys, vals = self.agg.heavy_hitters(type, 0, limit)
        return [HeavyHitter(key_string(bytes(k), self.key_fields)[0], int(v)) for k, v in zip(keys, vals)]

    def movers(self, type: int, limit: int, start_time=None, end_time=None, direction: int = 0) -> List[HeavyHitter]:
        """The flows of this task's key whose PacketCount (Type 0) / ByteCount (Type 1) changed
        most between ``start_time`` and ``end_time`` in the attached history
        (ExactHistory.movers): ORDER BY abs(change) DESC LIMIT ``limit``, ties by key bytes;
        ``Value`` is the signed change.  LIMIT 0 and an unknown Type select no row, as in
        ``heavy_hitters``."""
        hist = self._window_history(start_time)
        if limit < 0:
            raise ValueError("negative limit")
        _window(start_time, end_time)
        if direction not in (-1, 0, 1):
            raise ValueError(f"direction {direction}: +1 (increases), -1 (decreases) or 0 (either)")
        if type not in (0, 1) or limit == 0:
            return []
        keys, vals = hist.movers(self.key_fields, type, direction, 1, limit, start_time=start_time, end_time=end_time)
        return [HeavyHitter(key_string(bytes(k), self.key_fields)[0], int(v)) for k, v in zip(keys, vals)]

    def alerter_msg(self, rules) -> str:
        """AlerterMsg (task.go:213-282): total_packets / total_bytes / total_flows, the one
        unfiltered aggregate of the device table."""
        t = self.agg.aggregate([make_filter()])[0]
        totals = {"total_packets": (float(t.packets), "packets"), "total_bytes": (float(t.bytes), "bytes"),
                  "total_flows": (float(t.flows), "flows")}
        msgs = []
        for rule in rules:
            if rule.get("task_name") != self.name_:
                continue
            metric = rule.get("metric")
            if metric not in totals:
                continue
            value, unit = totals[metric]
            op, thr = rule.get("operator", ">"), float(rule.get("threshold", 0))
            if _check(value, thr, op):
                msgs.append(f"<h3>Alert: {rule.get('name', '')}</h3><ul><li><b>Task:</b> <code>{rule.get('task_name')}</code></li>"
                            f"<li><b>Metric:</b> <code>{metric}</code></li><li><b>Condition:</b> <code>{op} {thr:.2f}</code></li>"
                            f"<li><b>Observed Value:</b> <code>{value:.0f} {unit}</code></li></ul>")
        return "<br><hr><br>".join(msgs)

    Name = name
    Fields = fields
    DecodeFlowFunc = decode_flow_func
    ProcessPacket = process_packet
    Query = query
    Snapshot = snapshot
    Reset = reset
    AlerterMsg = alerter_msg
    AggregateFlows = aggregate_flows
    TraceFlow = trace_flow
    QueryHeavyHitters = heavy_hitters


def NewExact(name: str, key_fields: Sequence[str], num_shards: int = 0, **kw) -> ExactTask:  # exact/task.go:83
    return ExactTask(name, key_fields, num_shards, **kw)
