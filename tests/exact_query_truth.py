"""Truth side of the exact query-plane tests: the ClickHouse comparison itself.

The reference answers AggregateFlows / TraceFlow with `column = ?` over the rows the
exact writer stored, one column per key field (querier.go:143-188).  A flow's columns
are the parts of its Go key string strings.Join(fields, "-") (exact/task.go:330-366; IP
strings never contain "-"), so the truth needs nothing from the engine: split the
oracle's key strings, compare each part with the Go-printed filter value.
"""
from __future__ import annotations

import ipaddress
import struct

import numpy as np

from helpers import random_tuples

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
ARG = {"SrcIP": "src_ip", "DstIP": "dst_ip", "SrcPort": "src_port", "DstPort": "dst_port", "Protocol": "protocol"}


def go_value(field: str, value) -> str:
    """The string the reference's column holds for this filter value."""
    from go2netspectra_amd.exact import ip_to16
    from go2netspectra_amd.task import go_ip_string
    if field in ("SrcIP", "DstIP"):
        return go_ip_string(ip_to16(value))
    return str(int(value))


def truth_rows(export: dict, fields):
    """[(parts {field: string}, start, end, packets, bytes, key string)] of an oracle export."""
    rows = []
    for k, (st, en, pk, by) in export.items():
        parts = k.split("-")
        assert len(parts) == len(fields), k
        rows.append((dict(zip(fields, parts)), st, en, pk, by, k))
    return rows


def truth_summary(rows, fields, flt: dict):
    """Summary of the rows equal to ``flt`` ({field name: value}) on every field given."""
    from go2netspectra_amd import Summary
    want = {f: go_value(f, v) for f, v in flt.items()}
    if any(f not in fields for f in want):  # a NULL column: `NULL = ?` selects nothing
        return Summary()
    hit = [r for r in rows if all(r[0][f] == s for f, s in want.items())]
    if not hit:
        return Summary()
    m64 = (1 << 64) - 1
    return Summary(len(hit), sum(r[3] for r in hit) & m64, sum(r[4] for r in hit) & m64,
                   min(r[1] for r in hit), max(r[2] for r in hit), max(r[3] for r in hit), max(r[4] for r in hit))


def to_filter(flt: dict):
    from go2netspectra_amd import make_filter
    return make_filter(**{ARG[f]: v for f, v in flt.items()})


def key_bytes_of(key: str, fields) -> bytes:
    """The engine's canonical key bytes rebuilt from a Go key string."""
    out = b""
    for f, part in zip(fields, key.split("-")):
        if f in ("SrcIP", "DstIP"):
            a = ipaddress.ip_address(part)
            out += (bytes(10) + b"\xff\xff" + a.packed) if a.version == 4 else a.packed
        elif f in ("SrcPort", "DstPort"):
            out += struct.pack(">H", int(part))
        else:
            out += bytes([int(part)])
    return out


def truth_heavy(export: dict, fields, metric: int, threshold: int = 0, limit: int = 0):
    """[(key bytes, value)] with value >= threshold by (-value, key bytes), cut to limit."""
    rows = [(key_bytes_of(k, fields), v[3] if metric else v[2]) for k, v in export.items()]
    rows = sorted((r for r in rows if r[1] >= threshold), key=lambda r: (-r[1], r[0]))
    return rows[:limit] if limit else rows


def got_heavy(keys, vals):
    return [(bytes(k), int(v)) for k, v in zip(keys, vals)]


def tricky_stream(seed: int, n: int, nflows: int, big_frac: float = 0.2):
    """IPv4 flows, the same flows arriving IPv4-mapped over IPv6 (same key string), IPv6
    addresses whose slot bytes equal an IPv4 slot (a different string); wire lengths near
    2^32 on a fraction of the packets; timestamps in [-2^40, 2^40), not monotonic."""
    rng = np.random.default_rng(seed)
    t = random_tuples(rng, n, nflows, v6_frac=0.3, s=1.05)
    v6 = t["v6"].copy()
    ipver = np.where(v6, 6, 4).astype(np.uint8)
    m = (rng.random(n) < 0.15) & ~v6
    for a in ("src16", "dst16"):
        x = t[a]
        x[m, 12:16] = x[m, 0:4]
        x[m, 0:10] = 0
        x[m, 10:12] = 0xFF
    ipver[m] = 6
    alias = (rng.random(n) < 0.05) & ~v6 & ~m
    ipver[alias] = 6
    big = rng.random(n) < big_frac
    t["length"][big] = rng.integers((1 << 32) - (1 << 20), 1 << 32, int(big.sum()), dtype=np.uint64).astype(np.uint32)
    ts = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    return t, ipver, ts


def batch_of(t, ipver, ts, sel=slice(None)):
    from go2netspectra_amd import PacketBatch
    return PacketBatch(t["src16"][sel], t["dst16"][sel], t["sport"][sel], t["dport"][sel], t["proto"][sel],
                       t["length"][sel], ipver[sel], ts[sel])


def oracle_export(oracle, fields, t, ipver, ts, sel=slice(None)):
    o = oracle.Exact(fields)
    o.insert_tuples(t["src16"][sel], t["dst16"][sel], t["sport"][sel], t["dport"][sel], t["proto"][sel],
                    ipver[sel], t["length"][sel], ts[sel])
    return o.export()


def packet_value(t, ipver, i: int, field: str):
    """Filter value of ``field`` as packet i carries it (IPs as net.IP bytes: 4 or 16)."""
    if field in ("SrcIP", "DstIP"):
        slot = bytes(t["src16" if field == "SrcIP" else "dst16"][i])
        return slot[:4] if ipver[i] == 4 else slot
    return int(t[{"SrcPort": "sport", "DstPort": "dport", "Protocol": "proto"}[field]][i])
