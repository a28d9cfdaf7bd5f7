"""Truth side of the prefix tests (roll-up, spread roll-up, CIDR filters, hierarchical heavy
hitters): the stream, and the prefix mask restated on packets, sharing no code with the engine
or with go2netspectra_amd.exact.

The stream is the tricky stream of exact_query_truth.py (IPv4, IPv4-mapped and genuine IPv6
arrivals, 16-byte addresses whose bytes equal an IPv4 slot, random timestamps, wire lengths near
2^32) redrawn so that every tested prefix length has groups and a five-tuple table rolled up to
masked five-tuples still has fewer groups than half its flows: the upper three IPv4 octets are
each one of 2 values (10 / 200: they differ in their first bit), the last octet one of 64; the
upper seven 16-bit groups of an IPv6 address are each one of 2 values (2001 / fe80), the last
keeps its low byte; source and destination port are each one of 2 values.  So /1, /8, /16,
/17, /20, /24, /25 and /31 (the lowest bit of the host octet) each merge some groups and not
others, as do /1, /16 ... /65, /97 and /127 on the IPv6 side.
"""
from __future__ import annotations

import ipaddress

import numpy as np

from exact_query_truth import tricky_stream

N = 60_000
OCTETS = np.array([10, 200], np.uint8)
GROUPS = np.array([[0x20, 0x01], [0xFE, 0x80]], np.uint8)
SPORTS, DPORTS = np.array([80, 443], np.uint16), np.array([53, 8080], np.uint16)
_CACHE = {}


def is_mapped(x):
    return (x[:, :10] == 0).all(1) & (x[:, 10:12] == 0xFF).all(1)


def redraw(x) -> None:
    """In place, a function of the address alone (so flows stay flows): the IPv4 bytes of a slot
    (4 bytes + 12 zero bytes, whichever ipver carries it) and of a mapped form octet by octet,
    every other 16-byte value group by group."""
    mapped = is_mapped(x)
    slot = (x[:, 4:] == 0).all(1) & ~mapped
    v6 = ~mapped & ~slot
    for rows, off in ((mapped, 12), (slot, 0)):
        x[rows, off:off + 3] = OCTETS[x[rows, off:off + 3] & 1]
        x[rows, off + 3] &= 0x3F
    for g in range(8):
        pick = (x[v6, 2 * g] ^ x[v6, 2 * g + 1]) & 1
        x[v6, 2 * g] = GROUPS[pick, 0]
        if g < 7:
            x[v6, 2 * g + 1] = GROUPS[pick, 1]


def prefix_stream(nflows=5000, seed=17, mapped=True):
    """(t, ipver, ts).  mapped=False: the IPv4-mapped arrivals rewritten to the 4-byte form."""
    key = (nflows, seed, mapped)
    if key not in _CACHE:
        t, ipver, ts = tricky_stream(seed, N, nflows)
        for a in ("src16", "dst16"):
            redraw(t[a])
        t["sport"] = SPORTS[t["sport"] & 1]
        t["dport"] = DPORTS[t["dport"] & 1]
        if not mapped:  # (tricky_stream maps whole packets: both addresses)
            m = is_mapped(t["src16"])
            assert np.array_equal(m, is_mapped(t["dst16"])) and (ipver[m] == 6).all()
            for a in ("src16", "dst16"):
                x = t[a]
                x[m, 0:4] = x[m, 12:16]
                x[m, 4:] = 0
            ipver[m] = 4
        _CACHE[key] = (t, ipver, ts)
    return _CACHE[key]


def bits_mask(bits: int, nbytes: int) -> np.ndarray:
    """The leading ``bits`` bits of an ``nbytes``-byte value, as bytes."""
    v = ((1 << bits) - 1) << (8 * nbytes - bits)
    return np.frombuffer(v.to_bytes(nbytes, "big"), np.uint8)


def mask_ips(x, ipver, v4: int, v6: int):
    """The prefix mask on the addresses packets carry: an ipver-4 slot in bytes 0..3, an
    IPv4-mapped 16-byte form in bytes 12..15, every other 16-byte form by the IPv6 rule."""
    x = x.copy()
    four = np.asarray(ipver) == 4
    mapped = is_mapped(x) & ~four
    other = ~four & ~mapped
    x[four, 0:4] &= bits_mask(v4, 4)
    x[mapped, 12:16] &= bits_mask(v4, 4)
    x[other] &= bits_mask(v6, 16)
    return x


def pair_of(v):
    """(IPv4 bits, IPv6 bits) of a prefix argument: None whole, a lone int the IPv4 length."""
    if v is None:
        return 32, 128
    return (int(v), 128) if isinstance(v, int) else (int(v[0]), int(v[1]))


def mask_packets(t, ipver, prefix):
    """The tuples with SrcIP / DstIP masked by ``prefix`` ({"SrcIP": (v4, v6), "DstIP": ...})."""
    out = dict(t)
    for name, col in (("SrcIP", "src16"), ("DstIP", "dst16")):
        if prefix and name in prefix:
            out[col] = mask_ips(t[col], ipver, *pair_of(prefix[name]))
    return out


def network_of(ip16: bytes, v4: int, v6: int) -> bytes:
    """The mask on one To16 value through Python's ipaddress network arithmetic."""
    a = ipaddress.IPv6Address(bytes(ip16))
    if a.ipv4_mapped is not None:
        net = ipaddress.ip_network((a.ipv4_mapped, v4), strict=False)
        return bytes(10) + b"\xff\xff" + net.network_address.packed
    return ipaddress.ip_network((a, v6), strict=False).network_address.packed


def classes_present(x, ipver) -> int:
    """Address classes among the To16 forms of the addresses: IPv4 (slots of ipver 4 and mapped
    forms) and everything else."""
    four = (np.asarray(ipver) == 4) | is_mapped(x)
    return int(four.any()) + int((~four).any())
