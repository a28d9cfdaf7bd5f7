"""Boundary corpus for the 64-byte record parser (parse_fast_ipv4 / parse_record /
parse_l3 in gns_device.cuh, or_parse_hdr64_len in the C oracle).

corpus()      -> [(name, record64, wirelen)]: one record per value of every decision
                 point of the parser, at 0, 1, 2 and 3 VLAN tags.  Names are
                 "group/tN/detail"; group() gives the first part.
mutants(n)    -> n seeded mutations of corpus records.
orderings()   -> the three record orders that exercise the wave ballot of
                 parse_record_fast, as (hdr [n, 64] u8, wirelen [n] u32, origin [n]):
                 origin[i] >= 0 is the index of record i in the input list, -1 - k
                 is filler record k of filler_pool().
Deterministic: no global state, fixed seeds.
"""
from __future__ import annotations

import struct

import numpy as np

MAC = bytes.fromhex("006677889aaa001122334455")
TAGS = {0: [], 1: [0x8100], 2: [0x88A8, 0x8100], 3: [0x8100, 0x88A8, 0x8100]}
V4S, V4D = bytes([10, 1, 2, 3]), bytes([192, 168, 7, 9])
V6S = bytes.fromhex("20010db8000100020003000400050006")
V6D = bytes.fromhex("fe80000000000000aabbccddeeff0011")
TUNNEL = (4789, 6081, 2152)
DROPPED_ETHERTYPES = (0x0806, 0x8035, 0x88CC, 0x8808, 0x888E, 0x88F7, 0x8863)
OTHER_ETHERTYPES = (0x8864, 0x8847, 0x8848, 0x0805, 0x0807, 0x0000, 0xFFFF, 0x05DC, 0x0600, 0x9100, 0x88B5)
SHORT_LENGTHS = (1, 63, 64, 65, 257)
BALLOT_LANES = (0, 1, 31, 32, 62, 63)


def l2len(tags: int) -> int:
    return 14 + 4 * tags


def record(tags: int, ethertype: int, l3: bytes, wirelen: int, tpids=None):
    b = bytearray(MAC)
    for i, tpid in enumerate(tpids or TAGS[tags]):
        b += struct.pack(">HH", tpid, 0x2000 | (5 + i))
    b += struct.pack(">H", ethertype)
    b += l3
    return bytes(b[:64]) + bytes(max(0, 64 - len(b))), wirelen


def l4(proto: int, sport: int, dport: int) -> bytes:
    """24 bytes of transport header: ports, and a TCP data offset of 5."""
    b = bytearray(24)
    b[0:4] = struct.pack(">HH", sport, dport)
    if proto == 6:
        b[4:12] = struct.pack(">II", 0x01020304, 0x05060708)
        b[12], b[13] = 0x50, 0x10
    else:
        b[4:6] = struct.pack(">H", 24)
    return bytes(b)


def ipv4(proto=6, tot=100, ihl=5, frag=0, ver=4, sport=40000, dport=443, src=V4S, dst=V4D) -> bytes:
    h = bytearray(20)
    h[0] = (ver & 15) << 4 | (ihl & 15)
    h[2:4] = struct.pack(">H", tot)
    h[4:6] = b"\x12\x34"
    h[6:8] = struct.pack(">H", frag)
    h[8], h[9] = 64, proto
    h[12:16], h[16:20] = src, dst
    return bytes(h) + l4(proto, sport, dport)


def ipv6(nh=6, plen=60, ver=6, sport=40000, dport=443, src=V6S, dst=V6D) -> bytes:
    h = bytearray(40)
    h[0] = (ver & 15) << 4
    h[4:6] = struct.pack(">H", plen)
    h[6], h[7] = nh, 64
    h[8:24], h[24:40] = src, dst
    return bytes(h) + l4(nh, sport, dport)


def preparsed(kind=1, sver=4, dver=4, src=V4S, dst=V4D, sport=4444, dport=5555, proto=6, wirelen=60):
    b = bytearray(64)
    b[0:12] = MAC
    b[12:16] = bytes([0x88, 0xB5, kind, sver])
    b[16:16 + len(src)] = src
    b[32:32 + len(dst)] = dst
    b[48:53] = struct.pack(">HHB", sport, dport, proto)
    b[53] = dver
    return bytes(b), wirelen


def corpus():
    out = []

    def add(name, rw):
        out.append((name, rw[0], rw[1]))

    for t in (0, 1, 2, 3):
        L = l2len(t)
        tn = f"t{t}"
        # IPv4: bytes on the wire after the L2 header (TSO and a total length that never binds)
        for n in (0, 1, 19, 20, 21, 27, 28, 39, 40, 41, 100):
            for tot in (0, 100):
                for proto in (6, 17, 1):
                    add(f"v4_after_l2/{tn}/n{n}_tot{tot}_p{proto}",
                        record(t, 0x0800, ipv4(proto, tot), L + n))
        # IPv4 total length (the wire never binds)
        for tot in (0, 19, 20, 21, 27, 28, 39, 40, 41, 60, 65535):
            for proto in (6, 17):
                add(f"v4_total/{tn}/tot{tot}_p{proto}", record(t, 0x0800, ipv4(proto, tot), L + 100))
        # IPv4 header length
        for ihl in range(16):
            for tot in (20, 24, 60, 100):
                add(f"v4_ihl/{tn}/ihl{ihl}_tot{tot}", record(t, 0x0800, ipv4(6, tot, ihl=ihl), L + 100))
        # IPv4 flags + fragment offset
        for frag in (0, 1, 0x1FFF, 0x2000, 0x3FFF, 0x4000, 0x6000, 0x8000, 0xA000, 0xC000):
            for proto in (6, 17, 1):
                add(f"v4_frag/{tn}/f{frag:04x}_p{proto}", record(t, 0x0800, ipv4(proto, 100, frag=frag), L + 100))
        # version nibble (gopacket does not check it under either ethertype)
        for ver in (0, 5, 6, 15):
            add(f"ip_version/{tn}/v4_{ver}", record(t, 0x0800, ipv4(6, 100, ver=ver), L + 100))
            add(f"ip_version/{tn}/v6_{ver}", record(t, 0x86DD, ipv6(6, 60, ver=ver), L + 100))
        # every protocol / next header
        for p in range(256):
            add(f"v4_proto/{tn}/p{p}", record(t, 0x0800, ipv4(p, 100), L + 100))
            add(f"v6_nexthdr/{tn}/p{p}", record(t, 0x86DD, ipv6(p, 60), L + 100))
        # tunnel ports and their neighbours, either side
        for port in TUNNEL:
            for d in (-1, 0, 1):
                for proto in (6, 17):
                    for side in ("s", "d"):
                        sp, dp = (port + d, 1234) if side == "s" else (1234, port + d)
                        add(f"tunnel_port/{tn}/v4_p{proto}_{side}{port + d}",
                            record(t, 0x0800, ipv4(proto, 100, sport=sp, dport=dp), L + 100))
                        add(f"tunnel_port/{tn}/v6_p{proto}_{side}{port + d}",
                            record(t, 0x86DD, ipv6(proto, 60, sport=sp, dport=dp), L + 100))
        # IPv6: bytes on the wire after the L2 header x payload length
        for n in (0, 39, 40, 41, 47, 48, 59, 60, 61, 100):
            for plen in (0, 7, 8, 19, 20, 21, 60, 65535):
                for nh in (6, 17, 58):
                    add(f"v6_after_l2/{tn}/n{n}_plen{plen}_nh{nh}", record(t, 0x86DD, ipv6(nh, plen), L + n))
        # ethertypes: the drop list and shapes left to the host packer
        for et in DROPPED_ETHERTYPES + OTHER_ETHERTYPES:
            add(f"ethertype/{tn}/{et:04x}", record(t, et, ipv4(6, 46), 60))
        # a wire shorter than the Ethernet header
        for wl in range(14):
            add(f"short_wire/{tn}/wl{wl}", record(t, 0x0800, ipv4(6, 100), wl))
        # tag protocol ids the other way round
        if t:
            tp = [0x88A8 if x == 0x8100 else 0x8100 for x in TAGS[t]]
            add(f"v4_after_l2/{tn}/swapped_tpids", record(t, 0x0800, ipv4(6, 100), L + 100, tpids=tp))
            add(f"v6_after_l2/{tn}/swapped_tpids", record(t, 0x86DD, ipv6(17, 60), L + 100, tpids=tp))
    # pre-parsed 0x88B5 records (the host packer's and the Thrift decoder's output)
    for kind in (0, 1, 2):
        add(f"preparsed/kind{kind}", preparsed(kind=kind))
    wide_s, wide_d = V6S, V6D
    for sv in (0, 4, 6, 7):
        for dv in (0, 4, 6, 7):
            add(f"preparsed/ver{sv}_{dv}_narrow", preparsed(sver=sv, dver=dv))
            add(f"preparsed/ver{sv}_{dv}_wide", preparsed(sver=sv, dver=dv, src=wide_s, dst=wide_d))
            add(f"preparsed/ver{sv}_{dv}_mixed", preparsed(sver=sv, dver=dv, src=V4S, dst=wide_d))
    for sp in (0, 0xFFFF):
        for dp in (0, 0xFFFF):
            add(f"preparsed/ports{sp}_{dp}", preparsed(sport=sp, dport=dp, proto=17))
    for wl in (0, 60, 65535, 65536, 70000):
        add(f"preparsed/wl{wl}", preparsed(wirelen=wl, proto=255))
    return out


def group(name: str) -> str:
    return name.split("/", 1)[0]


# header-significant byte values: ethertype and TPID halves, version/IHL bytes, protocol
# numbers, length boundaries, the halves of the tunnel ports (4789 = 0x12B5, 6081 = 0x17C1,
# 2152 = 0x0868), fragment-word masks
SIGNIFICANT = (0x00, 0x01, 0x04, 0x05, 0x06, 0x08, 0x11, 0x12, 0x14, 0x17, 0x1F, 0x20, 0x28, 0x29, 0x2B, 0x2C,
               0x2F, 0x33, 0x3A, 0x3C, 0x3F, 0x40, 0x45, 0x46, 0x4F, 0x60, 0x68, 0x81, 0x86, 0x88, 0x89, 0xA8,
               0xB5, 0xC1, 0xDD, 0xFF)


def mutants(n: int, seed: int = 20261019, base=None):
    """n mutations of corpus records: 1-3 bytes in 12..61 changed (each changed byte random
    or header-significant with equal odds); the wire length redrawn from 0..79 for 30 % of
    them and from 0..2999 for 10 %."""
    base = corpus() if base is None else base
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        name, rec, wl = base[int(rng.integers(0, len(base)))]
        b = bytearray(rec)
        for _ in range(int(rng.integers(1, 4))):
            pos = int(rng.integers(12, 62))
            if rng.random() < 0.5:
                b[pos] = int(rng.integers(0, 256))
            else:
                b[pos] = SIGNIFICANT[int(rng.integers(0, len(SIGNIFICANT)))]
        u = rng.random()
        if u < 0.3:
            wl = int(rng.integers(0, 80))
        elif u < 0.4:
            wl = int(rng.integers(0, 3000))
        out.append((f"mutant/{i}/{name}", bytes(b), wl))
    return out


def frame_of(rec: bytes, wirelen: int) -> bytes:
    """The frame whose first 64 bytes and wire length the record states: cut to the wire
    length, or extended with zeros to it."""
    return rec[:wirelen] + bytes(max(0, wirelen - 64))


def filler_pool(n: int = 509, seed: int = 7):
    """Fast-shape records (untagged IPv4, IHL 5, TCP >= 20 bytes or UDP >= 8 bytes without a
    tunnel port): (hdr [n, 64], wirelen [n])."""
    rng = np.random.default_rng(seed)
    hdr = np.zeros((n, 64), np.uint8)
    hdr[:, 0:12] = np.frombuffer(MAC, np.uint8)
    hdr[:, 12] = 0x08
    wl = rng.integers(64, 1515, n).astype(np.uint32)
    tot = wl - 14
    tot[::7] = 0  # TSO
    hdr[:, 14] = 0x45
    hdr[:, 16], hdr[:, 17] = tot >> 8, tot & 0xFF
    hdr[::5, 20] = 0x40  # DF
    hdr[1::5, 20] = 0x80  # the reserved bit
    hdr[:, 22] = 64
    udp = rng.random(n) < 0.4
    hdr[:, 23] = np.where(udp, 17, 6)
    hdr[:, 26:34] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    ports = rng.integers(0, 65536, (n, 2))
    ports[np.isin(ports, TUNNEL)] = 1000
    hdr[:, 34:38] = ports.astype(">u2").view(np.uint8).reshape(n, 4)
    hdr[:, 38:46] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    hdr[~udp, 46] = 0x50
    return hdr, wl


def to_arrays(records):
    hdr = np.frombuffer(b"".join(r for _, r, _ in records), np.uint8).reshape(len(records), 64).copy()
    wl = np.array([w for _, _, w in records], np.uint64).astype(np.uint32)
    return hdr, wl


def _gather(origin, hdr, wl, fh, fw):
    o = np.asarray(origin, np.int64)
    fill = o < 0
    oh = np.empty((len(o), 64), np.uint8)
    ow = np.empty(len(o), np.uint32)
    oh[~fill], ow[~fill] = hdr[o[~fill]], wl[o[~fill]]
    oh[fill], ow[fill] = fh[-1 - o[fill]], fw[-1 - o[fill]]
    return oh, ow, o


def orderings(hdr, wl, tail: int = 100):
    """{"slow": as generated (every lane of every wave takes the general decoder),
        "lane": one input record per 64 records of filler, its lane stepping through
                BALLOT_LANES (one slow lane in an otherwise fast wave),
        "tail": a whole 256-record block of filler, then `tail` input records, then filler
                up to the next multiple of 256, repeated; the last unit ends with its
                input records (blocks and waves that never run the general decoder next
                to ones that do, and a ragged last block)}"""
    fh, fw = filler_pool()
    n, F = len(wl), len(fw)
    out = {"slow": (hdr, wl, np.arange(n, dtype=np.int64))}
    o = -1 - (np.arange(n * 64, dtype=np.int64) % F)
    lanes = np.array(BALLOT_LANES, np.int64)[np.arange(n) % len(BALLOT_LANES)]
    o[np.arange(n, dtype=np.int64) * 64 + lanes] = np.arange(n)
    out["lane"] = _gather(o, hdr, wl, fh, fw)
    parts, k = [], 0
    for i in range(0, n, tail):
        m = min(tail, n - i)
        parts.append(-1 - ((k + np.arange(256, dtype=np.int64)) % F))
        parts.append(np.arange(i, i + m, dtype=np.int64))
        k += 256
        if i + m < n:  # keep the next filler block aligned to 256 records
            parts.append(-1 - ((k + np.arange(256 - m % 256, dtype=np.int64)) % F))
            k += 256
    out["tail"] = _gather(np.concatenate(parts), hdr, wl, fh, fw)
    return out
