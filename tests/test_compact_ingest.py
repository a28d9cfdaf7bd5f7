"""Compact-record ingest, host side: gns_pack_pcap_compact_ts packs what
gns_pack_pcap_compact / _compact16 pack, with gns_pack_pcap_ts's timestamps; the
three gns_*_insert_compact calls check their arguments before any device call;
CompactBatch and HeaderBatch.compact on the host."""
import ctypes as ct
import os

import numpy as np
import pytest

import go2netspectra_amd as g
from go2netspectra_amd import _lib
from helpers import frame64, random_tuples


def mixed_frames(rng, n=400):
    """IPv4 and IPv6 frames, some behind a VLAN tag, and one ARP frame (no IP layer)."""
    t = random_tuples(rng, n, 60, v6_frac=0.25)
    frames = [frame64(t["src16"][i], t["dst16"][i], t["sport"][i], t["dport"][i], t["proto"][i], int(t["length"][i]),
                      v6=bool(t["v6"][i]), vlans=1 if i % 6 == 0 else 0) for i in range(n)]
    wl = [int(x) for x in t["length"]]
    arp = bytearray(64)
    arp[0:6], arp[6:12], arp[12:14] = b"\xff" * 6, b"\x00\x11\x22\x33\x44\x55", b"\x08\x06"
    frames.insert(n // 2, bytes(arp))
    wl.insert(n // 2, 64)
    assert t["v6"].any() and not t["v6"].all()
    return frames, wl


def write(tmp_path, kind, frames, wl):
    path = str(tmp_path / ("c." + kind))
    ts = 1_700_000_000_000_000_000 + np.arange(len(frames), dtype=np.int64) * 7000  # whole microseconds
    if kind == "pcap":
        g.write_pcap(path, frames, wl, snaplen=262144, ts_ns=ts)
    else:
        g.write_pcapng(path, frames, wl, ts_units=ts // 1000)
    return path


def pack_ts(path, cap, side_cap, rec_len):
    """gns_pack_pcap_compact_ts through ctypes: (r, rec, wl, ts, side, n_side, total, counts)."""
    L = g.load()
    rec, wl, ts = np.zeros((cap, 16), np.uint8), np.zeros(cap, np.uint32), np.zeros(cap, np.int64)
    side = np.zeros((max(side_cap, 1), 64), np.uint8)
    ns, total = ct.c_uint64(0), ct.c_uint64(0)
    r = L.gns_pack_pcap_compact_ts(os.fsencode(path), rec.ctypes.data, None if rec_len else wl.ctypes.data,
                                   ts.ctypes.data, cap, side.ctypes.data, side_cap, ct.byref(ns), ct.byref(total))
    cnt = (ct.c_uint64 * 3)()
    assert L.gns_pack_counts(cnt) == 0
    return r, rec, wl, ts, side, ns.value, total.value, list(cnt)


def pack_plain(path, cap, side_cap, rec_len):
    L = g.load()
    rec, wl = np.zeros((cap, 16), np.uint8), np.zeros(cap, np.uint32)
    side = np.zeros((max(side_cap, 1), 64), np.uint8)
    ns, total = ct.c_uint64(0), ct.c_uint64(0)
    if rec_len:
        r = L.gns_pack_pcap_compact16(os.fsencode(path), rec.ctypes.data, cap, side.ctypes.data, side_cap,
                                      ct.byref(ns), ct.byref(total))
    else:
        r = L.gns_pack_pcap_compact(os.fsencode(path), rec.ctypes.data, wl.ctypes.data, cap, side.ctypes.data,
                                    side_cap, ct.byref(ns), ct.byref(total))
    cnt = (ct.c_uint64 * 3)()
    assert L.gns_pack_counts(cnt) == 0
    return r, rec, wl, side, ns.value, total.value, list(cnt)


@pytest.mark.parametrize("kind", ["pcap", "pcapng"])
@pytest.mark.parametrize("rec_len", [False, True])
@pytest.mark.parametrize("limit", [None, 137])
def test_packer_with_timestamps_equals_the_packers_without(tmp_path, kind, rec_len, limit):
    frames, wl = mixed_frames(np.random.default_rng(20261019))
    path = write(tmp_path, kind, frames, wl)
    cap = limit or len(frames) + 5
    a = pack_ts(path, cap, 512, rec_len)
    b = pack_plain(path, cap, 512, rec_len)
    n = limit or len(frames)
    assert a[0] == b[0] == n and a[6] == b[5] == len(frames)           # written, total
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])   # records, wire lengths
    assert a[5] == b[4] > 0 and np.array_equal(a[4], b[3])             # n_side, side array
    assert a[7] == b[6] and sum(a[7]) == n                             # gns_pack_counts
    cls = a[1][:n, 13]
    assert (cls == 0).any() and (cls == 2).any() and ((cls == 1).any() or limit)
    hb = g.read_pcap(path, limit=limit)
    assert len(hb) == n and np.array_equal(a[3][:n], hb.ts)
    assert len(np.unique(hb.ts)) == n
    cb = g.read_pcap_compact(path, limit=limit, rec_len=rec_len, with_ts=True)
    assert isinstance(cb, g.CompactBatch) and len(cb) == n
    assert np.array_equal(cb.rec16, a[1][:n]) and np.array_equal(cb.ts, hb.ts) and np.array_equal(cb.side, a[4][:a[5]])
    assert (cb.wirelen is None) if rec_len else np.array_equal(cb.wirelen, hb.wirelen)
    tup = g.read_pcap_compact(path, limit=limit, rec_len=rec_len)  # the default return stays the tuple
    assert isinstance(tup, tuple) and np.array_equal(tup[0], cb.rec16)


def test_packer_range_errors(tmp_path):
    frames, wl = mixed_frames(np.random.default_rng(7), 40)
    big = write(tmp_path, "pcap", frames, [70_000] + wl[1:])
    r = pack_ts(big, 64, 64, True)
    assert r[0] == _lib.GNS_E_RANGE                       # the 16-byte form cannot hold 70000
    r = pack_ts(big, 64, 64, False)
    assert r[0] == len(frames) and r[2][0] == 70_000      # the 20-byte form does
    path = write(tmp_path, "pcapng", frames, wl)
    full = pack_ts(path, 64, 64, False)
    assert full[0] == len(frames) and full[5] > 1
    for rec_len in (False, True):
        r = pack_ts(path, 64, 1, rec_len)
        assert r[0] == _lib.GNS_E_RANGE and r[5] == full[5]   # *n_side = the count needed


def test_insert_compact_argument_errors_need_no_device():
    """Every argument error returns GNS_E_ARG before a device call: with a null handle
    (and each further bad argument beside it) nothing else can have been touched."""
    L = g.load()
    rec, side, ts = np.zeros((4, 16), np.uint8), np.zeros((1, 64), np.uint8), np.zeros(4, np.int64)
    R, S, T = rec.ctypes.data, side.ctypes.data, ts.ctypes.data
    for where in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for fn in (L.gns_ss_insert_compact, L.gns_spread_insert_compact):
            assert fn(None, R, None, 4, S, 1, where) == _lib.GNS_E_ARG       # null handle
            assert fn(None, None, None, 4, None, 0, where) == _lib.GNS_E_ARG  # null rec16, n > 0
            assert fn(None, R, None, 4, None, 1, where) == _lib.GNS_E_ARG    # n_side > 0, null side64
        ex = L.gns_ex_insert_compact
        assert ex(None, R, None, T, 4, S, 1, where) == _lib.GNS_E_ARG
        assert ex(None, None, None, T, 4, None, 0, where) == _lib.GNS_E_ARG
        assert ex(None, R, None, T, 4, None, 1, where) == _lib.GNS_E_ARG
        assert ex(None, R, None, None, 4, S, 1, where) == _lib.GNS_E_ARG     # null ts_ns
    assert b"null argument" in L.gns_last_error()


def test_compact_batch_on_the_host():
    rec = np.zeros((5, 16), np.uint8)
    cb = g.CompactBatch(rec, np.arange(5, dtype=np.uint32), np.zeros((0, 64), np.uint8))
    assert len(cb) == 5 and cb.ts is None and not cb.is_device()
    assert len(g.CompactBatch(rec[:0], None, None)) == 0
    hb = g.HeaderBatch(np.zeros((5, 64), np.uint8), np.full(5, 64, np.uint32))
    for rec_len in (False, True):
        with pytest.raises(ValueError):
            hb.compact(rec_len=rec_len)
