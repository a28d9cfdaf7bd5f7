"""Host side of the exact query plane (no GPU): filter construction, the Querier's argument
errors, merge_summaries, and the two C structs' layout."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from go2netspectra_amd import Summary, _lib, make_filter, merge_summaries
from go2netspectra_amd.exact import (ExactTask, check_filter, filter_fields, filter_from_flow_keys, filter_key_bytes,
                                     ip_to16)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT = {f: 1 << i for f, i in _lib.FIELD_IDS.items()}


def test_struct_sizes_match_the_header():
    assert ct.sizeof(_lib.ExFilter) == 44 and ct.sizeof(_lib.ExSummary) == 56
    assert _lib.ExFilter.src16.offset == 4 and _lib.ExFilter.dst16.offset == 20
    assert _lib.ExFilter.sport.offset == 36 and _lib.ExFilter.dport.offset == 38 and _lib.ExFilter.proto.offset == 40
    assert [f[0] for f in _lib.ExSummary._fields_] == ["flows", "packets", "bytes", "first_ns", "last_ns",
                                                       "max_packets", "max_bytes"]
    # the header declares the same members in the same order
    txt = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    body = re.search(r"typedef struct gns_ex_summary \{(.*?)\} gns_ex_summary;", txt, re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == [f[0] for f in _lib.ExSummary._fields_]
    body = re.search(r"typedef struct gns_ex_filter \{(.*?)\} gns_ex_filter;", txt, re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?\s*[,;]", body) == [f[0] for f in _lib.ExFilter._fields_]
    assert {"gns_ex_aggregate", "gns_ex_heavy_hitters"} <= set(_lib.EXPORTED)


def test_ip_spellings_are_one_filter():
    want = bytes(10) + b"\xff\xff" + bytes([1, 2, 3, 4])
    for ip in ("1.2.3.4", "::ffff:1.2.3.4", "::FFFF:102:304", "0:0:0:0:0:ffff:0102:0304", bytes([1, 2, 3, 4]), want):
        f = make_filter(src_ip=ip, dst_ip=ip)
        assert bytes(f.src16) == want and bytes(f.dst16) == want, ip
        assert f.mask == BIT["SrcIP"] | BIT["DstIP"]
    v6 = bytes.fromhex("20010db8000000000000000000000001")
    for ip in ("2001:db8::1", "2001:0db8:0000:0000:0000:0000:0000:0001", "2001:DB8:0:0::1", v6):
        assert bytes(make_filter(dst_ip=ip).dst16) == v6
    # an IPv6 address whose first four bytes look like an IPv4 slot stays what it is
    assert ip_to16("102:304::") == bytes([1, 2, 3, 4]) + bytes(12) != want
    for bad in ("1.2.3", "1.2.3.4.5", "2001:db8::g", b"\x01\x02\x03"):
        with pytest.raises(ValueError):
            make_filter(src_ip=bad)


def test_ports_protocol_and_open_fields():
    f = make_filter()
    assert f.mask == 0 and filter_fields(f) == []
    f = make_filter(src_ip="", dst_ip=None)  # the reference's empty string: no constraint
    assert f.mask == 0
    f = make_filter(src_port=0, dst_port=65535, protocol=0)
    assert (f.sport, f.dport, f.proto) == (0, 65535, 0)
    assert f.mask == BIT["SrcPort"] | BIT["DstPort"] | BIT["Protocol"]
    assert filter_fields(f) == ["SrcPort", "DstPort", "Protocol"]
    assert make_filter(dst_port="443").dport == 443
    for kw in (dict(src_port=-1), dict(dst_port=65536), dict(protocol=256), dict(protocol=-1)):
        with pytest.raises(ValueError):
            make_filter(**kw)


def test_filter_key_bytes_follow_the_layout():
    f = make_filter(src_ip="10.0.0.7", dst_port=0x1F90, protocol=17)
    m, v = filter_key_bytes(f, ["SrcPort", "Protocol", "DstIP", "DstPort"]) or (None, None)
    assert m is None  # SrcIP is not part of that key
    f = make_filter(dst_ip="10.0.0.7", dst_port=0x1F90, protocol=17)
    m, v = filter_key_bytes(f, ["SrcPort", "Protocol", "DstIP", "DstPort"])
    assert len(m) == len(v) == 21
    assert list(m) == [0, 0] + [255] * 19  # Protocol at byte 2, the IP at byte 3, the port at byte 19
    assert bytes(v) == b"\0\0" + b"\x11" + ip_to16("10.0.0.7") + b"\x1f\x90"
    m, v = filter_key_bytes(make_filter(src_ip="::1"), ["Protocol", "SrcIP"])
    assert list(m) == [0] + [255] * 16 and bytes(v) == b"\0" + ip_to16("::1")  # an IP at byte 1
    m, v = filter_key_bytes(make_filter(), ["SrcIP"])
    assert not m.any() and not v.any()  # mask == 0 matches every flow
    assert filter_key_bytes(make_filter(protocol=6), ["SrcIP"]) is None  # field not in the key: no flow


def test_bad_mask_is_rejected():
    f = make_filter(protocol=6)
    check_filter(f)
    for bits in (1, 1 << 6, 1 << 31):
        f.mask = BIT["Protocol"] | bits
        with pytest.raises(ValueError):
            check_filter(f)
        with pytest.raises(ValueError):
            filter_key_bytes(f, ["Protocol"])


def test_unsupported_flow_key_and_end_time():
    f = filter_from_flow_keys({"SrcIP": "1.2.3.4", "DstPort": "443", "Protocol": "6"})
    assert filter_fields(f) == ["SrcIP", "DstPort", "Protocol"] and f.dport == 443 and f.proto == 6
    with pytest.raises(ValueError, match="^unsupported flow key: TaskName$"):
        filter_from_flow_keys({"SrcIP": "1.2.3.4", "TaskName": "x"})
    with pytest.raises(ValueError, match="^unsupported flow key: srcip$"):
        filter_from_flow_keys({"srcip": "1.2.3.4"})
    # the argument errors come before any device work: a task object without a handle shows them
    task = ExactTask.__new__(ExactTask)
    task.name_, task.key_fields, task.agg = "t", ["SrcIP"], None
    with pytest.raises(ValueError, match="^unsupported flow key: Bytes$"):
        task.trace_flow({"Bytes": "1"})
    with pytest.raises(ValueError, match="end_time"):
        task.trace_flow({"SrcIP": "1.2.3.4"}, end_time=1_700_000_000)
    with pytest.raises(ValueError, match="end_time"):
        task.aggregate_flows(src_ip="1.2.3.4", end_time=1_700_000_000)
    with pytest.raises(ValueError, match="end_time"):
        task.aggregate_flows_many([dict(protocol=6), dict(protocol=17, end_time=5)])
    with pytest.raises(ValueError, match="end_time"):
        task.heavy_hitters(0, 10, end_time=0)
    assert task.heavy_hitters(0, 0) == [] and task.heavy_hitters(5, 10) == []  # LIMIT 0, unknown Type


def test_merge_summaries():
    assert merge_summaries([]) == Summary()
    assert merge_summaries([Summary(), Summary()]) == Summary()
    a = Summary(3, 10, 1000, -50, -20, 6, 700)
    b = Summary(2, 7, (1 << 64) - 500, -30, -10, 5, (1 << 64) - 900)
    assert merge_summaries([a]) == a
    # empty shards carry 0 timestamps that are not observations: with all-negative times
    # they would otherwise win the max
    got = merge_summaries([Summary(), a, Summary(), b, Summary()])
    assert got == Summary(5, 17, 500, -50, -10, 6, (1 << 64) - 900)
    pos = Summary(1, 1, 1, 100, 200, 1, 1)
    assert merge_summaries([Summary(), pos]) == pos  # ... and the min with positive ones
    assert merge_summaries([pos, a]) == Summary(4, 11, 1001, -50, 200, 6, 700)
    rng = np.random.default_rng(0)
    parts = [Summary(int(f), int(p), int(by), int(s), int(s + d), int(mp), int(mb)) for f, p, by, s, d, mp, mb in
             zip(rng.integers(0, 3, 40), rng.integers(0, 1 << 62, 40), rng.integers(0, 1 << 62, 40),
                 rng.integers(-(1 << 40), 1 << 40, 40), rng.integers(0, 1 << 30, 40), rng.integers(1, 1 << 40, 40),
                 rng.integers(1, 1 << 40, 40))]
    live = [p for p in parts if p.flows]
    got = merge_summaries(parts)
    m = (1 << 64) - 1
    assert got == Summary(sum(p.flows for p in live), sum(p.packets for p in live) & m, sum(p.bytes for p in live) & m,
                          min(p.first_ns for p in live), max(p.last_ns for p in live),
                          max(p.max_packets for p in live), max(p.max_bytes for p in live))
    assert merge_summaries(parts[::-1]) == got
