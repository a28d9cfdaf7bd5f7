"""Host side of the prefix roll-up, CIDR filters and hierarchical heavy hitters (no GPU): the C
ABI declares, exports and binds the calls, argument errors come before any device call,
mask_prefix agrees with Python's ipaddress network arithmetic, prefix_plan restates the
library's mask tables, make_filter parses CIDR strings, and the discounting step of hierarchical
heavy hitters is checked on handmade lists."""
import ctypes as ct
import ipaddress
import os
import re
import subprocess

import numpy as np
import pytest

from go2netspectra_amd import (ExactAggregator, ExactSpread, ExactTask, ExactView, _lib, discount_heavy_prefixes,
                               make_filter, make_prefix, mask_keys, mask_prefix, prefix_plan)
from go2netspectra_amd.exact import as_cidr, filter_key_bytes, ip_to16, parse_cidr
from prefix_truth import network_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
NAMES = ["gns_ex_rollup_prefix", "gns_spread_rollup_prefix", "gns_ex_aggregate_cidr", "gns_ex_view_aggregate_cidr"]


def test_library_declares_exports_and_binds_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r"\bT (gns_[a-z0-9_]+)", out))
    assert set(NAMES) <= set(_lib.EXPORTED)
    assert not [n for n in NAMES if n.startswith("gns_exs_") or n.startswith("gns_pairs_")]  # the pinned families
    txt = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    assert re.search(r"typedef struct gns_prefix \{ uint8_t src_v4, src_v6, dst_v4, dst_v6; \} gns_prefix;", txt)
    assert re.search(r"typedef struct gns_ex_cidr \{ gns_ex_filter f; uint8_t src_bits, dst_bits, _pad\[2\]; \} gns_ex_cidr;", txt)
    assert re.search(r"\bint gns_ex_rollup_prefix\(gns_ex \*dst, gns_ex \*src, const gns_prefix \*px, uint64_t out\[2\]\);", txt)
    assert re.search(r"\bint gns_spread_rollup_prefix\(gns_exs \*dst, gns_ex \*src, const gns_prefix \*flow_px, "
                     r"const gns_prefix \*elem_px,\s*uint64_t since, uint64_t \*cursor, uint64_t out\[2\]\);", txt)
    assert re.search(r"\bint gns_ex_aggregate_cidr\(gns_ex \*ex, const gns_ex_cidr \*filters, uint32_t nf, gns_ex_summary \*out", txt)
    assert re.search(r"\bint gns_ex_view_aggregate_cidr\(gns_ex_view \*v, const gns_ex_cidr \*f, uint32_t nf, gns_ex_summary \*out\);", txt)
    L = _lib.load()
    vp = ct.c_void_p
    assert L.gns_ex_rollup_prefix.argtypes == [vp, vp, vp, vp] and L.gns_ex_rollup_prefix.restype is ct.c_int
    assert L.gns_spread_rollup_prefix.argtypes == [vp, vp, vp, vp, ct.c_uint64, vp, vp]
    assert L.gns_ex_aggregate_cidr.argtypes == [vp, vp, ct.c_uint32, vp]
    assert L.gns_ex_view_aggregate_cidr.argtypes == [vp, vp, ct.c_uint32, vp]
    assert ct.sizeof(_lib.Prefix) == 4 and ct.sizeof(_lib.ExCidr) == 48 and _lib.ExCidr.src_bits.offset == 44
    for cls, names in ((ExactAggregator, ("rollup_from", "rollup", "spread", "hierarchical_heavy_hitters")),
                       (ExactTask, ("rollup", "spread", "hierarchical_heavy_hitters")), (ExactSpread, ("rollup_from",)),
                       (ExactView, ("aggregate",))):
        assert all(hasattr(cls, m) for m in names)


def test_argument_errors_come_before_any_device_call():
    L = _lib.load()
    out = (ct.c_uint64 * 2)(7, 9)
    cur = ct.c_uint64(5)
    h = ct.c_void_p(0x1000)  # never dereferenced: the argument checks come first
    full = _lib.Prefix(32, 128, 32, 128)
    # null handles, whatever the prefix
    for d, s in ((None, None), (None, h), (h, None)):
        assert L.gns_ex_rollup_prefix(d, s, ct.byref(full), out) == _lib.GNS_E_ARG
        assert b"null" in L.gns_last_error()
        assert L.gns_spread_rollup_prefix(d, s, ct.byref(full), ct.byref(full), 0, ct.byref(cur), out) == _lib.GNS_E_ARG
        assert b"null" in L.gns_last_error()
    # a null prefix
    assert L.gns_ex_rollup_prefix(h, h, None, out) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()
    assert L.gns_spread_rollup_prefix(h, h, None, ct.byref(full), 0, None, out) == _lib.GNS_E_ARG
    assert L.gns_spread_rollup_prefix(h, h, ct.byref(full), None, 0, None, out) == _lib.GNS_E_ARG
    # bits out of range, each of the four
    for bad in ((33, 128, 32, 128), (32, 129, 32, 128), (32, 128, 33, 128), (32, 128, 32, 129), (255, 255, 255, 255)):
        px = _lib.Prefix(*bad)
        assert L.gns_ex_rollup_prefix(h, h, ct.byref(px), out) == _lib.GNS_E_ARG
        assert b"prefix" in L.gns_last_error()
        assert L.gns_spread_rollup_prefix(h, h, ct.byref(px), ct.byref(full), 0, None, out) == _lib.GNS_E_ARG
        assert L.gns_spread_rollup_prefix(h, h, ct.byref(full), ct.byref(px), 0, None, out) == _lib.GNS_E_ARG
        assert b"prefix" in L.gns_last_error()
    assert (out[0], out[1], cur.value) == (7, 9, 5)
    # CIDR filters: null pointers, mask bits, bits above 128
    res = (_lib.ExSummary * 2)()
    flt = (_lib.ExCidr * 2)(as_cidr(make_filter(src_ip="1.2.3.4"), 120), as_cidr(make_filter()))
    for fn in (L.gns_ex_aggregate_cidr, L.gns_ex_view_aggregate_cidr):
        assert fn(None, flt, 2, res) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()
        assert fn(h, None, 2, res) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()
        assert fn(h, flt, 2, None) == _lib.GNS_E_ARG and b"null" in L.gns_last_error()
        flt[1].src_bits = 129
        assert fn(h, flt, 2, res) == _lib.GNS_E_ARG and b"bits" in L.gns_last_error()
        flt[1].src_bits, flt[1].dst_bits = 128, 200
        assert fn(h, flt, 2, res) == _lib.GNS_E_ARG and b"bits" in L.gns_last_error()
        flt[1].dst_bits = 128
        flt[1].f.mask = 1 << 9
        assert fn(h, flt, 2, res) == _lib.GNS_E_ARG and b"mask" in L.gns_last_error()
        flt[1].f.mask = 0


def random_ips(rng, n):
    """To16 values: IPv4, genuine IPv6, and the corner values of both classes."""
    x = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    x[: n // 2, :10] = 0
    x[: n // 2, 10:12] = 0xFF
    corner = ["0.0.0.0", "255.255.255.255", "::", "::1", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "::fffe:1.2.3.4",
              "0:0:0:0:0:ffff::", "::1:ffff:1.2.3.4", "128.0.0.1", "8000::"]
    return np.concatenate([x, np.array([list(ip_to16(c)) for c in corner], np.uint8)])


def test_mask_prefix_is_network_arithmetic_and_keeps_the_class():
    rng = np.random.default_rng(3)
    ips = random_ips(rng, 60)
    v4 = np.array([ipaddress.IPv6Address(bytes(r)).ipv4_mapped is not None for r in ips])
    assert v4.sum() >= 30 and (~v4).sum() >= 30
    for b6 in range(129):
        b4 = b6 % 33
        got = mask_prefix(ips, b4, b6)
        assert got.shape == ips.shape and got.dtype == np.uint8
        for r, g in zip(ips, got):
            assert g.tobytes() == network_of(r.tobytes(), b4, b6), (bytes(r).hex(), b4, b6)
        # only trailing bits go: a subset of the value's bits, the class kept, idempotent
        assert ((got & ~ips) == 0).all()
        assert np.array_equal(np.array([ipaddress.IPv6Address(bytes(r)).ipv4_mapped is not None for r in got]), v4)
        assert np.array_equal(mask_prefix(got, b4, b6), got)
    for b4 in range(33):  # every IPv4 length against every value, the IPv6 side whole
        got = mask_prefix(ips, b4, 128)
        assert all(g.tobytes() == network_of(r.tobytes(), b4, 128) for r, g in zip(ips, got))
    # nesting: a coarser mask over a finer one is the coarser one (coarser in both classes)
    for fine, coarse in (((24, 64), (16, 48)), ((31, 127), (1, 1)), ((17, 65), (17, 0)), ((32, 128), (0, 0)), ((9, 70), (9, 70))):
        assert np.array_equal(mask_prefix(mask_prefix(ips, *fine), *coarse), mask_prefix(ips, *coarse))
    # the ends of the range, and the range itself
    assert np.array_equal(mask_prefix(ips, 32, 128), ips)
    zero = mask_prefix(ips, 0, 0)
    assert set(map(bytes, zero)) == {ip_to16("0.0.0.0"), bytes(16)}
    for bad in ((33, 0), (0, 129), (-1, 0)):
        with pytest.raises(ValueError):
            mask_prefix(ips, *bad)
    assert mask_prefix(np.zeros((0, 16), np.uint8), 8, 8).shape == (0, 16)


def test_mask_keys_masks_the_ip_fields_of_a_layout_only():
    rng = np.random.default_rng(4)
    ips = random_ips(rng, 20)
    n = len(ips)
    keys = np.concatenate([rng.integers(0, 256, (n, 1), dtype=np.uint8), ips, ips[::-1]], axis=1)  # Protocol, SrcIP, DstIP
    got = mask_keys(keys, ["Protocol", "SrcIP", "DstIP"], {"SrcIP": (20, 56), "DstIP": 8})
    assert np.array_equal(got[:, 0], keys[:, 0])
    assert np.array_equal(got[:, 1:17], mask_prefix(ips, 20, 56))
    assert np.array_equal(got[:, 17:33], mask_prefix(ips[::-1], 8, 128))
    assert np.array_equal(mask_keys(keys, ["Protocol", "SrcIP", "DstIP"], None), keys)


def test_make_prefix_forms():
    def tup(px):
        return (px.src_v4, px.src_v6, px.dst_v4, px.dst_v6)
    assert tup(make_prefix(None)) == tup(make_prefix({})) == (32, 128, 32, 128)
    assert tup(make_prefix({"SrcIP": (24, 48), "DstIP": 16})) == (24, 48, 16, 128)  # a lone int: IPv4, IPv6 whole
    assert tup(make_prefix({"DstIP": (0, 0)})) == (32, 128, 0, 0)
    for bad in ({"SrcIP": 33}, {"SrcIP": (24, 129)}, {"DstIP": -1}, {"SrcPort": 8}, {"SrcIP": (1, 2, 3)}):
        with pytest.raises(ValueError):
            make_prefix(bad)


def expected_tables(dst_fields, prefix, encodeflow=False):
    """field / m4 / m6 per key byte from the definition, through integers instead of bytes."""
    px = {"SrcIP": (32, 128), "DstIP": (32, 128)}
    px.update({k: ((v, 128) if isinstance(v, int) else tuple(v)) for k, v in (prefix or {}).items()})
    field, m4, m6 = [], [], []
    for f in dst_fields:
        if f not in px:
            n = _lib.FIELD_SIZE[f]
            field += [2] * n
            m4 += [0xFF] * n
            m6 += [0xFF] * n
            continue
        v4, v6 = px[f]
        field += [0 if f == "SrcIP" else 1] * 16
        four = list((((1 << v4) - 1) << (32 - v4)).to_bytes(4, "big"))
        m4 += (four + [0xFF] * 12) if encodeflow else ([0xFF] * 12 + four)
        m6 += list((((1 << v6) - 1) << (128 - v6)).to_bytes(16, "big"))
    return field, m4, m6


CASES = [(FIVE, ["SrcIP"], {"SrcIP": (24, 48)}), (FIVE, ["SrcIP"], {"SrcIP": (0, 0)}), (FIVE, ["SrcIP"], {"SrcIP": (1, 1)}),
         (FIVE, ["SrcIP"], {"SrcIP": (17, 65)}), (FIVE, ["SrcIP"], {"SrcIP": (31, 127)}), (FIVE, ["SrcIP"], {"SrcIP": (8, 16)}),
         (FIVE, ["DstIP", "SrcIP", "SrcPort"], {"SrcIP": (16, 32), "DstIP": (25, 97)}),
         (["Protocol", "SrcIP", "DstIP"], ["SrcIP", "DstIP"], {"SrcIP": (20, 56), "DstIP": (20, 56)}),
         (FIVE, FIVE, {"SrcIP": (24, 64), "DstIP": (24, 64)}), (FIVE, ["SrcPort", "Protocol"], {"SrcIP": 8}),
         (FIVE, ["SrcIP", "SrcIP"], {"SrcIP": 24, "DstIP": 3}), (FIVE, FIVE, None)]


@pytest.mark.parametrize("src,dst,prefix", CASES, ids=[str(i) for i in range(len(CASES))])
def test_prefix_plan_tables(src, dst, prefix):
    from go2netspectra_amd import rollup_plan
    for enc in (False, True):
        g, field, m4, m6 = prefix_plan(src, dst, prefix, encodeflow=enc)
        assert g == rollup_plan(src, dst)
        assert (field, m4, m6) == expected_tables(dst, prefix, enc)
        assert len(g) == len(field) == len(m4) == len(m6) == sum(_lib.FIELD_SIZE[f] for f in dst)
    # the tables applied to keys are mask_prefix on the gathered fields
    rng = np.random.default_rng(6)
    K = sum(_lib.FIELD_SIZE[f] for f in src)
    keys = rng.integers(0, 256, (40, K), dtype=np.uint8)
    off = 0
    for f in src:
        if f in ("SrcIP", "DstIP"):
            keys[:20, off:off + 10] = 0
            keys[:20, off + 10:off + 12] = 0xFF
        off += _lib.FIELD_SIZE[f]
    g, field, m4, m6 = prefix_plan(src, dst, prefix)
    ipoff = {i: sum(_lib.FIELD_SIZE[f] for f in src[:src.index(name)]) for i, name in enumerate(("SrcIP", "DstIP")) if name in src}
    out = np.zeros((40, len(g)), np.uint8)
    for j in range(len(g)):
        if field[j] == 2:
            out[:, j] = keys[:, g[j]]
            continue
        o = ipoff[field[j]]
        v4 = (keys[:, o:o + 10] == 0).all(1) & (keys[:, o + 10:o + 12] == 0xFF).all(1)
        out[:, j] = keys[:, g[j]] & np.where(v4, m4[j], m6[j]).astype(np.uint8)
    assert np.array_equal(out, mask_keys(keys[:, g], dst, prefix))
    with pytest.raises(ValueError, match="DstIP"):
        prefix_plan(["SrcIP"], ["DstIP"], {"DstIP": 8})


def test_make_filter_parses_cidr_strings():
    f = make_filter(src_ip="10.1.0.0/16")
    assert isinstance(f, _lib.ExCidr) and (f.src_bits, f.dst_bits) == (112, 128)
    assert bytes(f.f.src16) == ip_to16("10.1.0.0") and f.f.mask == 1 << _lib.FIELD_IDS["SrcIP"]
    # host bits are kept as written and ignored by the match
    f = make_filter(src_ip="10.1.2.3/16", dst_ip="2001:db8::7/33", dst_port=53)
    assert (f.src_bits, f.dst_bits) == (112, 33) and bytes(f.f.src16) == ip_to16("10.1.2.3")
    assert bytes(f.f.dst16) == ip_to16("2001:db8::7") and f.f.dport == 53
    assert f.f.mask == sum(1 << _lib.FIELD_IDS[n] for n in ("SrcIP", "DstIP", "DstPort"))
    assert parse_cidr("1.2.3.4/0") == (ip_to16("1.2.3.4"), 96) and parse_cidr("::/0") == (bytes(16), 0)
    assert parse_cidr("1.2.3.4/32")[1] == 128 and parse_cidr("::ffff:1.2.3.0/120") == (ip_to16("1.2.3.0"), 120)
    # no length, or a full one: the plain filter
    for kw in (dict(src_ip="10.1.2.3"), dict(src_ip="10.1.2.3/32", dst_ip="::1/128"), dict(protocol=6), dict(src_ip=b"\x01\x02\x03\x04")):
        assert isinstance(make_filter(**kw), _lib.ExFilter)
    for bad in ("10.0.0.0/33", "::/129", "10.0.0.0/x", "/8"):
        with pytest.raises(ValueError):
            make_filter(src_ip=bad)
    # the key words a filter compares: partial-byte masks, the value masked too
    mask, value = filter_key_bytes(make_filter(src_ip="10.1.255.3/21"), ["Protocol", "SrcIP"])
    assert bytes(mask) == b"\x00" + b"\xff" * 14 + b"\xf8\x00"
    assert bytes(value) == b"\x00" + bytes(10) + b"\xff\xff\x0a\x01\xf8\x00"
    mask, value = filter_key_bytes(as_cidr(make_filter(src_ip="10.1.255.3"), 0), ["SrcIP"])
    assert not mask.any() and not value.any()
    assert filter_key_bytes(make_filter(dst_ip="10.0.0.0/8"), ["SrcIP"]) is None  # a field outside the layout
    plain = filter_key_bytes(make_filter(src_ip="10.1.255.3"), ["SrcIP"])
    wide = filter_key_bytes(as_cidr(make_filter(src_ip="10.1.255.3"), 128, 128), ["SrcIP"])
    assert all(np.array_equal(a, b) for a, b in zip(plain, wide))
    with pytest.raises(ValueError):
        as_cidr(make_filter(), 129)


def key(ip):
    return ip_to16(ip)


def test_discounting_of_hierarchical_heavy_hitters():
    levels = [(32, 128), (24, 64), (16, 48)]
    # one host carries its /24; the /24 has 3 more elsewhere; the /16 has a second heavy /24 and loose change
    lists = [
        (np.array([list(key("10.1.1.9"))], np.uint8), [12]),
        (np.array([list(key("10.1.1.0")), list(key("10.1.2.0"))], np.uint8), [15, 11]),
        (np.array([list(key("10.1.0.0")), list(key("10.2.0.0"))], np.uint8), [40, 10]),
    ]
    got = discount_heavy_prefixes(lists, levels, 10)
    assert got[0] == [(key("10.1.1.9"), 12, 12)]
    # 10.1.1.0/24: 15 - 12 = 3 -> heavy by its total alone, discounted away; 10.1.2.0/24 has no heavy host
    assert got[1] == [(key("10.1.2.0"), 11, 11)]
    # 10.1.0.0/16: the host (no reported /24 between) and the reported /24 discount it: 40 - 12 - 11 = 17
    assert got[2] == [(key("10.1.0.0"), 40, 17), (key("10.2.0.0"), 10, 10)]
    # at threshold 3 the /24 is reported and now stands between the host and the /16
    got = discount_heavy_prefixes(lists, levels, 3)
    assert got[1] == [(key("10.1.1.0"), 15, 3), (key("10.1.2.0"), 11, 11)]
    assert got[2] == [(key("10.1.0.0"), 40, 14), (key("10.2.0.0"), 10, 10)]
    # IPv6 rows go by the IPv6 lengths, and an IPv4 and an IPv6 prefix never meet
    six = [
        (np.array([list(key("2001:db8:0:1::5")), list(key("10.1.1.9"))], np.uint8), [20, 12]),
        (np.array([list(key("2001:db8:0:1::")), list(key("10.1.1.0"))], np.uint8), [26, 30]),
        (np.array([list(key("2001:db8::")), list(key("10.1.0.0"))], np.uint8), [26, 30]),
    ]
    got = discount_heavy_prefixes(six, levels, 10)
    assert got[1] == [(key("10.1.1.0"), 30, 18)]
    assert got[2] == []  # both /16-level rows are fully explained below
    # counts are Python ints beyond 2^63; the order of a list is kept
    big = [(np.array([list(key("1.1.1.1")), list(key("1.1.1.2"))], np.uint8), np.array([(1 << 63) + 5, 1 << 63], np.uint64)),
           (np.array([list(key("1.1.1.0"))], np.uint8), [(1 << 64) + 10])]
    got = discount_heavy_prefixes(big, [(32, 128), (24, 64)], 6)
    assert got[0] == [(key("1.1.1.1"), (1 << 63) + 5, (1 << 63) + 5), (key("1.1.1.2"), 1 << 63, 1 << 63)]
    assert got[1] == [] and all(isinstance(v, int) for row in got[0] for v in row[1:])
    # argument checks
    with pytest.raises(ValueError):
        discount_heavy_prefixes(lists, [(24, 64), (32, 128), (16, 48)], 10)  # not finest to coarsest
    with pytest.raises(ValueError):
        discount_heavy_prefixes(lists[:2], levels, 10)
    with pytest.raises(ValueError):
        discount_heavy_prefixes([], [], 10)


def test_go_binding_has_the_methods():
    src = open(os.path.join(ROOT, "integration", "go", "sketchgpu", "sketchgpu.go")).read()
    assert re.search(r"^type Prefix struct \{", src, re.M)
    assert re.search(r"^func \(e \*Exact\) RollupPrefixFrom\(src \*Exact, px Prefix\) \(projected, added uint64, err error\) \{", src, re.M)
    assert re.search(r"^type ExactCIDR struct \{", src, re.M)
    assert re.search(r"^func \(e \*Exact\) AggregateCIDR\(filters \[\]ExactCIDR\) \(\[\]ExactSummary, error\) \{", src, re.M)
    assert re.search(r"^func \(w \*ExactView\) AggregateCIDR\(filters \[\]ExactCIDR\) \(\[\]ExactSummary, error\) \{", src, re.M)
    # (the binding has no exact-spread handle, so gns_spread_rollup_prefix has no Go method, as gns_spread_rollup has none)
    for call in ("C.gns_ex_rollup_prefix(", "C.gns_ex_aggregate_cidr(", "C.gns_ex_view_aggregate_cidr("):
        assert call in src  # (test_go_binding.py checks each call's arity against the header)
