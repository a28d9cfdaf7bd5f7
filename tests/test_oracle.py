"""CPU: the oracle pinned against the golden vectors, and the two independent
restatements (C oracle vs pure-Python pyref) against each other."""
import json
import os

import numpy as np
import pytest

from oracle import pyref
from helpers import sizes_u32, zipf_keys

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_mm3_public_kats(oracle):
    kat = json.load(open(os.path.join(GOLD, "mm3_kat.json")))
    for v in kat["vectors"]:
        d = bytes.fromhex(v["data"])
        want = int(v["hash"], 16)
        assert oracle.mm3(d, v["seed"]) == want
        assert pyref.mm3(d, v["seed"]) == want


@pytest.mark.parametrize("h", ["c", "py"])
def test_mm3_smhasher_verification(oracle, h):
    fn = oracle.mm3 if h == "c" else pyref.mm3
    key = bytearray(256)
    hashes = bytearray()
    for i in range(256):
        key[i] = i
        hashes += fn(bytes(key[:i]), 256 - i).to_bytes(4, "little")
    want = int(json.load(open(os.path.join(GOLD, "mm3_kat.json")))["smhasher_verification"], 16)
    assert fn(bytes(hashes), 0) == want


def test_mm3_random_c_vs_python(oracle):
    rng = np.random.default_rng(1)
    for n in list(range(0, 40)) + [74]:
        for _ in range(5):
            d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            s = int(rng.integers(0, 2**32))
            assert oracle.mm3(d, s) == pyref.mm3(d, s)


def test_hand_traces(oracle):
    """count_min.go state machine, hand-derived expectations (tests/golden/cm_traces.json)."""
    tr = json.load(open(os.path.join(GOLD, "cm_traces.json")))
    for t in tr["traces"]:
        c = oracle.CountMin(1, 1, 1, 1, 4, np.array([7], np.uint32))
        for (k, s), st in zip(t["updates"], t["states"]):
            c.insert_keys(np.frombuffer(k.encode(), np.uint8).reshape(1, 4), np.array([s], np.uint32))
            C, S, Fc, Fs = c.export()
            assert [int(C[0]), bytes(Fc[0]).decode(), int(S[0]), bytes(Fs[0]).decode()] == st, t["name"]


def test_parse_vectors(oracle):
    pv = json.load(open(os.path.join(GOLD, "parse_vectors.json")))
    for v in pv["vectors"]:
        st, src, dst, sp, dp, pr = oracle.parse_hdr64(bytes.fromhex(v["record"]), v["wirelen"])
        assert st == v["status"], v["name"]
        if st == 0:
            assert (src.hex(), dst.hex(), sp, dp, pr) == (v["src16"], v["dst16"], v["sport"], v["dport"],
                                                          v["proto"]), v["name"]


@pytest.mark.parametrize("w,d,K,nflows,n", [(16, 2, 4, 30, 3000), (64, 3, 13, 200, 5000), (7, 4, 37, 50, 4000),
                                            (1, 1, 0, 1, 500)])
def test_countmin_c_vs_python(oracle, w, d, K, nflows, n):
    rng = np.random.default_rng(w + K)
    keys, flows, _ = zipf_keys(rng, n, nflows, K)
    sizes = sizes_u32(rng, n, big_frac=0.02)
    seeds = rng.integers(0, 2**32, d, dtype=np.uint64).astype(np.uint32)
    c = oracle.CountMin(w, d, 500, 5, K, seeds)
    c.insert_keys(keys, sizes)
    p = pyref.CountMinSeq(w, d, 500, 5, K, seeds.tolist())
    for k, s in zip(keys, sizes):
        p.insert(bytes(k), int(s))
    C, S, Fc, Fs = c.export()
    assert C.tolist() == p.C and S.tolist() == p.S
    assert [bytes(x) for x in Fc] == p.Fc and [bytes(x) for x in Fs] == p.Fs
    for f in flows[:50]:
        assert c.query(bytes(f)) == p.query(bytes(f))
    assert c.heavy("count") == p.heavy("count") and c.heavy("size") == p.heavy("size")


def test_superspread_c_vs_python(oracle):
    rng = np.random.default_rng(3)
    flows = rng.integers(0, 256, (20, 16), dtype=np.uint8)
    fl = flows[rng.integers(0, 20, 2000)]
    el = rng.integers(0, 256, (2000, 8), dtype=np.uint8)
    seeds = np.array([5, 6, 7], np.uint32)
    c = oracle.SuperSpread(32, 3, 10, 16, 5, 0.5, 1.08, 16, 8, seeds, 99, 1234)
    c.insert(fl, el)
    p = pyref.SuperSpreadSeq(32, 3, 10, 16, 5, 0.5, 1.08, 16, 8, seeds.tolist(), 99, 1234)
    for f, e in zip(fl, el):
        p.insert(bytes(f), bytes(e))
    values, keys, regs, pbits = c.export()
    assert values.tolist() == p.values
    assert [bytes(k) for k in keys] == p.keys
    assert regs.tolist() == p.regs
    assert pbits.tolist() == p.pbits
    assert c.heavy() == p.heavy()
    for f in flows:
        assert c.query(bytes(f)) == p.query(bytes(f))


def test_go_pow_integer_path(oracle):
    L = oracle.lib()
    for base in (0.5, 1.08, 2.0, 0.9, 1.5):
        for e in list(range(-80, 81)) + [-1000, -5000, 300]:
            got = L.or_go_pow(base, float(e))
            assert got == pyref.go_pow_int(base, float(e))
            if base in (0.5, 2.0) and abs(e) <= 1000:
                assert got == base ** e  # powers of two are exact under any algorithm


def test_golden_streams_reproduced(oracle):
    z = np.load(os.path.join(GOLD, "cm_stream.npz"))
    w, d, st, ct, K = (int(x) for x in z["params"])
    c = oracle.CountMin(w, d, st, ct, K, z["seeds"])
    c.insert_keys(z["keys"], z["sizes"])
    C, S, Fc, Fs = c.export()
    assert np.array_equal(C, z["C"]) and np.array_equal(S, z["S"])
    assert np.array_equal(Fc, z["FPc"]) and np.array_equal(Fs, z["FPs"])
    assert [v for _, v in c.heavy("count")] == z["hh_count"].tolist()
    s = np.load(os.path.join(GOLD, "ss_stream.npz"))
    w, d, thr, m, size, kf, ke = (int(x) for x in s["params"])
    base, b = (float(x) for x in s["fparams"])
    hm, rs = (int(x) for x in s["seeds64"])
    ss = oracle.SuperSpread(w, d, thr, m, size, base, b, kf, ke, s["seeds"], hm, rs)
    ss.insert(s["flows"], s["elems"])
    values, keys, regs, pbits = ss.export()
    assert np.array_equal(values, s["values"]) and np.array_equal(regs, s["regs"])
    assert np.array_equal(pbits, s["pbits"]) and np.array_equal(keys, s["keys"])


def test_det_log_c_python_and_accuracy(oracle):
    """The deterministic log behind the declared geometric waiting times:
    C and Python round identically, and both stay within 2 ulp of libm."""
    from oracle import pyref
    import math
    rng = np.random.default_rng(17)
    xs = np.concatenate([rng.random(3000), 1.0 - rng.random(500) * 1e-9, [1.0, 0.5, 2.0 ** -53, 0.70710678118654752]])
    xs = xs[xs > 0]
    for x in xs:
        c = oracle.lib().or_det_log(float(x))
        assert c == pyref.det_log(float(x))
        assert abs(c - math.log(x)) <= 2 * math.ulp(math.log(x)) + 1e-300
    for p in np.concatenate([rng.random(1000) * 1e-3, rng.random(1000), [1e-300, 1e-17, 1e-4, 0.999999]]):
        c = oracle.lib().or_det_log1m(float(p))
        assert c == pyref.det_log1m(float(p))
        assert abs(c - math.log1p(-p)) <= 1e-12 * abs(math.log1p(-p))


def _same_bits(c, py, what):
    py = np.array(py, np.float64)
    bad = np.nonzero(c.view(np.uint64) != py.view(np.uint64))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} differ, first at {bad[0]}: C={c[bad[0]]!r} pyref={py[bad[0]]!r}"


def test_gomath_grids_c_vs_python(oracle):
    """The grids the device helpers are compared on (gomath_grids.py, test_gomath_gpu.py): the C
    oracle's side of that comparison equals pyref, the second restatement, bit for bit -- b^+-v
    up to v = 12000 into the subnormal band and underflow, ldexp / frexp around their thresholds,
    the log at its reduction boundary and the powers of two, log1m around its series cut, the
    generator at packet indices around 2^27, 2^32 and 2^63."""
    import math

    import gomath_grids as G
    x, y = G.pow_grid()
    _same_bits(oracle.gomath_eval(oracle.GM_POW, x, y), [pyref.go_pow_int(a, b) for a, b in zip(x.tolist(), y.tolist())],
               "go_pow")
    x, e = G.ldexp_grid()

    def py_ldexp(f, k):
        try:
            return math.ldexp(f, k)
        except OverflowError:
            return math.copysign(math.inf, f)
    c = oracle.gomath_eval(oracle.GM_LDEXP, x, G.as_f64(e.view(np.uint64)))
    _same_bits(c, [py_ldexp(f, k) for f, k in zip(x.tolist(), e.tolist())], "go_ldexp")
    fx = np.unique(np.concatenate([x, c]))
    cf, ce = oracle.gomath_eval(oracle.GM_FREXP, fx)
    pf = [math.frexp(v) for v in fx.tolist()]
    _same_bits(cf, [f for f, _ in pf], "go_frexp")
    assert ce.tolist() == [k for _, k in pf]
    x = G.log_grid()
    _same_bits(oracle.gomath_eval(oracle.GM_LOG, x), [pyref.det_log(v) for v in x.tolist()], "det_log")
    p = G.log1m_grid()
    _same_bits(oracle.gomath_eval(oracle.GM_LOG1M, p), [pyref.det_log1m(v) for v in p.tolist()], "det_log1m")
    pk, rd = G.uniform_grid()
    c = oracle.gomath_eval(oracle.GM_UNIFORM, G.as_f64(pk), G.as_f64(rd), seed=G.UNIFORM_SEED)
    _same_bits(c, [pyref.ss_uniform(G.UNIFORM_SEED, a, b >> 32, b & 0xFFFFFFFF) for a, b in zip(pk.tolist(), rd.tolist())],
               "ss_uniform")
    cells = G.cells_grid()
    c = oracle.gomath_eval(oracle.GM_HLL_SEEDS, G.as_f64(cells), seed=G.HLL_MASTER).view(np.uint64)
    want = [s1 << 32 | s0 for s0, s1 in (pyref.hll_seeds(G.HLL_MASTER, v) for v in cells.tolist())]
    assert c.tolist() == want


def _ipv6_zero_runs(rng, n):
    """IPv6 slots with random runs of zero groups (RFC 5952 '::' selection cases)."""
    out = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    for i in range(n):
        g = rng.integers(0, 8)
        ln = rng.integers(0, 9 - g)
        out[i, 2 * g:2 * (g + ln)] = 0
        if rng.random() < 0.2:
            out[i, :10] = 0
            out[i, 10:12] = 0xFF  # IPv4-mapped: prints dotted
        if rng.random() < 0.1:
            out[i, 2:4] = 0
    return out


def test_exact_key_strings_c_vs_python(oracle):
    """Go key strings (net.IP.String + strings.Join) from the C exact oracle equal the
    host's rebuild from canonical bytes (go2netspectra_amd.exact.key_string)."""
    from go2netspectra_amd.exact import key_string
    rng = np.random.default_rng(5)
    n = 3000
    src = _ipv6_zero_runs(rng, n)
    dst = _ipv6_zero_runs(rng, n)
    v4 = rng.random(n) < 0.3
    src[v4, 4:] = 0
    dst[v4, 4:] = 0
    sport = rng.integers(0, 65536, n).astype(np.uint16)
    dport = rng.integers(0, 65536, n).astype(np.uint16)
    proto = rng.integers(0, 256, n).astype(np.uint8)
    ipver = np.where(v4, 4, 6).astype(np.uint8)
    fields = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
    ex = oracle.Exact(fields)
    ex.insert_tuples(src, dst, sport, dport, proto, ipver, np.ones(n, np.uint32), np.arange(n))
    got = set(ex.export())
    want = set()
    for i in range(n):
        s16, d16 = bytes(src[i]), bytes(dst[i])
        if v4[i]:  # To16 of a 4-byte net.IP
            s16 = bytes(10) + b"\xff\xff" + s16[:4]
            d16 = bytes(10) + b"\xff\xff" + d16[:4]
        key = s16 + d16 + int(sport[i]).to_bytes(2, "big") + int(dport[i]).to_bytes(2, "big") + bytes([proto[i]])
        want.add(key_string(key, fields)[0])
    assert got == want


def test_thrift_golden_vectors(oracle):
    """packetcodec_test.go: the legacy protobuf payload (:123) is rejected; the
    round-trip values (:13-98, net.ParseIP -> 16-byte forms) decode back."""
    from go2netspectra_amd.thrift import marshal_packet_info, pack_messages
    import ipaddress
    legacy = bytes.fromhex("0a060880e2cfaa0612140a04c000020a1204c633641418bb0320fb412806188001")
    m1 = marshal_packet_info(1700000000 * 10**9 + 123, bytes(10) + b"\xff\xff" + ipaddress.ip_address("192.0.2.10").packed,
                             ipaddress.ip_address("2001:db8::1").packed, 443, 8080, 17, 128)
    m2 = marshal_packet_info(1700000010 * 10**9 + 456, bytes(10) + b"\xff\xff" + bytes([198, 51, 100, 1]),
                             ipaddress.ip_address("2001:db8::2").packed, 53000, 8443, 6, 256)
    buf, offs = pack_messages([legacy, m1, m2, b"", b"\x00"])
    out = oracle.thrift_decode(buf, offs)
    assert out["ok"].tolist() == [0, 1, 1, 0, 0]  # b"" (EOF) and a bare STOP (missing fields) fail
    assert bytes(out["dst16"][1]) == ipaddress.ip_address("2001:db8::1").packed
    assert out["sport"][1] == 443 and out["dport"][1] == 8080 and out["proto"][1] == 17
    assert out["length"][1] == 128 and out["ts"][1] == 1700000000 * 10**9 + 123
    assert out["sver"][1] == 6 and out["dver"][2] == 6
    assert out["sport"][2] == 53000 and out["length"][2] == 256
    # the canonical 4-byte-IP message is 70 bytes
    assert len(marshal_packet_info(0, b"\1\2\3\4", b"\5\6\7\10", 1, 2, 6, 60)) == 70


def test_thrift_decode_c_vs_python(oracle):
    """C restatement (recursive Skip) == pure-Python restatement on fuzzed messages."""
    from go2netspectra_amd.thrift import pack_messages
    from helpers import py_thrift_decode, thrift_messages
    rng = np.random.default_rng(11)
    msgs = thrift_messages(rng, 4000, bad_frac=0.2)
    buf, offs = pack_messages(msgs)
    out = oracle.thrift_decode(buf, offs)
    nok = 0
    for i, m in enumerate(msgs):
        want = py_thrift_decode(m)
        assert bool(out["ok"][i]) == (want is not None), (i, m.hex())
        if want is None:
            continue
        nok += 1
        ts, s, d, sp, dp, pr, ln = want
        assert out["ts"][i] == ts and out["length"][i] == ln
        assert bytes(out["src16"][i]) == (s[:16] + bytes(16))[:16]
        assert bytes(out["dst16"][i]) == (d[:16] + bytes(16))[:16]
        assert (out["sport"][i], out["dport"][i], out["proto"][i]) == (sp, dp, pr)
        assert out["sver"][i] == {4: 4, 16: 6}.get(len(s), 0)
    assert 2500 < nok < 3900


def test_thrift_near_misses_c_vs_python(oracle):
    """CPU twin of test_thrift_gpu.py::test_fast_path_near_misses: on the 70-byte messages
    around the device fast path the two CPU restatements agree; the valid variants decode
    to their own fields and every one-byte header replacement is rejected."""
    from go2netspectra_amd.thrift import pack_messages
    from helpers import py_thrift_decode, thrift_near_misses
    valid, invalid = thrift_near_misses()
    assert len(valid) == 12 and len(invalid) == 34 * 14 - 34  # every checked byte is one of the 14 values
    msgs = [m for _, m, _ in valid] + [m for _, m in invalid]
    out = oracle.thrift_decode(*pack_messages(msgs))
    for i, (name, m, want) in enumerate(valid):
        assert py_thrift_decode(m) == want, name
        ts, s, d, sp, dp, pr, ln = want
        assert out["ok"][i] and out["ts"][i] == ts and out["length"][i] == ln, name
        assert bytes(out["src16"][i]) == s + bytes(16 - len(s)) and bytes(out["dst16"][i]) == d + bytes(16 - len(d)), name
        assert (out["sport"][i], out["dport"][i], out["proto"][i]) == (sp, dp, pr), name
        assert (out["sver"][i], out["dver"][i]) == ({4: 4}.get(len(s), 0), {4: 4}.get(len(d), 0)), name
    for i, (name, m) in enumerate(invalid, len(valid)):
        assert py_thrift_decode(m) is None and not out["ok"][i], name
