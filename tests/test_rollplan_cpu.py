"""gns_rollplan.hpp on the host: the gather and the mask tables every roll-up is planned with,
byte for byte against the Python restatements in exact.py (rollup_plan, prefix_plan for the
To16 and the EncodeFlow form, spread_rollup_plan).  A stand-alone program around the header,
built with ASan + UBSan; the cases go in on stdin, one per line, and the tables come back."""
import os
import shutil
import subprocess

import pytest

from go2netspectra_amd import _lib, make_prefix, prefix_plan, rollup_plan, spread_rollup_plan

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "gns_rollplan.hpp"

// a case: K src[K] R, then per row: n dst[n] has_px src_v4 src_v6 dst_v4 dst_v6 encodeflow.
// The R rows share one ipoff, as a spread roll-up's flow and element rows do.
int main() {
    unsigned K;
    while (std::scanf("%u", &K) == 1) {
        std::vector<uint8_t> src(K);  // exactly K bytes: a gather that runs past the layout is reported
        unsigned v, R;
        for (auto &b : src) { if (std::scanf("%u", &v) != 1) return 2; b = (uint8_t)v; }
        if (std::scanf("%u", &R) != 1) return 2;
        uint8_t ipoff[2] = {0xFF, 0xFF};
        for (unsigned r = 0; r < R; r++) {
            unsigned n, p[6];
            if (std::scanf("%u", &n) != 1) return 2;
            std::vector<uint8_t> dst(n);
            for (auto &b : dst) { if (std::scanf("%u", &v) != 1) return 2; b = (uint8_t)v; }
            for (auto &x : p) if (std::scanf("%u", &x) != 1) return 2;
            gns_prefix px;
            px.src_v4 = (uint8_t)p[1]; px.src_v6 = (uint8_t)p[2]; px.dst_v4 = (uint8_t)p[3]; px.dst_v6 = (uint8_t)p[4];
            gns::RollRow row;
            std::vector<uint8_t> g(n);
            const int miss = gns::roll_tables(src.data(), K, dst.data(), n, p[0] ? &px : nullptr, p[5] != 0, &row, ipoff);
            const int miss2 = gns::roll_gather(src.data(), K, dst.data(), n, g.data());
            if (miss != miss2) return 3;
            if (miss >= 0) { std::printf("miss %d %s\n", miss, gns::tuple_field_name(dst[miss])); continue; }
            if (n && memcmp(g.data(), row.g, n)) return 3;
            const uint8_t *tab[4] = {row.g, row.fld, row.m4, row.m6};
            for (auto t : tab) {
                for (unsigned j = 0; j < n; j++) std::printf("%u ", t[j]);
                std::printf("\n");
            }
        }
        std::printf("ipoff %u %u\n", ipoff[0], ipoff[1]);
    }
    return 0;
}
"""

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
BASE = {"SrcIP": 0, "DstIP": 16, "SrcPort": 32, "DstPort": 34, "Protocol": 36}  # make_plan's numbering
V4 = [0, 1, 7, 8, 9, 24, 31, 32]
V6 = [0, 1, 63, 64, 65, 127, 128]

# (source layout, destination layout)
LAYOUTS = [
    (FIVE, FIVE),                                                   # the five-tuple to itself
    (FIVE, ["DstPort"]),                                            # a single field
    (FIVE, ["SrcIP"]),
    (FIVE, ["Protocol", "DstPort", "DstIP", "SrcPort", "SrcIP"]),   # a permutation
    (["SrcIP", "DstPort", "SrcIP", "DstIP"], ["DstIP", "SrcIP"]),   # repeated in the source: the first occurrence
    (FIVE, ["SrcIP", "SrcPort", "SrcIP"]),                          # repeated in the destination
    (["Protocol", "SrcIP"], ["SrcIP", "Protocol"]),                 # an IP field at an unaligned offset
    (["SrcPort", "Protocol", "DstIP", "SrcIP"], ["SrcIP", "DstIP"]),
]
ABSENT = [
    (["SrcIP", "DstPort"], ["SrcIP", "DstIP"]),
    (["SrcIP", "DstIP"], ["Protocol"]),
    (["DstIP", "SrcPort", "DstPort"], ["DstPort", "SrcPort", "SrcIP", "DstIP"]),
]
# (source, flow, element)
SPREADS = [
    (FIVE, ["SrcIP"], ["DstIP"]),
    (FIVE, ["SrcIP"], ["SrcIP"]),                                   # one field as both flow and element
    (["Protocol", "SrcIP"], ["SrcIP"], ["Protocol"]),
    (["Protocol", "DstIP", "SrcIP"], ["DstIP", "Protocol"], ["SrcIP", "DstIP"]),
    (FIVE, ["SrcIP", "DstPort"], ["SrcPort", "Protocol"]),
]
SPREADS_ABSENT = [
    (["SrcIP", "DstPort"], ["DstIP"], ["SrcIP"], "flow"),
    (["SrcIP", "DstPort"], ["SrcIP"], ["SrcPort"], "element"),
]


def tuple_bytes(fields):
    return [BASE[f] + b for f in fields for b in range(_lib.FIELD_SIZE[f])]


def prefixes():
    """Every listed length at least once per field and address class, and None (no mask)."""
    out = [None]
    n = max(len(V4), len(V6))
    for i in range(n):
        out.append({"SrcIP": (V4[i % len(V4)], V6[i % len(V6)]), "DstIP": (V4[-1 - i % len(V4)], V6[-1 - i % len(V6)])})
    out.append({"SrcIP": 24})
    out.append({"DstIP": (32, 64)})
    return out


def px_words(prefix):
    if prefix is None:  # a null gns_prefix
        return [0, 0, 0, 0, 0]
    px = make_prefix(prefix)
    return [1, px.src_v4, px.src_v6, px.dst_v4, px.dst_v6]


def row_words(dst, prefix, encodeflow):
    t = tuple_bytes(dst)
    return [len(t)] + t + px_words(prefix) + [int(encodeflow)]


def case_line(src, rows):
    t = tuple_bytes(src)
    w = [len(t)] + t + [len(rows)]
    for r in rows:
        w += row_words(*r)
    return " ".join(map(str, w))


def want_ipoff(src, dsts):
    return [rollup_plan(src, [f])[0] if any(f in d for d in dsts) else 0xFF for f in ("SrcIP", "DstIP")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "go2netspectra_amd", "csrc")
    tmp = tmp_path_factory.mktemp("rollplan")
    src, exe = tmp / "rollplan_driver.cpp", str(tmp / "rollplan_driver")
    src.write_text(DRIVER)
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, str(src), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-3000:]
        return [[int(x) if x.isdigit() else x for x in ln.split()] for ln in r.stdout.splitlines()]
    return run


def test_header_includes_no_hip():
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(here, "..", "go2netspectra_amd", "csrc", "gns_rollplan.hpp")).read()
    assert "#include <hip" not in txt and "__device__" not in txt and "__global__" not in txt


def test_gather_and_mask_tables_match_the_python_plans(driver):
    cases = [(s, d, px, enc) for s, d in LAYOUTS for px in prefixes() for enc in (False, True)]
    out = driver([case_line(s, [(d, px, enc)]) for s, d, px, enc in cases])
    assert len(out) == 5 * len(cases)
    for i, (s, d, px, enc) in enumerate(cases):
        g, fld, m4, m6, ipoff = out[5 * i:5 * i + 5]
        what = (s, d, px, enc)
        assert g == rollup_plan(s, d), what
        assert (g, fld, m4, m6) == tuple(map(list, prefix_plan(s, d, px, encodeflow=enc))), what
        assert ipoff == ["ipoff"] + want_ipoff(s, [d]), what
        if px is None:  # a null prefix keeps every bit
            assert m4 == [0xFF] * len(g) and m6 == [0xFF] * len(g), what


def test_an_absent_field_is_named_as_python_names_it(driver):
    out = driver([case_line(s, [(d, None, False)]) for s, d in ABSENT])
    assert len(out) == 2 * len(ABSENT)
    for i, (s, d) in enumerate(ABSENT):
        tag, j, name = out[2 * i]
        assert tag == "miss"
        missing = next(f for f in d if f not in s)
        assert name == missing and tuple_bytes(d)[j] == BASE[missing]  # the field's first byte
        with pytest.raises(ValueError, match=f"rollup: key field {name} is not part of the source's layout"):
            rollup_plan(s, d)


def test_spread_rows_match_spread_rollup_plan(driver):
    pxs = prefixes()
    cases = [(s, f, e, pxs[k % len(pxs)], pxs[(k + 3) % len(pxs)]) for k, (s, f, e) in enumerate(SPREADS * len(pxs))]
    out = driver([case_line(s, [(f, fpx, True), (e, epx, True)]) for s, f, e, fpx, epx in cases])
    assert len(out) == 9 * len(cases)
    for i, (s, f, e, fpx, epx) in enumerate(cases):
        rows, ipoff = out[9 * i:9 * i + 8], out[9 * i + 8]
        what = (s, f, e, fpx, epx)
        assert (rows[0], rows[4]) == tuple(map(list, spread_rollup_plan(s, f, e))), what
        assert tuple(rows[0:4]) == tuple(map(list, prefix_plan(s, f, fpx, encodeflow=True))), what
        assert tuple(rows[4:8]) == tuple(map(list, prefix_plan(s, e, epx, encodeflow=True))), what
        assert ipoff == ["ipoff"] + want_ipoff(s, [f, e]), what  # each IP field the rows read, once, in any order


def test_spread_absent_field_names_row_and_field(driver):
    out = driver([case_line(s, [(f, None, True), (e, None, True)]) for s, f, e, _ in SPREADS_ABSENT])
    assert len(out) == 6 * len(SPREADS_ABSENT)  # per case: one row's four tables, the other's miss, ipoff
    for i, (s, f, e, which) in enumerate(SPREADS_ABSENT):
        tag, _, name = out[6 * i + (0 if which == "flow" else 4)]
        assert tag == "miss"
        assert name == next(x for x in (f if which == "flow" else e) if x not in s)
        with pytest.raises(ValueError, match=rf"key field {name} is not part of the source's layout \({which} layout\)"):
            spread_rollup_plan(s, f, e)
