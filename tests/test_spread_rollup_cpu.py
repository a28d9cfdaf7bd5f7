"""Host side of the spread roll-up (no GPU): the C ABI declares, exports and binds
gns_spread_rollup outside the pinned gns_exs_ / gns_pairs_ families, the null-handle errors
come before any device call, spread_rollup_plan restates the library's layout check, and
to16_to_encodeflow restates the key-form conversion on hand-written rows."""
import ctypes as ct
import os
import re
import subprocess

import numpy as np
import pytest

from go2netspectra_amd import _lib
from go2netspectra_amd.exact import ip_to16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
NAME = "gns_spread_rollup"


def test_symbol_declared_once_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    decl = re.findall(r"\bint gns_spread_rollup\s*\(([^)]*)\)\s*;", header)
    assert len(decl) == 1
    assert re.sub(r"\s+", " ", decl[0]) == "gns_exs *dst, gns_ex *src, uint64_t since, uint64_t *cursor, uint64_t out[2]"
    assert "GNS_SPREAD_ROLLUP_PIECE" in header  # the test-only piece size is documented where the call is
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in set(re.findall(r"\bT (gns_[a-z0-9_]+)", out))
    assert NAME in _lib.EXPORTED
    fn = getattr(_lib.load(), NAME)
    assert fn.restype is ct.c_int
    assert fn.argtypes == [ct.c_void_p, ct.c_void_p, ct.c_uint64, ct.c_void_p, ct.c_void_p]


def test_the_name_is_outside_the_pinned_families():
    assert not NAME.startswith("gns_exs_") and not NAME.startswith("gns_pairs_")
    header = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    assert NAME not in re.findall(r"\bint (gns_(?:exs|pairs)_[a-z0-9_]+)\s*\(", header)


def test_python_surface():
    from go2netspectra_amd import ExactAggregator, ExactSpread, ExactTask, spread_rollup_plan, to16_to_encodeflow
    assert hasattr(ExactSpread, "rollup_from") and hasattr(ExactAggregator, "spread") and hasattr(ExactTask, "spread")
    assert callable(spread_rollup_plan) and callable(to16_to_encodeflow)
    assert ExactSpread.STAGES[3] == "project" and ExactSpread.STAGES[:3] == ["insert", "resolve", "grow"]
    assert ExactSpread.STAGES[5] == "total"


def test_null_handles_are_errors_before_any_device_call():
    L = _lib.load()
    out = (ct.c_uint64 * 2)(7, 9)
    cur = ct.c_uint64(11)
    h = ct.c_void_p(0x1000)  # never dereferenced: the null check comes first
    assert L.gns_spread_rollup(None, None, 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()
    assert L.gns_spread_rollup(None, h, 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert L.gns_spread_rollup(h, None, 0, ct.byref(cur), out) == _lib.GNS_E_ARG
    assert L.gns_spread_rollup(h, None, 5, None, None) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()
    assert (out[0], out[1], cur.value) == (7, 9, 11)


def test_plan_accepts_subsets_permutations_and_repeats():
    from go2netspectra_amd import rollup_plan, spread_rollup_plan
    # offsets in FIVE: SrcIP 0, DstIP 16, SrcPort 32, DstPort 34, Protocol 36
    assert spread_rollup_plan(FIVE, ["SrcIP"], ["DstIP"]) == (list(range(16)), list(range(16, 32)))
    assert spread_rollup_plan(FIVE, ["DstIP"], ["SrcIP"]) == (list(range(16, 32)), list(range(16)))
    assert spread_rollup_plan(FIVE, ["SrcIP", "DstIP"], ["DstPort"]) == (list(range(32)), [34, 35])
    assert spread_rollup_plan(FIVE, ["SrcPort", "Protocol"], ["DstPort"]) == ([32, 33, 36], [34, 35])
    assert spread_rollup_plan(FIVE, ["SrcIP"], FIVE) == (list(range(16)), list(range(37)))
    # a permuted source; a field used by both layouts; a field repeated inside one
    src = ["Protocol", "DstIP", "SrcIP"]
    assert spread_rollup_plan(src, ["SrcIP"], ["DstIP", "Protocol"]) == (list(range(17, 33)), list(range(1, 17)) + [0])
    assert spread_rollup_plan(FIVE, ["SrcPort"], ["SrcPort", "Protocol", "SrcPort"]) == ([32, 33], [32, 33, 36, 32, 33])
    # a field repeated in src is read at its first occurrence
    assert spread_rollup_plan(["Protocol", "SrcPort", "Protocol"], ["Protocol"], ["SrcPort"]) == ([0], [1, 2])
    for flow, elem in ((FIVE, FIVE[::-1]), (["DstPort"], ["SrcIP", "SrcIP"])):
        pf, pe = spread_rollup_plan(FIVE, flow, elem)
        assert pf == rollup_plan(FIVE, flow) and pe == rollup_plan(FIVE, elem)
        assert all(0 <= g < 37 for g in pf + pe)


def test_plan_names_a_missing_field():
    from go2netspectra_amd import spread_rollup_plan
    with pytest.raises(ValueError, match="DstIP"):
        spread_rollup_plan(["SrcIP"], ["SrcIP"], ["DstIP"])
    with pytest.raises(ValueError, match="SrcPort"):
        spread_rollup_plan(["SrcIP", "DstIP"], ["SrcPort", "SrcIP"], ["DstIP"])
    with pytest.raises(ValueError, match="Protocol"):
        spread_rollup_plan(FIVE[:4], ["SrcIP"], FIVE)
    # a handle made from key sizes alone has no field lists to project onto
    with pytest.raises(ValueError, match="field lists"):
        spread_rollup_plan(FIVE, [], [])
    with pytest.raises(ValueError, match="field lists"):
        spread_rollup_plan(FIVE, ["SrcIP"], None)


V4 = bytes([192, 0, 2, 7])
V6 = bytes.fromhex("20010db8000000000000000000000001")
ALIAS = V4 + bytes(12)           # a genuine 16-byte address whose bytes equal an IPv4 slot
MAPPED = bytes(10) + b"\xff\xff" + V4


def test_form_conversion_on_hand_written_rows():
    from go2netspectra_amd import to16_to_encodeflow
    rows = np.array([
        list(MAPPED + V6 + b"\x01\xbb\xc3\x50\x06"),                       # mapped IPv4 -> the 4-byte form; IPv6 stays
        list(V6 + MAPPED + b"\xff\xff\x00\x00\x11"),                       # the same on the destination side
        list(bytes(10) + b"\xff\xff" + bytes(4) + bytes(16) + bytes(5)),   # ::ffff:0.0.0.0 and :: -> 16 zero bytes both
        list(ALIAS + bytes(10) + b"\xff\xfe" + V4 + b"\x00\x01\x00\x02\x03"),  # neither is mapped: untouched
        list(bytes(9) + b"\x01\xff\xff" + V4 + bytes(9) + b"\xff\xff\xff" + V4 + bytes(5)),  # a nonzero byte in the ten
    ], np.uint8)
    got = to16_to_encodeflow(rows, FIVE)
    assert got.shape == rows.shape and got.dtype == np.uint8
    assert bytes(got[0]) == V4 + bytes(12) + V6 + b"\x01\xbb\xc3\x50\x06"
    assert bytes(got[1]) == V6 + V4 + bytes(12) + b"\xff\xff\x00\x00\x11"
    assert bytes(got[2]) == bytes(37)
    assert bytes(got[3]) == bytes(rows[3]) and bytes(got[4]) == bytes(rows[4])
    assert bytes(rows[0][:16]) == MAPPED  # the input is not modified
    # ports and protocol are copied wherever they lie, and only IP fields are looked at: a port
    # pair ff ff after ten zero bytes of other fields is no mapped prefix
    fields = ["Protocol", "SrcPort", "SrcIP", "DstPort"]
    row = np.array([list(b"\x00" + b"\xff\xff" + MAPPED + b"\xff\xff")], np.uint8)
    assert bytes(to16_to_encodeflow(row, fields)[0]) == b"\x00\xff\xff" + V4 + bytes(12) + b"\xff\xff"
    row = np.array([list(b"\x00\x00\x00\x00\xff")], np.uint8)
    assert bytes(to16_to_encodeflow(row, ["SrcPort", "DstPort", "Protocol"])[0]) == bytes(row[0])
    assert to16_to_encodeflow(np.zeros((0, 16), np.uint8), ["SrcIP"]).shape == (0, 16)


def test_conversion_inverts_ip_to16_on_the_4_byte_form():
    from go2netspectra_amd import to16_to_encodeflow
    rng = np.random.default_rng(3)
    v4 = rng.integers(0, 256, (64, 4), dtype=np.uint8)
    v4[0] = 0            # 0.0.0.0
    v4[1] = 255
    to16 = np.array([list(ip_to16(bytes(a))) for a in v4], np.uint8)
    back = to16_to_encodeflow(to16, ["DstIP"])
    assert np.array_equal(back[:, :4], v4) and (back[:, 4:] == 0).all()
    # textual spellings go through the same form
    for text, want in (("1.2.3.4", bytes([1, 2, 3, 4])), ("::ffff:10.0.0.9", bytes([10, 0, 0, 9]))):
        row = np.frombuffer(ip_to16(text), np.uint8)[None, :]
        assert bytes(to16_to_encodeflow(row, ["SrcIP"])[0]) == want + bytes(12)
    # a 16-byte address is its own To16 form and comes back unchanged
    row = np.frombuffer(ip_to16(V6), np.uint8)[None, :]
    assert bytes(to16_to_encodeflow(row, ["SrcIP"])[0]) == V6
