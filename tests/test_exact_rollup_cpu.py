"""Host side of the exact aggregator's roll-up (no GPU): the C ABI declares, exports and binds
gns_ex_rollup, the Go binding calls it, the null-handle errors come before any device call,
and rollup_plan restates the library's layout check (absent field, repeated field,
permutation)."""
import ctypes as ct
import os
import re
import subprocess

import pytest

from go2netspectra_amd import ExactAggregator, ExactTask, _lib, rollup_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]


def test_library_declares_exports_and_binds_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "gns_ex_rollup" in set(re.findall(r"\bT (gns_[a-z0-9_]+)", out))
    assert "gns_ex_rollup" in _lib.EXPORTED
    txt = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    assert re.search(r"\bint gns_ex_rollup\s*\(\s*gns_ex \*dst,\s*gns_ex \*src,\s*uint64_t out\[2\]\)", txt)
    assert "GNS_EX_ROLLUP_PIECE" in txt  # the test-only piece size is documented where the call is
    fn = _lib.load().gns_ex_rollup
    assert fn.restype is ct.c_int and fn.argtypes == [ct.c_void_p, ct.c_void_p, ct.c_void_p]
    assert all(hasattr(ExactAggregator, m) for m in ("rollup_from", "rollup")) and hasattr(ExactTask, "rollup")


def test_null_handles_are_errors_before_any_device_call():
    L = _lib.load()
    out = (ct.c_uint64 * 2)(7, 9)
    h = ct.c_void_p(0x1000)  # never dereferenced: the null check comes first
    assert L.gns_ex_rollup(None, None, out) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()
    assert L.gns_ex_rollup(None, h, out) == _lib.GNS_E_ARG
    assert L.gns_ex_rollup(h, None, out) == _lib.GNS_E_ARG
    assert L.gns_ex_rollup(None, h, None) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()
    assert (out[0], out[1]) == (7, 9)


def test_go_binding_has_the_method():
    src = open(os.path.join(ROOT, "integration", "go", "sketchgpu", "sketchgpu.go")).read()
    assert re.search(r"^func \(e \*Exact\) RollupFrom\(src \*Exact\) \(projected, added uint64, err error\) \{", src, re.M)
    assert "C.gns_ex_rollup(" in src  # (test_go_binding.py checks the call's arity against the header)


def test_rollup_plan_is_the_byte_gather_between_two_layouts():
    # offsets in FIVE: SrcIP 0, DstIP 16, SrcPort 32, DstPort 34, Protocol 36
    assert rollup_plan(FIVE, FIVE) == list(range(37))
    assert rollup_plan(FIVE, ["SrcIP"]) == list(range(16))
    assert rollup_plan(FIVE, ["DstPort", "Protocol"]) == [34, 35, 36]
    assert rollup_plan(FIVE, ["Protocol"]) == [36]
    # a permutation
    assert rollup_plan(FIVE, ["DstIP", "SrcIP", "SrcPort"]) == list(range(16, 32)) + list(range(16)) + [32, 33]
    assert rollup_plan(["Protocol", "SrcPort"], ["SrcPort", "Protocol"]) == [1, 2, 0]
    # a field repeated in dst is copied once per occurrence
    assert rollup_plan(FIVE, ["SrcPort", "Protocol", "SrcPort"]) == [32, 33, 36, 32, 33]
    # ... and one repeated in src is read at its first occurrence
    assert rollup_plan(["Protocol", "SrcPort", "Protocol"], ["Protocol", "Protocol"]) == [0, 0]
    # an absent field
    with pytest.raises(ValueError, match="DstIP"):
        rollup_plan(["SrcIP"], ["DstIP"])
    with pytest.raises(ValueError, match="Protocol"):
        rollup_plan(["SrcIP", "DstIP", "SrcPort", "DstPort"], FIVE)
    # every plan entry is an offset inside the source key
    for dst in (FIVE, FIVE[::-1], ["DstPort"], ["SrcIP", "SrcIP"]):
        plan = rollup_plan(FIVE, dst)
        assert len(plan) == sum(_lib.FIELD_SIZE[f] for f in dst) and all(0 <= g < 37 for g in plan)
