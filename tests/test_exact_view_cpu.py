"""Host side of the exact engine's snapshot views (no GPU): the C ABI exports and binds the
six gns_ex_view_* entry points and the Go binding's type, the null-argument errors come
before any device call, and apply_delta is the consumer's fold of a delta export."""
import ctypes as ct
import os
import re
import subprocess

import numpy as np

from go2netspectra_amd import ExactView, _lib, apply_delta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW = ["gns_ex_view_create", "gns_ex_view_destroy", "gns_ex_view_refresh", "gns_ex_view_snapshot",
        "gns_ex_view_aggregate", "gns_ex_view_heavy_hitters"]


def test_library_exports_and_binds_the_view_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gns_[a-z0-9_]+)", out))
    assert set(VIEW) <= exported
    assert set(VIEW) <= set(_lib.EXPORTED)
    txt = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    assert "typedef struct gns_ex_view gns_ex_view;" in txt
    for name in VIEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    L = _lib.load()
    for name in VIEW:
        fn = getattr(L, name)
        assert fn.restype is ct.c_int and fn.argtypes, name
    assert L.gns_ex_view_refresh.argtypes == [ct.c_void_p, ct.c_uint64, ct.c_void_p]
    # the view calls take what the handle's calls take
    for a, b in (("gns_ex_view_snapshot", "gns_ex_snapshot"), ("gns_ex_view_aggregate", "gns_ex_aggregate"),
                 ("gns_ex_view_heavy_hitters", "gns_ex_heavy_hitters")):
        assert getattr(L, a).argtypes == getattr(L, b).argtypes
    assert all(hasattr(ExactView, m) for m in ("refresh", "snapshot_arrays", "aggregate", "heavy_hitters", "close"))


def test_go_binding_has_the_view_type():
    src = open(os.path.join(ROOT, "integration", "go", "sketchgpu", "sketchgpu.go")).read()
    assert re.search(r"^type ExactView struct \{", src, re.M)
    for name in VIEW:  # (test_go_binding.py checks each call's arity against the header)
        assert "C.%s(" % name in src, name
    for method in ("NewView", "Refresh", "Flows", "Aggregate", "HeavyHitters", "Close"):
        recv = r"\(e \*Exact\)" if method == "NewView" else r"\(w \*ExactView\)"
        assert re.search(r"^func %s %s\(" % (recv, method), src, re.M), method


def test_null_arguments_are_errors_before_any_device_call():
    L = _lib.load()
    h = ct.c_void_p()
    assert L.gns_ex_view_create(None, ct.byref(h)) == _lib.GNS_E_ARG and not h.value
    assert L.gns_ex_view_create(ct.c_void_p(0x1000), None) == _lib.GNS_E_ARG  # a null out: the handle is not touched
    cur, n = ct.c_uint64(7), ct.c_uint64(5)
    assert L.gns_ex_view_refresh(None, 0, ct.byref(cur)) == _lib.GNS_E_ARG and cur.value == 7
    assert L.gns_ex_view_snapshot(None, None, None, None, None, None, ct.byref(n)) == _lib.GNS_E_ARG and n.value == 5
    f, out = (_lib.ExFilter * 1)(), (_lib.ExSummary * 1)()
    assert L.gns_ex_view_aggregate(None, f, 1, out) == _lib.GNS_E_ARG
    assert L.gns_ex_view_heavy_hitters(None, 0, 0, 0, None, None, ct.byref(n)) == _lib.GNS_E_ARG
    assert L.gns_ex_view_destroy(None) == 0
    assert b"null" in L.gns_last_error()


def rows(*r):
    """snapshot_arrays() of hand-made rows (key bytes, start, end, packets, bytes)."""
    if not r:
        return (np.zeros((0, 3), np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint64),
                np.zeros(0, np.uint64))
    return (np.array([list(x[0]) for x in r], np.uint8), np.array([x[1] for x in r], np.int64),
            np.array([x[2] for x in r], np.int64), np.array([x[3] for x in r], np.uint64),
            np.array([x[4] for x in r], np.uint64))


def test_apply_delta_is_the_consumers_rule():
    a, b, c = b"\x01\x02\x03", b"\x01\x02\x04", b"\xff\x00\x00"
    full = rows((a, -5, 10, 3, 300), (b, 7, 7, 1, (1 << 40) + 1))
    state = apply_delta({}, full)
    assert state == {a: (-5, 10, 3, 300), b: (7, 7, 1, (1 << 40) + 1)}
    assert all(type(x) is int for v in state.values() for x in v)
    # a later row overrides (rows are cumulative, not increments), a new key appears, the rest stays
    delta = rows((a, -5, 99, 8, 900), (c, 50, 60, (1 << 63) + 2, 1))
    nxt = apply_delta(state, delta)
    assert nxt == {a: (-5, 99, 8, 900), b: (7, 7, 1, (1 << 40) + 1), c: (50, 60, (1 << 63) + 2, 1)}
    assert state == {a: (-5, 10, 3, 300), b: (7, 7, 1, (1 << 40) + 1)}  # pure: the input map is untouched
    # within one delta the later row wins too
    assert apply_delta({}, rows((a, 1, 1, 1, 1), (a, 1, 2, 2, 2)))[a] == (1, 2, 2, 2)
    # an empty delta is the identity
    assert apply_delta(nxt, rows()) == nxt and apply_delta({}, rows()) == {}
    # folding the deltas in order equals the last full export
    assert apply_delta(apply_delta({}, full), delta) == apply_delta({}, rows((a, -5, 99, 8, 900), (b, 7, 7, 1, (1 << 40) + 1),
                                                                           (c, 50, 60, (1 << 63) + 2, 1)))
