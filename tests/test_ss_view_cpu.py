"""Host side of SuperSpread's snapshot views (no GPU): the C ABI exports, declares and binds
the eight gns_ss_view_* entry points, the null-argument errors come before any device
call and leave the outputs untouched, the Python layers have the view methods, and the Go
binding has the type with every call."""
import ctypes as ct
import os
import re
import subprocess

from go2netspectra_amd import Manager, SketchTask, SuperSpread, SuperSpreadView, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW = ["gns_ss_view_create", "gns_ss_view_destroy", "gns_ss_view_refresh", "gns_ss_view_query",
        "gns_ss_view_query_device", "gns_ss_view_heavy_hitters", "gns_ss_view_heavy_rows",
        "gns_ss_view_export_state"]


def test_library_exports_declares_and_binds_the_view_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gns_[a-z0-9_]+)", out))
    assert set(VIEW) <= exported
    assert set(VIEW) <= set(_lib.EXPORTED)
    txt = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    assert "typedef struct gns_ss_view gns_ss_view;" in txt
    assert re.search(r"^#define GNS_SS_VIEW_STATE 1u\b", txt, re.M)
    for name in VIEW:
        assert re.search(r"^int %s\s*\(" % name, txt, re.M), name
    L = _lib.load()
    for name in VIEW:
        fn = getattr(L, name)
        assert fn.restype is ct.c_int and fn.argtypes, name
    assert L.gns_ss_view_refresh.argtypes == [ct.c_void_p, ct.c_uint32]
    assert _lib.GNS_SS_VIEW_STATE == 1
    # the view's query and list calls take what the handle's calls take
    for a, b in (("gns_ss_view_query", "gns_ss_query"), ("gns_ss_view_query_device", "gns_ss_query_device"),
                 ("gns_ss_view_heavy_hitters", "gns_ss_heavy_hitters")):
        assert getattr(L, a).argtypes == getattr(L, b).argtypes, a
    assert len(L.gns_ss_view_export_state.argtypes) == len(L.gns_ss_export_state.argtypes) + 2


def test_null_arguments_are_errors_before_any_device_call():
    L = _lib.load()
    E = _lib.GNS_E_ARG
    h = ct.c_void_p(0x55)
    assert L.gns_ss_view_create(None, ct.byref(h)) == E and h.value == 0x55  # (no handle: out is not written)
    assert L.gns_ss_view_create(ct.c_void_p(0x1000), None) == E  # a null out: the handle is not touched
    assert L.gns_ss_view_refresh(None, 0) == E
    assert L.gns_ss_view_refresh(None, _lib.GNS_SS_VIEW_STATE) == E
    n = ct.c_uint64(5)
    out = (ct.c_uint64 * 2)(7, 7)
    key = (ct.c_uint8 * 16)()
    assert L.gns_ss_view_query(None, key, 16, 1, out) == E and list(out) == [7, 7]
    assert L.gns_ss_view_query_device(None, key, 16, 1, out) == E and list(out) == [7, 7]
    flows, vals = (ct.c_uint8 * 16)(*([9] * 16)), (ct.c_uint32 * 1)(9)
    assert L.gns_ss_view_heavy_hitters(None, flows, vals, ct.byref(n)) == E and n.value == 5
    assert list(flows) == [9] * 16 and vals[0] == 9
    assert L.gns_ss_view_heavy_rows(None, None, ct.byref(n)) == E and n.value == 5
    rec, cnt = ct.c_uint64(3), (ct.c_uint64 * 3)(1, 2, 3)
    assert L.gns_ss_view_export_state(None, None, None, None, None, ct.byref(rec), cnt) == E
    assert rec.value == 3 and list(cnt) == [1, 2, 3]
    assert b"null" in L.gns_last_error()
    assert L.gns_ss_view_destroy(None) == 0


def test_python_layers_have_the_view_methods():
    for m in ("refresh", "query_many", "query", "heavy_hitters_arrays", "heavy_hitters", "heavy_hitters_rows_device",
              "export_state", "counters", "close"):
        assert callable(getattr(SuperSpreadView, m)), m
    assert callable(SuperSpread.view)
    assert SuperSpread.STAGES[6] == "view" and SuperSpread.STAGES[:6] == ["extract", "resolve", "encode", "apply",
                                                                           "unused", "total"]
    for m in ("view", "snapshot_from", "save_from"):
        assert callable(getattr(SketchTask, m)), m
    for m in ("views", "refresh_views", "snapshot_from_views"):
        assert callable(getattr(Manager, m)), m


def test_go_binding_has_the_view_type():
    src = open(os.path.join(ROOT, "integration", "go", "sketchgpu", "sketchgpu.go")).read()
    assert re.search(r"^type SuperSpreadView struct \{", src, re.M)
    for name in VIEW:  # (test_go_binding.py checks each call's arity against the header)
        assert "C.%s(" % name in src, name
    for method in ("NewView", "Refresh", "Query", "HeavyHitters", "Close"):
        recv = r"\(s \*SuperSpread\)" if method == "NewView" else r"\(w \*SuperSpreadView\)"
        assert re.search(r"^func %s %s\(" % (recv, method), src, re.M), method
    assert re.search(r"^func \(w \*SuperSpreadView\) Refresh\(state bool\)", src, re.M)
