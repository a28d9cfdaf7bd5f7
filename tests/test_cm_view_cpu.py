"""CPU: the detached Count-Min view's calls exist at every layer (library, header,
ctypes binding), reject a null view before any device call, and the checkpoint of a view
is a CountMin file."""
import os
import re
import subprocess

import numpy as np

from go2netspectra_amd import _lib, checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gns_cm_view_refresh_at", "gns_cm_view_query_device", "gns_cm_view_heavy_rows", "gns_cm_view_export_state"]


def test_symbols_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gns_[a-z0-9_]+)", out))
    txt = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    declared = set(re.findall(r"\bint (gns_[a-z0-9_]+)\s*\(", txt))
    L = _lib.load()
    for name in NEW:
        assert name in exported, name
        assert name in declared, name
        assert name in _lib.EXPORTED, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is not None, name
    assert re.search(r"#define\s+GNS_CM_VIEW_DETACH\s+1u", txt)
    assert _lib.GNS_CM_VIEW_DETACH == 1


def test_null_view_is_an_argument_error():
    L = _lib.load()
    n = np.zeros(2, np.uint64)
    out = np.zeros(4, np.uint64)
    keys = np.zeros((4, 16), np.uint8)
    assert L.gns_cm_view_refresh_at(None, _lib.GNS_CM_VIEW_DETACH) == _lib.GNS_E_ARG
    assert L.gns_cm_view_refresh_at(None, 0) == _lib.GNS_E_ARG
    assert L.gns_cm_view_query_device(None, keys.ctypes.data, 16, 4, out.ctypes.data) == _lib.GNS_E_ARG
    assert L.gns_cm_view_heavy_rows(None, None, n.ctypes.data, None, n[1:].ctypes.data) == _lib.GNS_E_ARG
    assert L.gns_cm_view_export_state(None, None, None, None, None, None) == _lib.GNS_E_ARG
    assert b"null" in L.gns_last_error()


class CountMin:  # what checkpoint.describe reads of the live class (its name included)
    width, depth, key_bytes = 8, 2, 5
    flow_fields = ["SrcIP"]
    size_threshold, count_threshold = 1000, 10
    _seeds = np.array([7, 9], np.uint32)
    bucket_range = None


class CountMinView:  # stand-in for sketch.CountMinView: checkpoint.save goes by the class name
    def __init__(self):
        self.parent = CountMin()
        n, K = 16, 5
        rng = np.random.default_rng(3)
        self.state = (rng.integers(0, 99, n).astype(np.uint32), rng.integers(0, 99, n).astype(np.uint32),
                      rng.integers(0, 256, (n, 8), dtype=np.uint8)[:, :K], rng.integers(0, 256, (n, 8), dtype=np.uint8)[:, :K])

    def export_state(self):
        return self.state

    def counters(self):
        return {"inserted": 123, "dropped": 4, "unsupported": 5}


def test_checkpoint_of_a_view_is_a_countmin_file(tmp_path):
    view = CountMinView()
    checkpoint.save(view, tmp_path / "v.npz")
    meta, arrays = checkpoint.read(tmp_path / "v.npz")
    assert meta["class"] == "CountMin" and meta["counters"] == [123, 4, 5]
    checkpoint.check_meta(meta, checkpoint.describe(view.parent))
    assert sorted(arrays) == sorted(checkpoint.ARRAYS["CountMin"])
    for name, want in zip(("C", "S", "FPc", "FPs"), view.state):
        assert arrays[name].dtype == want.dtype and np.array_equal(arrays[name], want)
    assert arrays["FPc"].flags["C_CONTIGUOUS"]
