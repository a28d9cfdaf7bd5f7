"""Exact spread pair set interface (gns_pairs_export / _merge / _merge_from), the
parts that need no GPU: the three C symbols are declared, exported and bound
outside the gns_exs_ family, argument errors come before any device call, and
the checkpoint file format knows the class ExactSpread."""
import ctypes as ct
import os
import re
import subprocess

import numpy as np
import pytest

import go2netspectra_amd as g
from go2netspectra_amd import _lib, checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ["gns_pairs_export", "gns_pairs_merge", "gns_pairs_merge_from"]


def test_symbols_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "gns_sketch.h")) as f:
        header = f.read()
    assert set(re.findall(r"\bint (gns_pairs_[a-z0-9_]+)\s*\(", header)) == set(PAIRS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (gns_pairs_[a-z0-9_]+)", out)) == set(PAIRS)
    assert set(PAIRS) <= set(_lib.EXPORTED)
    assert not [s for s in PAIRS if s.startswith("gns_exs_")]
    L = g.load()
    for name in PAIRS:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is ct.c_int, name


def test_null_arguments_are_argument_errors():
    L = g.load()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    n = ct.c_uint64(4)
    assert L.gns_pairs_export(None, 0, p, p, ct.byref(n), None, _lib.MEM_HOST) == _lib.GNS_E_ARG
    assert n.value == 4
    assert L.gns_pairs_merge(None, p, 16, p, 16, 1, _lib.MEM_HOST) == _lib.GNS_E_ARG
    assert L.gns_pairs_merge_from(None, None, 0, None) == _lib.GNS_E_ARG
    # a null n is refused before the handle is looked at (p is no handle and is never read as one);
    # so is a null source or destination of merge_from
    assert L.gns_pairs_export(p, 0, None, None, None, None, _lib.MEM_HOST) == _lib.GNS_E_ARG
    assert L.gns_pairs_merge_from(p, None, 0, None) == _lib.GNS_E_ARG
    assert L.gns_pairs_merge_from(None, p, 0, None) == _lib.GNS_E_ARG
    assert (buf == 0).all()


META = {"format": 1, "class": "ExactSpread", "flow_fields": ["SrcIP"], "elem_fields": ["DstIP", "DstPort"],
        "flow_bytes": 16, "elem_bytes": 18}


def test_checkpoint_knows_the_class():
    assert checkpoint.PARAMS["ExactSpread"] == ["flow_fields", "elem_fields", "flow_bytes", "elem_bytes"]
    assert checkpoint.ARRAYS["ExactSpread"] == ["flows", "elems"]
    assert checkpoint.FORMAT == 1


def _changed(v):
    if isinstance(v, list):
        return v[:-1] if v else ["SrcIP"]
    return v + 1


@pytest.mark.parametrize("name", ["class"] + ["flow_fields", "elem_fields", "flow_bytes", "elem_bytes"])
def test_each_metadata_field_is_compared_and_named(name):
    live = META
    checkpoint.check_meta(dict(live), live)
    checkpoint.check_meta(dict(live, counters=[1, 2, 3]), live)  # state, not parameters: never compared
    assert name == "class" or name in checkpoint.PARAMS["ExactSpread"]
    saved = dict(live)
    saved[name] = "ExactAggregator" if name == "class" else _changed(live[name])
    with pytest.raises(ValueError, match=f"'{name}'"):
        checkpoint.check_meta(saved, live)
    if name != "class":
        del saved[name]
        with pytest.raises(ValueError, match=f"'{name}'"):
            checkpoint.check_meta(saved, live)


@pytest.mark.parametrize("rows", [0, 1, 1000])
def test_file_round_trip_of_pair_rows(tmp_path, rows):
    rng = np.random.default_rng(rows)
    arrays = {"flows": rng.integers(0, 256, (rows, 16), dtype=np.uint8),
              "elems": rng.integers(0, 256, (rows, 18), dtype=np.uint8)}
    path = tmp_path / "pairs.npz"
    checkpoint.write(path, META, arrays)
    meta, got = checkpoint.read(path)
    assert meta == META
    assert sorted(got) == sorted(checkpoint.ARRAYS["ExactSpread"])
    for k, a in arrays.items():
        assert got[k].dtype == np.uint8 and got[k].shape == a.shape and np.array_equal(got[k], a), k
