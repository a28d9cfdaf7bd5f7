"""Exact spread engine, host side: the gns_exs_* ABI is declared, exported and
bound; argument errors need no device; the accuracy protocol's arithmetic
(cm_test.go:191-229) against hand-worked cases."""
import os
import re
import subprocess

import pytest

import go2netspectra_amd as g
from go2netspectra_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXS = ["gns_exs_create", "gns_exs_destroy", "gns_exs_insert_keys", "gns_exs_insert_tuples", "gns_exs_insert_headers",
       "gns_exs_flush", "gns_exs_query", "gns_exs_query_device", "gns_exs_heavy_hitters", "gns_exs_snapshot",
       "gns_exs_reset", "gns_exs_counters", "gns_exs_dict_stats", "gns_exs_set_timing", "gns_exs_stage_times"]

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]


def test_abi_declared_exported_bound():
    txt = open(os.path.join(ROOT, "include", "gns_sketch.h")).read()
    declared = set(re.findall(r"\bint (gns_exs_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(EXS)
    assert "typedef struct gns_exs_params" in txt
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gns_exs_[a-z0-9_]+)", out))
    assert exported == set(EXS)
    assert set(EXS) <= set(_lib.EXPORTED)
    L = g.load()
    for name in EXS:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is not None, name


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(g.GnsError) as e:
        g.ExactSpread(["SrcIP"], ["DstIP"])
    assert e.value.code == _lib.GNS_E_NODEV


@pytest.mark.parametrize("flow,elem,kw", [
    ([], ["DstIP"], {}),                              # flow_bytes == 0
    (["SrcIP"], [], {}),                              # elem_bytes == 0
    (["SrcIP"], ["NoSuchField"], {}),                 # unknown names contribute 0 bytes
    (FIVE + ["SrcPort"], ["DstIP"], {}),              # 39 bytes
    (["SrcIP"], FIVE + ["Protocol"], {}),             # 38 bytes
    (None, None, {"flow_bytes": 38, "elem_bytes": 4}),
    (None, None, {"flow_bytes": 4, "elem_bytes": 0}),
    (["SrcIP"] * 9, ["DstIP"], {}),                   # more than 8 fields
])
def test_bad_layouts_rejected_without_a_device(flow, elem, kw):
    """Sizes of 0 or above 37 and layouts deeper than 8 are argument errors, reported
    before any device call: the same answer with and without a GPU."""
    with pytest.raises((g.GnsError, ValueError)) as e:
        g.ExactSpread(flow, elem, **kw)
    if isinstance(e.value, g.GnsError):
        assert e.value.code == _lib.GNS_E_ARG


def test_evaluate_heavy_hitters_hand_worked():
    from go2netspectra_amd.accuracy import evaluate_heavy_hitters as ev
    # disjoint: nothing matches
    assert ev({b"a": 10, b"b": 20}, {b"c": 5}) == (0.0, 0.0, 0.0, 0.0, 0, 2, 1)
    # identical sets and values
    assert ev({b"a": 10, b"b": 20}, {b"a": 10, b"b": 20}) == (0.0, 1.0, 1.0, 1.0, 2, 0, 0)
    # partial overlap: a over by 50 %, b under by 25 %; c is a false positive, d is missed
    mre, p, r, f1, tp, fp, fn = ev({b"a": 15, b"b": 30, b"c": 7}, {b"a": 10, b"b": 40, b"d": 9})
    assert (tp, fp, fn) == (2, 1, 1)
    assert mre == pytest.approx((0.5 + 0.25) / 2, abs=1e-15)
    assert p == pytest.approx(2 / 3, abs=1e-15) and r == pytest.approx(2 / 3, abs=1e-15)
    assert f1 == pytest.approx(2 / 3, abs=1e-15)
    # empty detected: recall has a denominator, precision and F1 do not
    assert ev({}, {b"a": 1, b"b": 2}) == (0.0, 0.0, 0.0, 0.0, 0, 0, 2)
    # empty truth
    assert ev({b"a": 1}, {}) == (0.0, 0.0, 0.0, 0.0, 0, 1, 0)
    # both empty: every ratio is 0
    assert ev({}, {}) == (0.0, 0.0, 0.0, 0.0, 0, 0, 0)
    # precision 1, recall 1/2
    mre, p, r, f1, tp, fp, fn = ev({b"a": 8}, {b"a": 10, b"b": 3})
    assert (tp, fp, fn) == (1, 0, 1) and mre == pytest.approx(0.2, abs=1e-15)
    assert p == 1.0 and r == 0.5 and f1 == pytest.approx(2 * 0.5 / 1.5, abs=1e-15)
