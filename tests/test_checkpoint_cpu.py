"""The write side of the state interface, the parts that need no GPU: the three C
symbols exist (library and header) and reject a null handle, and the checkpoint
file format round-trips, compares its metadata field by field and rejects a
truncated file."""
import ctypes as ct
import os

import numpy as np
import pytest

import go2netspectra_amd as g
from go2netspectra_amd import _lib, checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gns_cm_import_state", "gns_ss_import_state", "gns_ex_merge")


def test_symbols_in_library_and_header():
    L = g.load()
    with open(os.path.join(ROOT, "include", "gns_sketch.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name


def test_null_handle_is_an_argument_error():
    L = g.load()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    assert L.gns_cm_import_state(None, p, p, p, p, None) == _lib.GNS_E_ARG
    assert L.gns_ss_import_state(None, p, p, p, p, 0, None) == _lib.GNS_E_ARG
    assert L.gns_ex_merge(None, p, p, p, p, p, 1, _lib.MEM_HOST) == _lib.GNS_E_ARG


def _arrays(rng):
    return {"C": rng.integers(0, 2**32, 24, dtype=np.uint64).astype(np.uint32),
            "FPc": rng.integers(0, 256, (24, 13), dtype=np.uint8),
            "pbits": rng.random(24).view(np.uint64),
            "start": rng.integers(-(1 << 60), 1 << 60, 7).astype(np.int64),
            "empty": np.zeros((0, 37), np.uint8)}


META = {"CountMin": {"format": 1, "class": "CountMin", "width": 4096, "depth": 4, "key_bytes": 37,
                     "flow_fields": ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"], "size_threshold": 100000,
                     "count_threshold": 50, "seeds": [1, 2, 3, 4], "bucket_range": None, "counters": [5, 6, 7]},
        "SuperSpread": {"format": 1, "class": "SuperSpread", "width": 4096, "depth": 2, "flow_bytes": 16,
                        "elem_bytes": 16, "flow_fields": ["SrcIP"], "elem_fields": ["DstIP"], "threshold": 1,
                        "seeds": None, "m": 128, "size": 5, "base": 0.5, "b": 1.08,
                        "hll_master": 0x1234ABCD5678EF01, "rng_seed": 0x0DDBA11CAFEF00D5, "records": 99,
                        "counters": [1, 2, 3]},
        "ExactAggregator": {"format": 1, "class": "ExactAggregator", "key_fields": ["SrcIP"], "key_bytes": 16}}


def test_file_round_trip_keeps_dtypes_shapes_and_metadata(tmp_path):
    arrays = _arrays(np.random.default_rng(1))
    path = tmp_path / "state.npz"
    checkpoint.write(path, META["SuperSpread"], arrays)
    assert os.path.exists(path) and not os.path.exists(str(path) + ".npz")
    meta, got = checkpoint.read(path)
    assert meta == META["SuperSpread"]  # 64-bit seeds survive the JSON record
    assert sorted(got) == sorted(arrays)
    for k, a in arrays.items():
        assert got[k].dtype == a.dtype and got[k].shape == a.shape and np.array_equal(got[k], a), k


def _changed(v):
    if v is None:
        return [9]
    if isinstance(v, list):
        return v[:-1] if v else ["SrcIP"]
    if isinstance(v, float):
        return v + 0.25
    if isinstance(v, int):
        return v + 1
    return str(v) + "x"


@pytest.mark.parametrize("cls", sorted(META))
def test_each_metadata_field_is_compared_and_named(cls):
    live = META[cls]
    checkpoint.check_meta(dict(live), live)
    other = dict(live, counters=[0, 0, 0], records=0)  # state, not parameters: never compared
    checkpoint.check_meta(other, live)
    for name in ["class"] + checkpoint.PARAMS[cls]:
        saved = dict(live)
        saved[name] = _changed(live[name])
        with pytest.raises(ValueError, match=f"'{name}'"):
            checkpoint.check_meta(saved, live)
        if name != "class":
            del saved[name]
            with pytest.raises(ValueError, match=f"'{name}'"):
                checkpoint.check_meta(saved, live)


def test_first_differing_field_is_the_one_named():
    live = META["CountMin"]
    saved = dict(live, depth=3, seeds=[4, 3, 2, 1])
    with pytest.raises(ValueError, match="'depth'"):
        checkpoint.check_meta(saved, live)


def test_truncated_and_foreign_files_raise(tmp_path):
    arrays = _arrays(np.random.default_rng(2))
    path = tmp_path / "state.npz"
    checkpoint.write(path, META["CountMin"], arrays)
    blob = open(path, "rb").read()
    for cut in (len(blob) // 2, len(blob) - 10, 20, 0):
        short = tmp_path / f"cut{cut}.npz"
        with open(short, "wb") as f:
            f.write(blob[:cut])
        with pytest.raises(Exception):
            checkpoint.read(short)
    plain = tmp_path / "plain.npz"
    with open(plain, "wb") as f:
        np.savez(f, C=arrays["C"])
    with pytest.raises(ValueError):
        checkpoint.read(plain)
    with pytest.raises(ValueError):
        checkpoint.write(tmp_path / "x.npz", META["CountMin"], {"__meta__": arrays["C"]})
