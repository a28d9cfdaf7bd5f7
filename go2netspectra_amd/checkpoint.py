"""Checkpoint files: an engine's whole state in one ``.npz``, and back.

The reference keeps a measurement period's state in process memory only (SURVEY
§5 "Checkpoint/resume: no"); here it lives in HBM.  ``save`` exports it through
the engines' read side (gns_cm_export_state, gns_ss_export_state or a
SuperSpread view's gns_ss_view_export_state, gns_ex_snapshot, gns_pairs_export, gns_ex_hist_export), ``restore`` puts it back through the write
side (gns_cm_import_state, gns_ss_import_state, gns_ex_merge / gns_pairs_merge
into an emptied table, gns_ex_hist_append_rows per snapshot into a cleared history).

A file holds the state arrays plus one metadata record (JSON): the class and
the parameters a state depends on -- geometry, key layout, thresholds, row seeds
as given, for SuperSpread also m, size, base, b, hll_master, rng_seed -- and the
part of the state that is no array (``records``, the counters).  The C side
cannot detect a state loaded under other seeds, so ``restore`` compares the
parameters with the live object first and raises ValueError naming the first
field that differs.

``write`` / ``read`` / ``check_meta`` are the pure file part: numpy only, usable
without a GPU.
"""
from __future__ import annotations

import json
from typing import Dict, Tuple

import numpy as np

FORMAT = 1
_META = "__meta__"

# parameters compared by restore, in the order they are reported
PARAMS = {
    "CountMin": ["width", "depth", "key_bytes", "flow_fields", "size_threshold", "count_threshold", "seeds",
                 "bucket_range"],
    "SuperSpread": ["width", "depth", "flow_bytes", "elem_bytes", "flow_fields", "elem_fields", "threshold", "seeds",
                    "m", "size", "base", "b", "hll_master", "rng_seed"],
    "ExactAggregator": ["key_fields", "key_bytes"],
    "ExactSpread": ["flow_fields", "elem_fields", "flow_bytes", "elem_bytes"],
    "ExactHistory": ["key_fields", "key_bytes"],
}
# the arrays a file of each class holds
ARRAYS = {
    "CountMin": ["C", "S", "FPc", "FPs"],
    "SuperSpread": ["values", "keys", "regs", "pbits"],
    "ExactAggregator": ["keys", "start", "end", "pkts", "bytes"],
    "ExactSpread": ["flows", "elems"],
    # the log rows in log order with the snapshot that wrote each, and the snapshot times (int64)
    "ExactHistory": ["keys", "start", "end", "pkts", "bytes", "written", "times"],
}


def history_slices(written: np.ndarray, n_snapshots: int):
    """[(lo, hi)] per snapshot: the rows of one snapshot are contiguous in an exported log
    (``written`` never decreases); a snapshot without rows gets an empty range.  ValueError
    for a ``written`` that is not sorted or names a snapshot that ``times`` lacks."""
    w = np.asarray(written, np.int64)
    if w.size and (np.any(np.diff(w) < 0) or w[0] < 0 or w[-1] >= n_snapshots):
        raise ValueError("history file: 'written' is not a sorted list of snapshot numbers below len(times)")
    edges = np.searchsorted(w, np.arange(n_snapshots + 1), side="left")
    return [(int(edges[i]), int(edges[i + 1])) for i in range(n_snapshots)]


def write(path, meta: dict, arrays: Dict[str, np.ndarray]) -> None:
    """One .npz at exactly ``path``: the arrays as given (dtype and shape kept) and ``meta``."""
    if _META in arrays:
        raise ValueError(f"array name {_META!r} is reserved")
    rec = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    with open(path, "wb") as f:
        np.savez(f, **{_META: rec}, **{k: np.asarray(v) for k, v in arrays.items()})


def read(path) -> Tuple[dict, Dict[str, np.ndarray]]:
    """(meta, arrays) of a file ``write`` made; a truncated or foreign file raises."""
    with np.load(path, allow_pickle=False) as z:
        if _META not in z.files:
            raise ValueError(f"{path}: not a checkpoint (no metadata record)")
        meta = json.loads(bytes(z[_META]).decode())
        arrays = {k: z[k] for k in z.files if k != _META}  # every member is read here
    if meta.get("format") != FORMAT:
        raise ValueError(f"{path}: checkpoint format {meta.get('format')!r}, expected {FORMAT}")
    return meta, arrays


def _plain(v):
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        return [_plain(x) for x in v.tolist()]
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


def describe(obj) -> dict:
    """The metadata record of a live CountMin / SuperSpread / ExactAggregator / ExactSpread /
    ExactHistory (no state)."""
    cls = type(obj).__name__
    if cls not in PARAMS:
        raise TypeError(f"no checkpoint format for {cls}")
    meta = {"format": FORMAT, "class": cls}
    for name in PARAMS[cls]:
        meta[name] = _plain(getattr(obj, "_seeds" if name == "seeds" else name))
    return meta


def check_meta(saved: dict, live: dict) -> None:
    """ValueError naming the first parameter of ``saved`` that differs from ``live``."""
    if saved.get("class") != live.get("class"):
        raise ValueError(f"checkpoint field 'class' differs: file {saved.get('class')!r}, object {live.get('class')!r}")
    for name in PARAMS.get(live["class"], []):
        if name not in saved:
            raise ValueError(f"checkpoint field {name!r} is missing from the file")
        if saved[name] != live[name]:
            raise ValueError(f"checkpoint field {name!r} differs: file {saved[name]!r}, object {live[name]!r}")


def save(obj, path) -> None:
    """Export ``obj``'s state (after its pending inserts) into one file.  A SuperSpreadView
    refreshed with state=True, or a CountMinView refreshed with detach=True, writes the file
    its sketch would have written at the refresh -- from any thread, while the sketch keeps
    ingesting."""
    if type(obj).__name__ == "SuperSpreadView":
        meta = describe(obj.parent)
        v, k, r, p = obj.export_state()
        c = obj.counters()
        meta["counters"] = [c["inserted"], c["dropped"], c["unsupported"]]
        meta["records"] = c["records"]
        write(path, meta, {"values": v, "keys": np.ascontiguousarray(k), "regs": r, "pbits": p.view(np.uint64)})
        return
    if type(obj).__name__ == "CountMinView":  # a detached snapshot: the file of the refresh point
        meta = describe(obj.parent)
        c = obj.counters()  # raises on a plain snapshot, before anything is exported
        C, S, Fc, Fs = obj.export_state()
        meta["counters"] = [int(c["inserted"]), int(c["dropped"]), int(c["unsupported"])]
        write(path, meta, {"C": C, "S": S, "FPc": np.ascontiguousarray(Fc), "FPs": np.ascontiguousarray(Fs)})
        return
    meta = describe(obj)
    cls = meta["class"]
    if cls == "CountMin":
        C, S, Fc, Fs = obj.export_state()
        arrays = {"C": C, "S": S, "FPc": np.ascontiguousarray(Fc), "FPs": np.ascontiguousarray(Fs)}
        c = obj.counters()
        meta["counters"] = [int(c["inserted"]), int(c["dropped"]), int(c["unsupported"])]
    elif cls == "SuperSpread":
        v, k, r, p = obj.export_state()
        arrays = {"values": v, "keys": np.ascontiguousarray(k), "regs": r, "pbits": p.view(np.uint64)}
        c = obj.counters()
        meta["counters"] = [int(c["inserted"]), int(c["dropped"]), int(c["unsupported"])]
        meta["records"] = int(c["records"])
    elif cls == "ExactSpread":  # the pair set is the whole state; counters are not part of the file
        f, e, _ = obj.export_pairs()
        arrays = {"flows": np.ascontiguousarray(f), "elems": np.ascontiguousarray(e)}
    elif cls == "ExactHistory":  # the whole log: restore re-appends it snapshot by snapshot
        k, st, en, pk, by, wr, ts = obj.export_log()
        arrays = {"keys": np.ascontiguousarray(k), "start": st, "end": en, "pkts": pk, "bytes": by, "written": wr,
                  "times": np.asarray(ts, np.int64)}
    else:
        k, st, en, pk, by = obj.snapshot_arrays()
        arrays = {"keys": np.ascontiguousarray(k), "start": st, "end": en, "pkts": pk, "bytes": by}
    write(path, meta, arrays)


def restore(obj, path) -> None:
    """Replace ``obj``'s state by the file's.  The file's parameters must equal the object's."""
    meta, arrays = read(path)
    live = describe(obj)
    check_meta(meta, live)
    cls = live["class"]
    for name in ARRAYS[cls]:
        if name not in arrays:
            raise ValueError(f"{path}: array {name!r} is missing")
    if cls == "CountMin":
        obj.import_state(arrays["C"], arrays["S"], arrays["FPc"], arrays["FPs"],
                         counters=np.array(meta["counters"], np.uint64))
    elif cls == "SuperSpread":
        obj.import_state(arrays["values"], arrays["keys"], arrays["regs"], arrays["pbits"].view(np.float64),
                         meta["records"], counters=np.array(meta["counters"], np.uint64))
    elif cls == "ExactSpread":
        obj.reset()
        obj.merge_pairs(arrays["flows"], arrays["elems"])
    elif cls == "ExactHistory":
        ts = np.asarray(arrays["times"], np.int64)
        cuts = history_slices(arrays["written"], len(ts))  # (checked before anything is cleared)
        obj.clear()
        for t, (lo, hi) in zip(ts.tolist(), cuts):  # a snapshot without rows still registers its time
            obj.append_rows(arrays["keys"][lo:hi], arrays["start"][lo:hi], arrays["end"][lo:hi], arrays["pkts"][lo:hi],
                            arrays["bytes"][lo:hi], t)
    else:
        obj.reset()
        obj.merge(arrays["keys"], arrays["start"], arrays["end"], arrays["pkts"], arrays["bytes"])
