"""The reference's accuracy protocol for heavy hitters and superspreaders.

evaluate_heavy_hitters mirrors evaluateHeavyHitters (cm_test.go:191-229);
spread_report runs the SuperSpread evaluation of ss_test.go:86-136 with an
ExactSpread as the ground-truth map: per-flow relative error over every seen
flow, and precision / recall / F1 of the detected superspreaders.
"""
from __future__ import annotations

from typing import Dict, Tuple


def evaluate_heavy_hitters(detected: Dict[bytes, int], truth: Dict[bytes, int]
                           ) -> Tuple[float, float, float, float, int, int, int]:
    """(mre, precision, recall, f1, tp, fp, fn) of cm_test.go:191-229.

    detected: key -> estimated value, truth: key -> actual value.  mre is the mean
    of |est - actual| / actual over the true positives; every ratio whose
    denominator is zero stays 0, as in the reference."""
    mre_sum = 0.0
    tp = fp = fn = 0
    for key, est in detected.items():
        if key in truth:
            actual = truth[key]
            tp += 1
            mre_sum += abs((int(est) - int(actual)) / float(actual))
        else:
            fp += 1
    for key in truth:
        if key not in detected:
            fn += 1
    mre = precision = recall = f1 = 0.0
    if tp > 0:
        mre = mre_sum / tp
    if tp + fp > 0:
        precision = tp / (tp + fp)
    if tp + fn > 0:
        recall = tp / (tp + fn)
    if precision + recall > 0:
        f1 = 2 * (precision * recall) / (precision + recall)
    return mre, precision, recall, f1, tp, fp, fn


def spread_report(sketch, exact, threshold: int) -> dict:
    """The ss_test.go:86-136 protocol: ``sketch`` (a SuperSpread) against ``exact`` (an
    ExactSpread fed the same stream).

    Every flow of exact.snapshot_arrays() is queried in the sketch on the device
    (query_many on a device tensor); ``are`` is the mean over those flows of
    |est - truth| / truth.  ss_test.go:94 as written computes est - truth/truth =
    est - 1 (an operator-precedence slip: the division binds before the
    subtraction); the intended formula is implemented here.  The detected
    superspreaders, sketch.heavy_hitters(), are compared with the true ones,
    exact.heavy_hitters(threshold), through evaluate_heavy_hitters."""
    import torch

    flows, truth = exact.snapshot_arrays()
    n = int(len(truth))
    are = 0.0
    if n:
        dev = torch.device("cuda", sketch.device)
        est = sketch.query_many(torch.from_numpy(flows).to(dev)).to(torch.float64)
        tru = torch.from_numpy(truth.astype("int64")).to(dev).to(torch.float64)
        are = float(((est - tru).abs() / tru).sum().item()) / n
    detected = {h.Flow: h.Count for h in sketch.heavy_hitters().Count}
    true_ss = {h.Flow: h.Count for h in exact.heavy_hitters(threshold).Count}
    mre, precision, recall, f1, tp, fp, fn = evaluate_heavy_hitters(detected, true_ss)
    return {"are": are, "mre": mre, "precision": precision, "recall": recall, "f1": f1, "tp": tp, "fp": fp,
            "fn": fn, "flows": n, "true_superspreaders": len(true_ss)}
