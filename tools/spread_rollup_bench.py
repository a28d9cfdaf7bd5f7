#!/usr/bin/env python3
"""The spread roll-up against the routes it stands beside, on one GPU.

The configs[2] stream of tools/spread_accuracy.py (SyntheticTraffic(fanout=2^20), flow SrcIP,
element DstIP, the default SuperSpread geometry) is generated on the device window by window;
every window goes to a five-tuple ExactAggregator, to an ExactSpread and to a SuperSpread.
Then, in one child process under one time limit (a run that fails or runs out of time starts
nothing more on the GPU):

  (1) rollup   gns_spread_rollup of the five-tuple table to SrcIP / DstIP, full, into a fresh
               handle sized so that it does not grow (every repeat: wall ms and the handle's
               stage times), and once into a handle of the default capacities
  (2) delta    one further window into the aggregator, then rollup_from(since=cursor) into the
               handle of (1): wall ms, rows projected, pairs added
  (3) ingest   what the ExactSpread fed the same packets from device memory cost, per window:
               the route that exists without the roll-up, while the packets are resident
  (4) host     snapshot_arrays() of the aggregator, numpy projection + form conversion
               (to16_to_encodeflow) + de-duplication, merge_pairs into a fresh handle
  (5) truth    accuracy.spread_report of the SuperSpread with the rolled-up handle as truth
               against the one fed directly: every field equal (``are`` is a float64 sum over the
               flows in snapshot order, which differs between two handles; it is compared to
               n * 2^-52 relative, the bound of a reordered sum, and both values are recorded)

One JSON goes to profiles/spread_rollup_<packets>.json.

    python tools/spread_rollup_bench.py [100000000] [--window 25000000] [--reps 3] [--out profiles]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
FLOW, ELEM = ["SrcIP"], ["DstIP"]
SS_W, SS_D, SS_M, SS_THR, SS_FANOUT = 32768, 2, 128, 4096, 1 << 20
SS_HLL, SS_RNG = 0x0123456789ABCDEF, 0x0DDBA11CAFEF00D5


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("packets", type=int, nargs="?", default=100_000_000)
    ap.add_argument("--window", type=int, default=25_000_000, help="packets generated and fed per step")
    ap.add_argument("--max-flows", type=int, default=1 << 26, help="the aggregator's initial capacity")
    ap.add_argument("--max-pairs", type=int, default=1 << 26, help="pre-sized spread handles: pair capacity")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def host_route(np, src, dst):
    """snapshot -> numpy projection, form conversion, de-duplication -> merge_pairs; wall ms of each."""
    from go2netspectra_amd import rollup_plan, to16_to_encodeflow
    t0 = time.perf_counter()
    keys = src.snapshot_arrays()[0]
    t1 = time.perf_counter()
    rows = to16_to_encodeflow(keys[:, rollup_plan(FIVE, FLOW + ELEM)], FLOW + ELEM)  # [n, 32]
    cols = np.ascontiguousarray(rows).view("<u8")
    order = np.lexsort(cols.T[::-1])
    cols = cols[order]
    keep = np.ones(len(cols), bool)
    keep[1:] = (cols[1:] != cols[:-1]).any(1)
    rows = cols[keep].view(np.uint8)
    t2 = time.perf_counter()
    dst.merge_pairs(rows[:, :16], rows[:, 16:])
    dst.flush()
    t3 = time.perf_counter()
    return {"snapshot_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3, "merge_ms": (t3 - t2) * 1e3,
            "total_ms": (t3 - t0) * 1e3, "rows_snapshot": int(len(keys)), "rows_merged": int(keep.sum())}


def same_table(np, a, b) -> bool:
    """Two spread handles hold the same flows and spreads (the canonical list of every flow)."""
    fa, va = a.heavy_hitters_arrays(1)
    fb, vb = b.heavy_hitters_arrays(1)
    return fa.shape == fb.shape and bool(np.array_equal(fa, fb)) and bool(np.array_equal(va, vb))


def child(args):
    import numpy as np
    import torch
    from go2netspectra_amd import ExactAggregator, ExactSpread, SuperSpread, SyntheticTraffic
    from go2netspectra_amd.accuracy import spread_report
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host alone"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    syn = SyntheticTraffic(device=args.device, fanout=SS_FANOUT)
    ss = SuperSpread(SS_W, SS_D, SS_THR, SS_M, 5, 0.5, 1.08, flow_fields=FLOW, elem_fields=ELEM,
                     hll_master=SS_HLL, rng_seed=SS_RNG, device=args.device)
    src = ExactAggregator(FIVE, max_flows=args.max_flows, device=args.device)
    cap_pairs = args.max_pairs  # the capacities of profiles/spread_accuracy_100m_presized.json: no growth at 125M packets
    ex = ExactSpread(FLOW, ELEM, max_flows=1 << 21, max_pairs=cap_pairs, batch_packets=args.window, device=args.device)
    win = min(args.window, args.packets)
    hdr = torch.empty((win, 64), dtype=torch.uint8, device=dev)
    wl = torch.empty((win,), dtype=torch.int32, device=dev)
    res = {"tool": "spread_rollup_bench", "packets": args.packets, "window": win, "reps": args.reps,
           "stream": "configs[2]: SyntheticTraffic(fanout=2^20), flow SrcIP, element DstIP",
           "ingest": {"aggregator_ms": [], "exact_spread_ms": []}}

    def feed(first, m, with_sketch):
        h, w = hdr[:m], wl[:m]
        syn.fill(h, w, first=first)
        ts = torch.arange(first, first + m, dtype=torch.int64, device=dev) * 1000 + 1_700_000_000_000_000_000
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        src.insert_headers(h, w, ts)
        src.flush()
        t1 = time.perf_counter()
        ex.insert_headers(h, w)
        ex.flush()
        t2 = time.perf_counter()
        res["ingest"]["aggregator_ms"].append(round((t1 - t0) * 1e3, 3))
        res["ingest"]["exact_spread_ms"].append(round((t2 - t1) * 1e3, 3))  # (3)
        if with_sketch:
            ss.insert_headers(h, w)
            ss.flush()

    done = 0
    while done < args.packets:
        m = min(win, args.packets - done)
        feed(done, m, True)
        done += m
    n_flows, n_pairs = src.counters()["flows"], ex.dict_stats()["pairs_claimed"]
    res.update(flows_five_tuple=n_flows, aggregator_slots=src.dict_stats()["slots"], pairs=n_pairs,
               flows_spread=ex.counters()["flows"])
    res["ingest"]["exact_spread_total_ms"] = round(sum(res["ingest"]["exact_spread_ms"]), 3)

    # (1) full roll-up, pre-sized, every repeat
    runs, rolled = [], None
    for rep in range(args.reps + 1):  # the first one warms up (module load, first allocation of the staging rows)
        if rolled is not None:
            rolled.close()
        rolled = ExactSpread(FLOW, ELEM, max_flows=1 << 21, max_pairs=cap_pairs, device=args.device)
        rolled.set_timing(True)
        t0 = time.perf_counter()
        cursor, projected, new = rolled.rollup_from(src)
        wall = (time.perf_counter() - t0) * 1e3
        st = rolled.stage_times()
        runs.append({"wall_ms": round(wall, 3), "projected": projected, "new_pairs": new,
                     "stage_ms": {k: round(v[0], 3) for k, v in st.items() if not k.startswith("unused")},
                     "launches": {k: int(v[1]) for k, v in st.items() if not k.startswith("unused")},
                     "growths": [rolled.dict_stats()["flow_growths"], rolled.dict_stats()["pair_growths"]]})
        rolled.set_timing(False)
        assert (projected, new) == (n_flows, n_pairs), (projected, new, n_flows, n_pairs)
    res["rollup"] = {"warmup": runs[0], "runs": runs[1:],
                     "wall_ms_median": sorted(r["wall_ms"] for r in runs[1:])[len(runs[1:]) // 2]}
    grown = ExactSpread(FLOW, ELEM, device=args.device)
    t0 = time.perf_counter()
    grown.rollup_from(src)
    res["rollup"]["default_capacities"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                                           "growths": [grown.dict_stats()["flow_growths"], grown.dict_stats()["pair_growths"]]}
    grown.close()
    res["rollup"]["equals_direct"] = same_table(np, rolled, ex)
    assert res["rollup"]["equals_direct"]

    # (5) the rolled-up handle as SuperSpread's truth
    r_rolled, r_direct = spread_report(ss, rolled, SS_THR), spread_report(ss, ex, SS_THR)
    tol = r_direct["flows"] * 2.0 ** -52 * max(abs(r_direct["are"]), 1e-300)
    same = all(r_rolled[k] == r_direct[k] for k in r_direct if k != "are") and abs(r_rolled["are"] - r_direct["are"]) <= tol
    res["spread_report"] = {"rolled_up": r_rolled, "direct": r_direct, "equal": bool(same),
                            "are_abs_diff": abs(r_rolled["are"] - r_direct["are"]), "are_tolerance": tol}
    assert same, res["spread_report"]

    # (4) the host route
    hosted = ExactSpread(FLOW, ELEM, max_flows=1 << 21, max_pairs=cap_pairs, device=args.device)
    res["host_route"] = host_route(np, src, hosted)
    res["host_route"]["equals_direct"] = same_table(np, hosted, ex)
    assert res["host_route"]["equals_direct"]
    hosted.close()

    # (2) one further window, then the delta
    feed(done, win, False)
    rolled.set_timing(True)
    rolled.stage_times(reset=True)
    t0 = time.perf_counter()
    c2, projected, new = rolled.rollup_from(src, since=cursor)
    wall = (time.perf_counter() - t0) * 1e3
    st = rolled.stage_times()
    res["delta"] = {"window": win, "wall_ms": round(wall, 3), "projected": projected, "new_pairs": new,
                    "flows_five_tuple_after": src.counters()["flows"], "cursor": [cursor, c2],
                    "stage_ms": {k: round(v[0], 3) for k, v in st.items() if not k.startswith("unused")},
                    "exact_spread_window_ms": res["ingest"]["exact_spread_ms"][-1],
                    "equals_direct": same_table(np, rolled, ex)}
    assert res["delta"]["equals_direct"] and projected == src.counters()["flows"] - n_flows
    for h in (rolled, ex, src, ss):
        h.close()
    syn.close()
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    args = parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), str(args.packets), "--child", "--window", str(args.window),
           "--max-flows", str(args.max_flows), "--max-pairs", str(args.max_pairs), "--reps", str(args.reps), "--device", str(args.device)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s", file=sys.stderr)
        return 2
    if out.returncode != 0:
        print(f"exit {out.returncode}\n{out.stdout}\n{out.stderr}", file=sys.stderr)
        return 2
    res = json.loads(out.stdout.strip().splitlines()[-1])
    with open(os.path.join(args.out, f"spread_rollup_{args.packets}.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
