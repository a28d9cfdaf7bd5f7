#!/usr/bin/env python3
"""The history roll-up (gns_ex_hist_rollup) against the host route it replaces and against the
live roll-up of the same rows, on one GPU.

The workload is tools/exact_history_bench.py's: a handle filled with the synthetic stream
(SyntheticTraffic(flows=N, zipf_s=0.2), 12 packets per flow; default N = 2^22 five-tuple
flows), one whole view and nine delta views of about --delta of the flows appended to a
history: ten snapshots.  Then, in ONE child process under a time limit (a child that fails or
runs out of time ends the run: nothing more is started on the GPU), for the roll-ups to SrcIP,
to SrcIP at /24, to (DstPort, Protocol) and to the same five-tuple layout, each as of the newest
and as of the middle snapshot:

  hist_rollup   wall time of ExactAggregator.rollup_from_history into an empty handle
  host route    ExactHistory.snapshot_arrays(T) -> ExactAggregator.merge into an empty
                five-tuple handle -> rollup_from into an empty handle of the layout, the three
                steps timed apart
  live_rollup   the last of those steps alone: gns_ex_rollup[_prefix] of a live table holding
                the same rows (existing code: the baseline is not the code under test)

Every destination is created outside the timed region with room for the flows it receives.
The flows / packets / bytes totals of the new call and of the host route are asserted equal.
Times are medians over --reps calls after --warmup, with the smallest and the largest.  One JSON
per size goes to profiles/exact_history_rollup_<flows>.json.

    python tools/exact_history_rollup_bench.py [--flows 4194304] [--out profiles]
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
CASES = [("SrcIP", ["SrcIP"], None), ("SrcIP_24", ["SrcIP"], {"SrcIP": (24, 64)}),
         ("DstPort_Protocol", ["DstPort", "Protocol"], None), ("same_layout", FIVE, None)]


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--flows", type=int, nargs="+", default=[1 << 22])
    ap.add_argument("--packets-per-flow", type=int, default=12)
    ap.add_argument("--delta", type=float, default=0.10, help="fraction of the flows a delta window touches")
    ap.add_argument("--deltas", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def child(args, target):
    import numpy as np
    import torch
    from go2netspectra_amd import ExactAggregator, ExactHistory, SyntheticTraffic, make_filter
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host alone"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    agg = ExactAggregator(FIVE, max_flows=target, device=args.device)
    win = 1 << 23
    hdr = torch.empty((win, 64), dtype=torch.uint8, device=dev)
    wl = torch.empty((win,), dtype=torch.int32, device=dev)
    pos = [0]

    def insert(syn, n):
        done = 0
        while done < n:
            m = min(win, n - done)
            syn.fill(hdr[:m], wl[:m], pos[0])
            ts = torch.arange(pos[0], pos[0] + m, dtype=torch.int64, device=dev) * 1000 + 1_700_000_000_000_000_000
            agg.insert_headers(hdr[:m], wl[:m], ts)
            agg.flush()
            done += m
            pos[0] += m

    syn = SyntheticTraffic(flows=target, zipf_s=0.2, device=args.device)
    insert(syn, target * args.packets_per_flow)
    view = agg.view()
    cursor = view.refresh()
    hist = ExactHistory(FIVE, max_rows=2 * target, max_flows=target, device=args.device)
    hist.append(view, 0)
    npk = int(-np.log(1.0 - args.delta) * target)  # uniform draws touching ~delta of the flows
    for i in range(args.deltas):
        insert(syn, npk)
        cursor = view.refresh(cursor)
        hist.append(view, 10 * (i + 1))
    del hdr, wl
    view.close()
    agg.close()
    syn.close()
    times = hist.times()
    res = {"reps": args.reps, "warmup": args.warmup, "stats": hist.stats(), "cases": {}}
    whens = [("newest", None), ("middle", times[len(times) // 2])]
    total = lambda a: (lambda s: (s.flows, s.packets, s.bytes))(a.aggregate([make_filter()])[0])
    for wname, T in whens:
        live = hist.aggregate([make_filter()], end_time=T)[0].flows
        for cname, fields, prefix in CASES:
            new_ms, exp_ms, mrg_ms, rol_ms, groups = [], [], [], [], None
            for rep in range(args.warmup + args.reps):
                # the new call
                dst = ExactAggregator(fields, max_flows=live, device=args.device)
                out, ms = clock(lambda: dst.rollup_from_history(hist, end_time=T, prefix=prefix))
                assert out[0] == live, out
                got = total(dst)
                dst.close()
                # the host route: export, merge, live roll-up
                arrays, e_ms = clock(lambda: hist.snapshot_arrays(end_time=T))
                tmp = ExactAggregator(FIVE, max_flows=live, device=args.device)
                _, m_ms = clock(lambda: tmp.merge(*arrays))
                dst = ExactAggregator(fields, max_flows=live, device=args.device)
                _, r_ms = clock(lambda: dst.rollup_from(tmp, prefix=prefix))
                assert total(dst) == got, (cname, wname, total(dst), got)
                dst.close()
                tmp.close()
                del arrays
                if rep >= args.warmup:
                    new_ms.append(ms); exp_ms.append(e_ms); mrg_ms.append(m_ms); rol_ms.append(r_ms)
                groups = got[0]
            host = [a + b + c for a, b, c in zip(exp_ms, mrg_ms, rol_ms)]
            res["cases"][f"{cname}@{wname}"] = {
                "live_rows": live, "groups": groups, "hist_rollup": stats(new_ms), "host_route": stats(host),
                "host_export": stats(exp_ms), "host_merge": stats(mrg_ms), "live_rollup": stats(rol_ms)}
    hist.close()
    return res


def main() -> int:
    args = parse_args()
    if args.child:
        print(json.dumps(child(args, args.flows[0])), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    for target in args.flows:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--flows", str(target), "--packets-per-flow",
               str(args.packets_per_flow), "--delta", str(args.delta), "--deltas", str(args.deltas), "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--device", str(args.device)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{target} flows: no result within {args.timeout} s; stopping", file=sys.stderr)
            return 2
        if out.returncode != 0:
            print(f"{target} flows: exit {out.returncode}; stopping\n{out.stdout}\n{out.stderr}", file=sys.stderr)
            return 2
        res = dict({"flows_target": target, "packets_filled": target * args.packets_per_flow},
                   **json.loads(out.stdout.strip().splitlines()[-1]))
        print(f"{target}: {json.dumps(res)}", flush=True)
        with open(os.path.join(args.out, f"exact_history_rollup_{target}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
