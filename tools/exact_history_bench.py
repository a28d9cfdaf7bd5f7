#!/usr/bin/env python3
"""The exact history (gns_ex_hist_*) against the view scan it extends and the host route it
replaces, on one GPU.

For each table size (resident five-tuple flows; default 2^22) a handle is filled with the
synthetic stream (SyntheticTraffic(flows=N, zipf_s=0.2), 12 packets per flow), then, in ONE
child process under a time limit (a child that fails or runs out of time ends the run:
nothing more is started on the GPU):

  append     wall time of history.append of a whole view into an empty history (every key
             new), of the same whole view again (every key known), and of each of nine
             delta views of about --delta of the flows (a window of uniform-ish packets)
  as-of      wall time of history.aggregate of 1 and of 64 filters at the newest snapshot
             after ONE whole view, next to view.aggregate of the same view in the same run
             (existing code over the same rows: the baseline is not the code under test),
             the answers asserted equal; then the same two aggregates at the oldest and at
             the newest of the 10 snapshots, after the nine deltas
  host       the route without the history: the ten exports concatenated on the host, then
             a numpy latest-per-key group-by and the sums of one open filter as of the
             newest snapshot (export time and group-by time apart), the totals asserted
             equal to the device's

Times are medians over --reps calls after --warmup, with the smallest and the largest.
One JSON per size goes to profiles/exact_history_<flows>.json.

    python tools/exact_history_bench.py [--flows 4194304] [--out profiles]
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


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--flows", type=int, nargs="+", default=[1 << 22])
    ap.add_argument("--packets-per-flow", type=int, default=12)
    ap.add_argument("--delta", type=float, default=0.10, help="fraction of the flows a delta window touches")
    ap.add_argument("--deltas", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def timed(args, fn):
    """(last result, {median, min, max} ms) of fn over --reps calls after --warmup."""
    for _ in range(args.warmup):
        fn()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return out, {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def filters64():
    """64 filters of the kinds a dashboard sends: totals, protocols, ports, subnets."""
    from go2netspectra_amd import make_filter
    out = [make_filter(), make_filter(protocol=6), make_filter(protocol=17)]
    out += [make_filter(dst_port=p) for p in (53, 80, 123, 443, 8080)]
    out += [make_filter(src_ip=f"{a}.0.0.0/8") for a in range(1, 29)]
    out += [make_filter(dst_ip=f"10.{a}.0.0/16", protocol=6) for a in range(28)]
    return out[:64]


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
    rows_whole = view.aggregate([make_filter()])[0].flows
    res = {"key_bytes": agg.key_bytes, "reps": args.reps, "warmup": args.warmup, "rows_whole_view": rows_whole}

    one, many = [make_filter()], filters64()
    exports = []

    # --- one whole view ---
    hist = ExactHistory(FIVE, max_rows=2 * target, max_flows=target, device=args.device)
    out, ms = once(lambda: hist.append(view, 0))
    assert out == (rows_whole, rows_whole), out
    res["append_whole_new_keys_ms"] = ms
    exports.append(once(view.snapshot_arrays))
    asof = {}
    for name, flt in (("1", one), ("64", many)):
        want, tv = timed(args, lambda: view.aggregate(flt))
        got, th = timed(args, lambda: hist.aggregate(flt))
        assert got == want, "history of one whole view differs from the view"
        asof[name] = {"view_aggregate": tv, "hist_aggregate": th,
                      "extra_ms": th["median_ms"] - tv["median_ms"], "view_spread_ms": tv["max_ms"] - tv["min_ms"]}
    res["one_whole_view"] = asof
    totals_t0 = hist.aggregate(one)[0]

    # --- nine deltas ---
    npk = int(-np.log(1.0 - args.delta) * target)  # uniform draws touching ~delta of the flows
    appends = []
    for i in range(args.deltas):
        insert(syn, npk)
        cursor = view.refresh(cursor)
        out, ms = once(lambda: hist.append(view, 10 * (i + 1)))
        appends.append({"rows": out[0], "new_keys": out[1], "ms": ms})
        exports.append(once(view.snapshot_arrays))
    res["append_delta"] = appends
    res["delta_rows_fraction"] = sum(a["rows"] for a in appends) / max(len(appends), 1) / rows_whole
    asof = {}
    for name, flt in (("1", one), ("64", many)):
        old, t_old = timed(args, lambda: hist.aggregate(flt, end_time=5))
        new, t_new = timed(args, lambda: hist.aggregate(flt))
        asof[name] = {"oldest_of_10": t_old, "newest_of_10": t_new}
        assert old[0] == totals_t0 if name == "1" else True
    res["after_nine_deltas"] = asof
    res["stats"] = hist.stats()
    totals = hist.aggregate(one)[0]

    # --- the host route: exports concatenated, latest row per key, the open filter's sums ---
    res["host_export_ms_total"] = sum(ms for _, ms in exports)

    def host_route():
        keys = np.concatenate([e[0][0] for e in exports])
        pk = np.concatenate([e[0][3] for e in exports])
        by = np.concatenate([e[0][4] for e in exports])
        kv = np.ascontiguousarray(keys[::-1]).view(np.dtype((np.void, keys.shape[1]))).reshape(-1)
        _, first = np.unique(kv, return_index=True)  # the first from the end: the latest row of the key
        return len(first), int(pk[::-1][first].sum(dtype=np.uint64)), int(by[::-1][first].sum(dtype=np.uint64))
    got, ms = once(host_route)
    assert got == (totals.flows, totals.packets, totals.bytes), (got, totals)
    res["host_groupby_ms"] = ms

    # --- a whole view again: every key known ---
    view.refresh()
    out, ms = once(lambda: hist.append(view, 1000))
    res["append_whole_known_keys_ms"] = ms
    res["append_whole_known_rows"] = out[0]
    syn.close()
    hist.close()
    view.close()
    agg.close()
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
        with open(os.path.join(args.out, f"exact_history_{target}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
