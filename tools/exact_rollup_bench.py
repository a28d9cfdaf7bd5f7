#!/usr/bin/env python3
"""The exact aggregator's roll-up against the two routes it replaces, on one GPU.

A five-tuple handle is filled with the synthetic stream (SyntheticTraffic(flows=N,
zipf_s=0.2), 12 packets per flow, so practically every flow is resident; default N = 2^22).
Then, in one child process under one time limit (a run that fails or runs out of time starts
nothing more on the GPU), for the layouts ["SrcIP"] (many groups), ["DstPort", "Protocol"] and
["Protocol"] (three groups: the case that shows whether the in-workgroup combine works):

  (a) rollup   host-visible time of gns_ex_rollup into a fresh handle of the layout (the
               handle is created outside the timed region, sized so that it does not grow,
               and once more with the smallest table so that it grows all the way)
  (b) host     the route built from the existing calls: snapshot_arrays(), a numpy projection
               and group-by (sums, min start, max end: the stream order of the flows is not
               in a snapshot, so its times are not the reference's), merge() into a fresh handle
  (c) second   what a second handle keyed on the layout costs while the traffic arrives:
               its ingest time per 100M packets of the same stream

One JSON goes to profiles/exact_rollup_<flows>.json.

    python tools/exact_rollup_bench.py [--flows 4194304] [--window 25000000] [--out profiles]
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
LAYOUTS = [["SrcIP"], ["DstPort", "Protocol"], ["Protocol"]]


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--flows", type=int, default=1 << 22)
    ap.add_argument("--packets-per-flow", type=int, default=12)
    ap.add_argument("--window", type=int, default=25_000_000, help="packets per ingest call of (c)")
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def fill(args, torch, dev, handles, total, zipf_s, timed=False):
    """`total` packets of the synthetic stream into every handle; the wall seconds each took."""
    from go2netspectra_amd import SyntheticTraffic
    syn = SyntheticTraffic(flows=args.flows, zipf_s=zipf_s, device=args.device)
    win = min(args.window if timed else 1 << 23, total)
    hdr = torch.empty((win, 64), dtype=torch.uint8, device=dev)
    wl = torch.empty((win,), dtype=torch.int32, device=dev)
    spent, done = [0.0] * len(handles), 0
    while done < total:
        m = min(win, total - done)
        syn.fill(hdr[:m], wl[:m], done)
        ts = torch.arange(done, done + m, dtype=torch.int64, device=dev) * 1000 + 1_700_000_000_000_000_000
        torch.cuda.synchronize()
        for i, h in enumerate(handles):
            t0 = time.perf_counter()
            h.insert_headers(hdr[:m], wl[:m], ts)
            h.flush()
            spent[i] += time.perf_counter() - t0
        done += m
    syn.close()
    return spent


def host_route(np, src, dst, plan):
    """snapshot -> numpy projection and group-by -> merge; the wall ms of the three parts."""
    t0 = time.perf_counter()
    keys, st, en, pk, by = src.snapshot_arrays()
    t1 = time.perf_counter()
    proj = np.ascontiguousarray(keys[:, plan])
    words = np.zeros((len(proj), (proj.shape[1] + 7) // 8 * 8), np.uint8)  # the key as 64-bit columns
    words[:, :proj.shape[1]] = proj
    words = words.view(">u8")
    _, first, inv = np.unique(words[:, 0] if words.shape[1] == 1 else words, axis=0, return_index=True,
                              return_inverse=True)
    inv = inv.ravel()
    order = np.argsort(inv, kind="stable")
    cuts = np.flatnonzero(np.diff(inv[order], prepend=-1))
    rows = (proj[first], np.minimum.reduceat(st[order], cuts), np.maximum.reduceat(en[order], cuts),
            np.add.reduceat(pk[order], cuts), np.add.reduceat(by[order], cuts))
    t2 = time.perf_counter()
    dst.merge(*rows)
    t3 = time.perf_counter()
    return {"snapshot_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3, "merge_ms": (t3 - t2) * 1e3,
            "total_ms": (t3 - t0) * 1e3, "groups": int(len(cuts))}


def child(args):
    import numpy as np
    import torch
    from go2netspectra_amd import ExactAggregator, rollup_plan
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host alone"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    src = ExactAggregator(FIVE, max_flows=args.flows, device=args.device)
    fill(args, torch, dev, [src], args.flows * args.packets_per_flow, 0.2)
    res = {"flows_target": args.flows, "flows_resident": src.counters()["flows"], "slots": src.dict_stats()["slots"],
           "reps": args.reps, "layouts": {}}
    for fields in LAYOUTS:
        name, r = "-".join(fields), {}
        ms, counts = [], None
        for rep in range(args.reps + 1):  # the first one warms up
            dst = ExactAggregator(fields, max_flows=args.flows, device=args.device)
            t0 = time.perf_counter()
            counts = dst.rollup_from(src)
            ms.append((time.perf_counter() - t0) * 1e3)
            if rep == args.reps:
                total = dst.aggregate([{}])[0]
            dst.close()
        r["rollup_wall_ms"] = sorted(ms[1:])[len(ms[1:]) // 2]
        r["rollup_wall_ms_all"] = [round(x, 3) for x in ms[1:]]
        r["projected"], r["groups"] = counts
        dst = ExactAggregator(fields, max_flows=1, device=args.device)
        t0 = time.perf_counter()
        dst.rollup_from(src)
        r["rollup_growing_wall_ms"] = (time.perf_counter() - t0) * 1e3
        r["growths"] = dst.dict_stats()["growths"]
        dst.close()
        dst = ExactAggregator(fields, max_flows=args.flows, device=args.device)
        r["host_route"] = host_route(np, src, dst, rollup_plan(FIVE, fields))
        host_total = dst.aggregate([{}])[0]
        dst.close()
        assert r["host_route"]["groups"] == r["groups"]
        assert (host_total.flows, host_total.packets, host_total.bytes) == (total.flows, total.packets, total.bytes)
        res["layouts"][name] = r
    # (c) a second handle per layout beside the five-tuple one, over the same windows
    second = [ExactAggregator(f, max_flows=args.flows, device=args.device) for f in LAYOUTS]
    seconds = fill(args, torch, dev, second, args.window * args.windows, 1.1, timed=True)
    for h in second:
        h.close()
    for fields, sec in zip(LAYOUTS, seconds):
        res["layouts"]["-".join(fields)]["second_handle_ms_per_100M_packets"] = sec * 1e3 * 1e8 / (args.window * args.windows)
    res["second_handle_packets"] = args.window * args.windows
    a = {k: v["rollup_wall_ms"] for k, v in res["layouts"].items()}
    res["protocol_vs_srcip"] = a["Protocol"] / a["SrcIP"]
    src.close()
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    args = parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--flows", str(args.flows), "--packets-per-flow",
           str(args.packets_per_flow), "--window", str(args.window), "--windows", str(args.windows), "--reps",
           str(args.reps), "--device", str(args.device)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s", file=sys.stderr)
        return 2
    if out.returncode != 0:
        print(f"exit {out.returncode}\n{out.stdout}\n{out.stderr}", file=sys.stderr)
        return 2
    res = json.loads(out.stdout.strip().splitlines()[-1])
    with open(os.path.join(args.out, f"exact_rollup_{args.flows}.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
