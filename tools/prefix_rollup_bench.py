#!/usr/bin/env python3
"""The prefix roll-up, CIDR filters and hierarchical heavy hitters against the calls they extend
and the host route they replace, on one GPU.

A five-tuple handle is filled with the synthetic stream (SyntheticTraffic(flows=N, zipf_s=0.2),
12 packets per flow, so practically every flow is resident; default N = 2^22).  Then, in one
child process under one time limit (a run that fails or runs out of time starts nothing more on
the GPU), with interleaved repeats (every repeat in the JSON, the median beside them):

  rollup   gns_ex_rollup to ["SrcIP"] -- the yardstick -- and gns_ex_rollup_prefix to
           ["SrcIP"] at the full prefix, /24, /16 and /8 (IPv6: /128, /64, /48, /32), each into
           a fresh handle sized so that it does not grow
  chain    /24 -> /16 -> /8 chained against the three rolled up directly
  spread   hosts per source /24 (gns_spread_rollup_prefix, flow SrcIP under /24, element SrcIP)
           against gns_spread_rollup to SrcIP / DstIP
  cidr     a batch of 64 CIDR filters against a batch of 64 equality filters
  hhh      four-level hierarchical heavy hitters of SrcIP, end to end
  host     the host route to "bytes per source /24": snapshot_arrays(), mask_prefix, numpy group-by

One JSON goes to profiles/prefix_rollup_<flows>[_<tag>].json.  GNS_LIB selects another build of
the library (an A/B of the projection kernel: --tag names it, --only rollup keeps to that part).

    python tools/prefix_rollup_bench.py [--flows 4194304] [--reps 5] [--out profiles]
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
LEVELS = [("full", (32, 128)), ("/24", (24, 64)), ("/16", (16, 48)), ("/8", (8, 32))]


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--flows", type=int, default=1 << 22)
    ap.add_argument("--packets-per-flow", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the whole run")
    ap.add_argument("--only", default="", help="comma list of parts (rollup, chain, spread, cidr, hhh, host); default all")
    ap.add_argument("--tag", default="", help="suffix of the output file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def fill(args, torch, dev, handle, total):
    from go2netspectra_amd import SyntheticTraffic
    syn = SyntheticTraffic(flows=args.flows, zipf_s=0.2, device=args.device)
    win = min(1 << 23, total)
    hdr = torch.empty((win, 64), dtype=torch.uint8, device=dev)
    wl = torch.empty((win,), dtype=torch.int32, device=dev)
    done = 0
    while done < total:
        m = min(win, total - done)
        syn.fill(hdr[:m], wl[:m], done)
        ts = torch.arange(done, done + m, dtype=torch.int64, device=dev) * 1000 + 1_700_000_000_000_000_000
        torch.cuda.synchronize()
        handle.insert_headers(hdr[:m], wl[:m], ts)
        handle.flush()
        done += m
    syn.close()


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    """Repeats after the warm-up one."""
    return {"ms": round(median(ms[1:]), 3), "all": [round(x, 3) for x in ms[1:]]}


def child(args):
    import numpy as np
    import torch
    from go2netspectra_amd import ExactAggregator, ExactSpread, make_filter, mask_prefix
    from go2netspectra_amd.exact import as_cidr
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host alone"
    parts = set(filter(None, args.only.split(","))) or {"rollup", "chain", "spread", "cidr", "hhh", "host"}
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    src = ExactAggregator(FIVE, max_flows=args.flows, device=args.device)
    fill(args, torch, dev, src, args.flows * args.packets_per_flow)
    n_src = src.counters()["flows"]
    res = {"flows_target": args.flows, "flows_resident": n_src, "slots": src.dict_stats()["slots"], "reps": args.reps,
           "library": os.path.basename(os.environ.get("GNS_LIB", "libgns_sketch.so")), "parts": sorted(parts)}

    def rolled(source, prefix, max_flows):
        dst = ExactAggregator(["SrcIP"], max_flows=max_flows, device=args.device)
        ms, counts = timed(lambda: dst.rollup_from(source, prefix=prefix))
        return ms, counts, dst

    if "rollup" in parts:
        names = ["gns_ex_rollup"] + [n for n, _ in LEVELS]
        ms, counts = {n: [] for n in names}, {}
        for _ in range(args.reps + 1):  # interleaved; the first repeat warms up
            for n, prefix in [("gns_ex_rollup", None)] + [(n, {"SrcIP": lv}) for n, lv in LEVELS]:
                t, counts[n], dst = rolled(src, prefix, args.flows)
                ms[n].append(t)
                dst.close()
        res["rollup"] = {n: dict(summary(ms[n]), projected=counts[n][0], groups=counts[n][1]) for n in names}
        assert all(c[0] == n_src for c in counts.values()) and counts["full"] == counts["gns_ex_rollup"]
    if "chain" in parts:
        chain, direct = [], []
        for _ in range(args.reps + 1):
            cur, made, t = src, [], 0.0
            for _, lv in LEVELS[1:]:
                dt, _, cur = rolled(cur, {"SrcIP": lv}, args.flows)
                made.append(cur)
                t += dt
            chain.append(t)
            t = 0.0
            for (_, lv), ch in zip(LEVELS[1:], made):
                dt, _, d = rolled(src, {"SrcIP": lv}, args.flows)
                t += dt
                assert d.counters()["flows"] == ch.counters()["flows"]
                d.close()
                ch.close()
            direct.append(t)
        res["chain"] = {"chained_24_16_8": summary(chain), "direct_24_16_8": summary(direct)}
    if "spread" in parts:
        ms = {"gns_spread_rollup SrcIP/DstIP": [], "hosts per /24": []}
        info = {}
        for _ in range(args.reps + 1):
            for n, flow, elem, fpx in (("gns_spread_rollup SrcIP/DstIP", ["SrcIP"], ["DstIP"], None),
                                       ("hosts per /24", ["SrcIP"], ["SrcIP"], {"SrcIP": (24, 64)})):
                sp = ExactSpread(flow, elem, max_flows=args.flows, max_pairs=2 * args.flows, device=args.device)
                t, out = timed(lambda: sp.rollup_from(src, flow_prefix=fpx))
                ms[n].append(t)
                info[n] = {"projected": out[1], "pairs": out[2], "flows": sp.counters()["flows"]}
                sp.close()
        res["spread"] = {n: dict(summary(ms[n]), **info[n]) for n in ms}
    if "cidr" in parts or "host" in parts:
        keys, st, en, pk, by = src.snapshot_arrays()
    if "cidr" in parts:
        pick = keys[:: max(1, len(keys) // 64)][:64]
        eq = [make_filter(src_ip=bytes(k[:16])) for k in pick]
        cidr = [as_cidr(f, 96 + (8, 16, 24, 21)[i % 4]) for i, f in enumerate(eq)]
        ms = {"equality x64": [], "cidr x64": []}
        flows = {}
        for _ in range(args.reps + 1):
            for n, batch in (("equality x64", eq), ("cidr x64", cidr)):
                t, out = timed(lambda: src.aggregate(batch))
                ms[n].append(t)
                flows[n] = sum(s.flows for s in out)
        res["cidr"] = {n: dict(summary(ms[n]), flows_matched=flows[n]) for n in ms}
    if "hhh" in parts:
        total = src.aggregate([{}])[0].packets
        thr = max(1, total // 1000)
        ms, out = [], None
        for _ in range(min(args.reps, 3) + 1):
            t, out = timed(lambda: src.hierarchical_heavy_hitters("SrcIP", [lv for _, lv in LEVELS], 0, thr))
            ms.append(t)
        res["hhh"] = dict(summary(ms), threshold=thr, reported=[len(lv) for lv in out])
    if "host" in parts:
        t0 = time.perf_counter()
        snap = src.snapshot_arrays()
        t1 = time.perf_counter()
        nets = mask_prefix(snap[0][:, :16], 24, 64)
        t2 = time.perf_counter()
        words = np.ascontiguousarray(nets).view(">u8")
        _, inv = np.unique(words, axis=0, return_inverse=True)
        sums = np.bincount(inv.ravel(), weights=snap[4].astype(np.float64))
        t3 = time.perf_counter()
        res["host"] = {"snapshot_ms": (t1 - t0) * 1e3, "mask_prefix_ms": (t2 - t1) * 1e3, "numpy_groupby_ms": (t3 - t2) * 1e3,
                       "total_ms": (t3 - t0) * 1e3, "groups": int(len(sums))}
    src.close()
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    args = parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--flows", str(args.flows), "--packets-per-flow",
           str(args.packets_per_flow), "--reps", str(args.reps), "--device", str(args.device), "--only", args.only]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s", file=sys.stderr)
        return 2
    if out.returncode != 0:
        print(f"exit {out.returncode}\n{out.stdout}\n{out.stderr}", file=sys.stderr)
        return 2
    res = json.loads(out.stdout.strip().splitlines()[-1])
    name = f"prefix_rollup_{args.flows}" + (f"_{args.tag}" if args.tag else "") + ".json"
    with open(os.path.join(args.out, name), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
