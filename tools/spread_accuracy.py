#!/usr/bin/env python3
"""SuperSpread's accuracy on the stream the benchmark runs, against the exact
spread engine, and the exact engine's own insert rate.

The configs[2] stream (SyntheticTraffic(fanout=2^20), flow SrcIP, element DstIP,
the default SuperSpread task geometry d=2 w=32768 m=128 threshold 4096) is
generated on the device window by window; every window goes to a SuperSpread
and to an ExactSpread.  Prints one JSON line: accuracy.spread_report (the
ss_test.go:86-136 protocol), the ExactSpread insert rate (timed around
insert_headers + flush + device sync with the handle's stage times on) next to
SuperSpread's on the same windows, and the per-stage milliseconds.

    python tools/spread_accuracy.py 100000000 [--window 25000000] [--batch 0] [--max-pairs N --max-flows N]

With the default capacities the timed region includes every table growth from 4M
pairs up (device allocations and rehashes, host-synchronous); --max-pairs /
--max-flows large enough for the stream time the steady state instead.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SS_W, SS_D, SS_M, SS_THR, SS_FANOUT = 32768, 2, 128, 4096, 1 << 20
SS_HLL, SS_RNG = 0x0123456789ABCDEF, 0x0DDBA11CAFEF00D5


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("packets", type=int)
    ap.add_argument("--window", type=int, default=25_000_000, help="packets generated and fed per step")
    ap.add_argument("--batch", type=int, default=0, help="ExactSpread device batch (0 = its default)")
    ap.add_argument("--max-pairs", type=int, default=0, help="ExactSpread initial pair capacity (0 = its default)")
    ap.add_argument("--max-flows", type=int, default=0, help="ExactSpread initial flow capacity (0 = its default)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch
    from go2netspectra_amd import ExactSpread, SuperSpread, SyntheticTraffic
    from go2netspectra_amd.accuracy import spread_report

    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    syn = SyntheticTraffic(device=args.device, fanout=SS_FANOUT)
    ss = SuperSpread(SS_W, SS_D, SS_THR, SS_M, 5, 0.5, 1.08, flow_fields=["SrcIP"], elem_fields=["DstIP"],
                     hll_master=SS_HLL, rng_seed=SS_RNG, device=args.device)
    ex = ExactSpread(["SrcIP"], ["DstIP"], max_flows=args.max_flows, max_pairs=args.max_pairs,
                     batch_packets=args.batch, device=args.device)
    ex.set_timing(True)
    win = min(args.window, args.packets)
    hdr = torch.empty((win, 64), dtype=torch.uint8, device=dev)
    wl = torch.empty((win,), dtype=torch.int32, device=dev)
    t_ex = t_ss = 0.0
    done = 0
    while done < args.packets:
        m = min(win, args.packets - done)
        h, w = hdr[:m], wl[:m]
        syn.fill(h, w, first=done)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ex.insert_headers(h, w)
        ex.flush()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        ss.insert_headers(h, w)
        ss.flush()
        torch.cuda.synchronize(dev)
        t_ex += t1 - t0
        t_ss += time.perf_counter() - t1
        done += m
    st = ex.stage_times()
    stages = {k: round(v[0], 3) for k, v in st.items() if not k.startswith("unused")}
    dev_ms = st["total"][0]  # the batches' own stages on the device (HIP events), growth excluded
    rep = spread_report(ss, ex, SS_THR)
    ce, ds = ex.counters(), ex.dict_stats()
    out = {"tool": "spread_accuracy", "packets": args.packets, "window": win,
           "stream": "configs[2]: SyntheticTraffic(fanout=2^20), flow SrcIP, element DstIP",
           "sketch": {"width": SS_W, "depth": SS_D, "m": SS_M, "threshold": SS_THR},
           "report": rep,
           "exact_gpkt_s": round(done / t_ex / 1e9, 4), "superspread_gpkt_s": round(done / t_ss / 1e9, 4),
           "exact_device_gpkt_s": round(done / dev_ms / 1e6, 4) if dev_ms > 0 else None,
           "exact_capacity": {"max_pairs": args.max_pairs, "max_flows": args.max_flows, "batch": args.batch},
           "exact_stage_ms": stages, "exact_batches": ce["batches"], "distinct_pairs": ce["new_pairs"],
           "flows": ce["flows"], "dict_stats": ds}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
