#!/usr/bin/env python3
"""What the exact spread engine's pair set interface costs, beside the only other route.

On the configs[2] stream of tools/spread_accuracy.py (SyntheticTraffic(fanout=2^20), flow
SrcIP, element DstIP; default 100M packets in 25M-packet windows, tables sized for the
stream) it times, wall clock around the call with the device idle before and after:

  export_device   gns_pairs_export of the whole set into device memory (count call included)
  export_host     the same into host memory (staged in pieces of 2^20 table slots)
  d2h             the exported bytes copied device -> host once by torch (pageable memory, as
                  the export's destination): what the bus and the host's paging cost alone
  delta_device    the export since the cursor above, after one further window
  merge_from      gns_pairs_merge_from between two handles that each ingested half the stream
  reingest        what there was before the union: the second half's packets inserted again
                  from device memory (insert_headers + flush) into a handle holding the first

The exports are repeated (--reps) and every time is listed; the merge and the re-ingest
change the state and run once.  Beside each time stand the bytes the call moves at least:
one read of the pair table plus the rows written.  The merged handle's snapshot is compared
with the snapshot of a handle fed the whole stream, and the export counts with the engine's
counters.  One JSON goes to profiles/exs_pairs_<geometry>.json.

    python tools/pairs_bench.py [--packets 100000000] [--window 25000000]
                                [--max-pairs 67108864 --max-flows 2097152 --batch 25000000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SS_FANOUT = 1 << 20


def main() -> int:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packets", type=int, default=100_000_000)
    ap.add_argument("--window", type=int, default=25_000_000)
    ap.add_argument("--max-pairs", type=int, default=1 << 26, help="initial pair capacity (0 = the engine's default: grown)")
    ap.add_argument("--max-flows", type=int, default=1 << 21)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(root, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from go2netspectra_amd import ExactSpread, SyntheticTraffic

    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    os.makedirs(args.out, exist_ok=True)
    win = min(args.window, args.packets)
    nwin = args.packets // win
    assert nwin >= 2 and nwin % 2 == 0 and nwin * win == args.packets, "an even number of whole windows"
    syn = SyntheticTraffic(device=args.device, fanout=SS_FANOUT)
    hdr = torch.empty((win, 64), dtype=torch.uint8, device=dev)
    wl = torch.empty((win,), dtype=torch.int32, device=dev)

    def handle():
        return ExactSpread(["SrcIP"], ["DstIP"], max_flows=args.max_flows, max_pairs=args.max_pairs,
                           batch_packets=args.batch, device=args.device)

    def feed(handles, w):
        """Window w into each handle; returns the seconds of insert + flush per handle."""
        syn.fill(hdr, wl, first=w * win)
        torch.cuda.synchronize(dev)
        spent = []
        for h in handles:
            t0 = time.perf_counter()
            h.insert_headers(hdr, wl)
            h.flush()
            spent.append(time.perf_counter() - t0)
        return spent

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return out, (time.perf_counter() - t0) * 1e3

    def ordered(h):
        f, v = h.snapshot_arrays()
        o = np.argsort(np.ascontiguousarray(f).view(np.dtype((np.void, f.shape[1]))).ravel())
        return f[o], v[o]

    whole, first, second, replay = handle(), handle(), handle(), handle()
    ingest_s = 0.0
    for w in range(nwin):
        half = [first, replay] if w < nwin // 2 else [second]
        ingest_s += feed([whole] + half, w)[0]
    km = whole.flow_bytes + whole.elem_bytes
    ds = whole.dict_stats()
    table_bytes = ds["pair_slots"] * (64 if km <= 60 else 128)
    res = {"tool": "pairs_bench", "packets": args.packets, "window": win,
           "stream": "configs[2]: SyntheticTraffic(fanout=2^20), flow SrcIP, element DstIP",
           "capacity": {"max_pairs": args.max_pairs, "max_flows": args.max_flows, "batch": args.batch},
           "pairs": ds["pairs_claimed"], "flows": ds["flows_claimed"], "pair_slots": ds["pair_slots"],
           "pair_growths": ds["pair_growths"], "pair_table_bytes": table_bytes, "row_bytes": km,
           "ingest_ms": ingest_s * 1e3}

    # full exports
    times = {"export_device": [], "export_host": [], "d2h": [], "delta_device": []}
    cur = 0
    for _ in range(args.reps):
        (f, e, cur), ms = wall(lambda: whole.export_pairs(device=True))
        times["export_device"].append(ms)
        assert len(f) == ds["pairs_claimed"]
        del f, e
    for _ in range(args.reps):
        (f, e, _), ms = wall(lambda: whole.export_pairs())
        times["export_host"].append(ms)
        assert len(f) == ds["pairs_claimed"]
        del f, e
    rows = torch.empty((ds["pairs_claimed"], km), dtype=torch.uint8, device=dev)
    for _ in range(args.reps):
        host, ms = wall(lambda: rows.cpu())
        times["d2h"].append(ms)
        del host
    del rows
    res["export_bytes"] = table_bytes + ds["pairs_claimed"] * km
    want = ordered(whole)

    # union of the halves against the re-ingest of the second half
    empty = ExactSpread(["SrcIP"], ["DstIP"], max_flows=64, max_pairs=256, device=args.device)
    first.merge_from(empty)  # the staging buffer is allocated outside the timed call
    before = first.counters()
    first.set_timing(True, stages=["resolve"])
    first.stage_times(reset=True)
    _, res["merge_from_ms"] = wall(lambda: first.merge_from(second))
    res["merge_resolve_ms"], res["merge_resolve_rounds"] = first.stage_times()["resolve"]
    first.set_timing(False)
    res["merge_pieces"] = -(-second.dict_stats()["pair_slots"] // min(1 << 20, args.batch or (4 << 20)))
    after = first.counters()
    res["merge_pairs_read"] = second.dict_stats()["pairs_claimed"]
    res["merge_pairs_added"] = after["new_pairs"] - before["new_pairs"]
    res["merge_growths"] = first.dict_stats()["pair_growths"]
    res["merge_bytes_source"] = second.dict_stats()["pair_slots"] * (64 if km <= 60 else 128)
    assert after["inserted"] == before["inserted"] and after["batches"] == before["batches"]
    got = ordered(first)
    res["merged_equals_whole"] = bool(all(np.array_equal(a, b) for a, b in zip(got, want)))
    reingest_s = 0.0
    for w in range(nwin // 2, nwin):
        reingest_s += feed([replay], w)[0]
    res["reingest_ms"] = reingest_s * 1e3
    res["reingest_packets"] = args.packets // 2
    got = ordered(replay)
    res["reingest_equals_whole"] = bool(all(np.array_equal(a, b) for a, b in zip(got, want)))
    res["merge_over_reingest"] = res["merge_from_ms"] / res["reingest_ms"]
    del got, want

    # the delta after one further window
    pairs0 = whole.counters()["new_pairs"]
    feed([whole], nwin)
    new = whole.counters()["new_pairs"] - pairs0
    for _ in range(args.reps):
        (f, e, _), ms = wall(lambda: whole.export_pairs(since=cur, device=True))
        times["delta_device"].append(ms)
        assert len(f) == new, (len(f), new)
        del f, e
    ds2 = whole.dict_stats()
    res["delta_pairs"] = new
    res["delta_bytes"] = ds2["pair_slots"] * (64 if km <= 60 else 128) + new * km
    for k, v in times.items():
        res[k + "_ms"] = [round(x, 3) for x in v]
        res[k + "_best_ms"] = round(min(v), 3)
    res["export_device_gb_s"] = round(res["export_bytes"] / res["export_device_best_ms"] / 1e6, 1)
    res["snapshot_check"] = "green" if res["merged_equals_whole"] and res["reingest_equals_whole"] else "RED"
    line = json.dumps(res)
    print(line, flush=True)
    geometry = f"mp{args.max_pairs}_b{args.batch}_{args.packets}"
    with open(os.path.join(args.out, f"exs_pairs_{geometry}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["snapshot_check"] == "green" else 1


if __name__ == "__main__":
    sys.exit(main())
