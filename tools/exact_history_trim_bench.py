#!/usr/bin/env python3
"""The life cycle of an exact history (gns_ex_hist_trim / _export / _append_rows, record with
``retain``) on one GPU, next to a copy floor, the existing pieces it is made of, and the host
route a user would otherwise run.

The setup is that of exact_history_bench.py: a handle filled with the synthetic stream
(SyntheticTraffic(flows=N, zipf_s=0.2), 12 packets per flow), one whole view plus nine deltas of
about --delta of the flows appended to a history.  Its log is exported once; every measurement
that consumes a history (a trim, a growth) starts from a fresh history restored from that log,
so each of the --reps timed calls after --warmup sees the same ten snapshots.  All in ONE child
process under a time limit (a child that fails or runs out of time ends the run: nothing more
is started on the GPU).

  trim       fold and drop at the 5th snapshot, fold down to one snapshot
  floor      a device-to-device copy of as many bytes as that trim reads plus writes
  pieces     existing code over the same rows: a log growth that copies as many rows as the
             trim keeps, and snapshot_arrays(end_time) at the trim point (the as-of compaction)
  export     export_log of the ten snapshots; restore = a fresh history plus one append_rows
             per snapshot
  host       the route without trim: export_log, a numpy latest-per-key filter of the expired
             rows, a fresh history, append_rows per snapshot (each phase timed once), the
             answers asserted equal to the trimmed history's
  record     ExactTask.record() of a delta interval with retain=4 against record() without it,
             two tasks fed the same stream

One JSON goes to profiles/exact_history_lifecycle_<flows>.json.

    python tools/exact_history_trim_bench.py [--flows 4194304] [--out profiles]
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
    ap.add_argument("--flows", type=int, default=1 << 22)
    ap.add_argument("--packets-per-flow", type=int, default=12)
    ap.add_argument("--delta", type=float, default=0.10, help="fraction of the flows a delta window touches")
    ap.add_argument("--deltas", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def timed(args, fn, setup=None):
    """(last result, {median, min, max} ms) of fn over --reps calls after --warmup; setup() runs
    untimed before each call and its result is fn's argument."""
    ms, out = [], None
    for i in range(args.warmup + args.reps):
        arg = setup() if setup else None
        out, t = once((lambda: fn(arg)) if setup else fn)
        if i >= args.warmup:
            ms.append(t)
        if hasattr(arg, "close"):
            arg.close()
    return out, spread(ms)


def child(args):
    import numpy as np
    import torch
    from go2netspectra_amd import ExactHistory, ExactTask, SyntheticTraffic, make_filter
    from go2netspectra_amd.checkpoint import history_slices
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host alone"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    target = args.flows
    tasks = [ExactTask("all", FIVE, max_flows=target, device=args.device),
             ExactTask("window", FIVE, max_flows=target, device=args.device)]
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
            for t in tasks:
                t.agg.insert_headers(hdr[:m], wl[:m], ts)
                t.agg.flush()
            done += m
            pos[0] += m

    syn = SyntheticTraffic(flows=target, zipf_s=0.2, device=args.device)
    insert(syn, target * args.packets_per_flow)
    hist = tasks[0].keep_history(max_rows=2 * target, max_flows=target)
    kept = tasks[1].keep_history(retain=4, max_rows=2 * target, max_flows=target)
    res = {"key_bytes": tasks[0].agg.key_bytes, "reps": args.reps, "warmup": args.warmup}

    # --- one whole view plus nine deltas, recorded with and without retention ---
    npk = int(-np.log(1.0 - args.delta) * target)  # uniform draws touching ~delta of the flows
    rec = {"all": [], "window": []}
    for i in range(args.deltas + 1):
        if i:
            insert(syn, npk)
        for t in tasks:
            out, ms = once(lambda: t.record(10 * i))
            rec[t.name()].append({"rows": out[0], "ms": ms})
    res["record"] = {"without_retain": spread([r["ms"] for r in rec["all"][1:]]),
                     "retain_4": spread([r["ms"] for r in rec["window"][1:]]),
                     "whole_view_without_retain_ms": rec["all"][0]["ms"], "whole_view_retain_4_ms": rec["window"][0]["ms"],
                     "delta_rows": [r["rows"] for r in rec["all"][1:]],
                     "stats_without_retain": hist.stats(), "stats_retain_4": kept.stats()}
    one = [make_filter()]
    a, b = kept.aggregate(one)[0], hist.aggregate(one)[0]
    assert (a.flows, a.packets, a.bytes) == (b.flows, b.packets, b.bytes) and len(kept.times()) == 4
    times = hist.times()
    c5 = 5
    t_fold = times[c5 - 1] + 1  # expires snapshots 0..4: the base is the 5th
    st = hist.stats()
    rows, slots = st["rows"], st["index_slots"]
    words = 1 + (res["key_bytes"] + 3) // 4  # {tag, key words} in a record of 4, 8 or 16 words
    rw = 4 * (4 if words <= 4 else 8 if words <= 8 else 16)
    row_bytes = rw + 32 + 8
    res["rows"], res["row_bytes"], res["index_slots"] = rows, row_bytes, slots

    # --- export and restore ---
    log, res["export_log"] = timed(args, hist.export_log)
    cuts = history_slices(log[5], len(log[6]))

    def fresh(max_rows=2 * target):
        h = ExactHistory(FIVE, max_rows=max_rows, max_flows=target, device=args.device)
        for t, (lo, hi) in zip(log[6].tolist(), cuts):
            h.append_rows(*[a[lo:hi] for a in log[:5]], t)
        return h
    h0, res["restore"] = timed(args, fresh)
    assert h0.aggregate(one) == hist.aggregate(one) and h0.stats()["keys"] == st["keys"]
    h0.close()

    # --- trims, each on a freshly restored history ---
    def copy_floor(nbytes):
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)

        def run():
            b.copy_(a)
            torch.cuda.synchronize(dev)
        return timed(args, run)[1]

    trims = {}
    for name, before, fold in (("fold_at_5th", t_fold, True), ("drop_at_5th", t_fold, False),
                               ("fold_to_one", times[-1] + 1, True)):
        out, ms = timed(args, lambda h: h.trim(before, fold=fold), setup=fresh)
        R = cuts[(c5 if name != "fold_to_one" else len(cuts)) - 1][1]  # rows of the expired snapshots
        moved = out["rows"]
        # flag reads (count and move) of the expired prefix, its rank words, the kept rows in and
        # out, the head words in and out and the mark list
        nbytes = (12 * R + 4 * R if fold else 0) + 2 * moved * row_bytes + 12 * slots
        trims[name] = dict(ms, out=out, prefix_rows=R, bytes_read_plus_written=nbytes, copy_floor=copy_floor(nbytes))
        trims[name]["ratio_to_floor"] = ms["median_ms"] / trims[name]["copy_floor"]["median_ms"]
    res["trim"] = trims

    # --- the existing pieces over the same rows ---
    # a log growth: a history whose log is exactly full (capacities are powers of two, so the
    # folded log is padded with rows of snapshot 0 under a later timestamp), then one more row
    ht = fresh()
    ht.trim(t_fold)
    tlog = ht.export_log()
    ht.close()
    moved = len(tlog[5])
    cap = 1
    while cap < moved:
        cap *= 2
    pad = cap - moved
    assert pad <= cuts[0][1], "the padding rows come from snapshot 0"
    tcuts = history_slices(tlog[5], len(tlog[6]))

    def full_log():
        h = ExactHistory(FIVE, max_rows=cap, max_flows=target, device=args.device)
        for t, (lo, hi) in zip(tlog[6].tolist(), tcuts):
            h.append_rows(*[a[lo:hi] for a in tlog[:5]], t)
        if pad:
            h.append_rows(*[a[:pad] for a in log[:5]], 1 << 39)
        assert h.stats()["rows"] == h.stats()["row_capacity"] == cap, h.stats()
        return h
    one_row = [a[-1:] for a in log[:5]]

    def grow_once(h):
        out = h.append_rows(*one_row, 1 << 40)
        assert h.stats()["row_capacity"] == 2 * cap
        return out
    _, grow = timed(args, grow_once, setup=full_log)
    h1 = fresh()
    ts_next = [1 << 40]

    def small_append():
        ts_next[0] += 1
        return h1.append_rows(*one_row, ts_next[0])
    _, nogrow = timed(args, small_append)
    h1.close()
    _, asof = timed(args, lambda: hist.snapshot_arrays(end_time=times[c5 - 1]))
    _, asof_count = timed(args, lambda: hist.aggregate(one, end_time=times[c5 - 1]))
    res["pieces"] = {"log_growth": grow, "log_growth_rows_copied": cap, "rows_kept_by_fold_at_5th": moved,
                     "append_one_row_without_growth": nogrow, "snapshot_arrays_at_trim_point": asof,
                     "aggregate_1_at_trim_point": asof_count}

    # --- the host route: export, filter on the host, a fresh history, append_rows per snapshot ---
    (k, s, e, p, b, w, ts), ms_export = once(hist.export_log)

    def host_filter():
        pre = int(cuts[c5 - 1][1])
        kv = np.ascontiguousarray(k[:pre][::-1]).view(np.dtype((np.void, k.shape[1]))).reshape(-1)
        _, first = np.unique(kv, return_index=True)  # the first from the end: the latest row of the key
        keep = np.sort(pre - 1 - first)
        idx = np.concatenate([keep, np.arange(pre, len(w))])
        wn = np.maximum(w[idx].astype(np.int64), c5 - 1) - (c5 - 1)
        return [a[idx] for a in (k, s, e, p, b)], wn, ts[c5 - 1:]
    (arrs, wn, tn), ms_filter = once(host_filter)

    def host_restore():
        h = ExactHistory(FIVE, max_rows=len(wn), max_flows=target, device=args.device)
        for t, (lo, hi) in zip(tn.tolist(), history_slices(wn, len(tn))):
            h.append_rows(*[a[lo:hi] for a in arrs], t)
        return h
    hh, ms_restore = once(host_restore)
    ht = fresh()
    ht.trim(t_fold)
    many = [make_filter(), make_filter(protocol=6), make_filter(protocol=17), make_filter(dst_port=443)]
    for T in (None, times[c5 - 1], times[c5], times[c5 - 1] - 1):
        assert hh.aggregate(many, end_time=T) == ht.aggregate(many, end_time=T), T
    assert all(np.array_equal(x, y) for x, y in zip(hh.export_log(), ht.export_log())), "host route and device trim differ"
    res["host_route"] = {"export_ms": ms_export, "numpy_filter_ms": ms_filter, "fresh_history_append_rows_ms": ms_restore,
                         "total_ms": ms_export + ms_filter + ms_restore,
                         "ratio_to_trim": (ms_export + ms_filter + ms_restore) / trims["fold_at_5th"]["median_ms"]}
    for h in (hh, ht, hist, kept):
        h.close()
    syn.close()
    for t in tasks:
        t.agg.close()
    return res


def main() -> int:
    args = parse_args()
    if args.child:
        print(json.dumps(child(args)), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--flows", str(args.flows), "--packets-per-flow",
           str(args.packets_per_flow), "--delta", str(args.delta), "--deltas", str(args.deltas), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--device", str(args.device)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"{args.flows} flows: no result within {args.timeout} s; stopping", file=sys.stderr)
        return 2
    if out.returncode != 0:
        print(f"{args.flows} flows: exit {out.returncode}; stopping\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}", file=sys.stderr)
        return 2
    res = dict({"flows_target": args.flows, "packets_filled": args.flows * args.packets_per_flow},
               **json.loads(out.stdout.strip().splitlines()[-1]))
    print(json.dumps(res), flush=True)
    with open(os.path.join(args.out, f"exact_history_lifecycle_{args.flows}.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
