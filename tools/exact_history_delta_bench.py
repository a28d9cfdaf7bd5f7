#!/usr/bin/env python3
"""The history delta (gns_ex_hist_rollup_between, gns_ex_movers) against the routes that exist
without it, on one GPU.

The workload is tools/exact_history_rollup_bench.py's: a handle filled with the synthetic stream
(SyntheticTraffic(flows=N, zipf_s=0.2), 12 packets per flow; default N = 2^22 five-tuple flows),
one whole view and nine delta views of about --delta of the flows appended to a history: ten
snapshots.  Then, in ONE child process under a time limit (a child that fails or runs out of
time ends the run: nothing more is started on the GPU), for the windows

  last       between the two newest snapshots
  middle     from the middle snapshot to the newest
  no_start   a NULL start: the table as of the newest snapshot through the window kernels

and the layouts SrcIP, SrcIP at /24 and the same five-tuple layout:

  between       wall time of gns_ex_hist_rollup_between into an empty handle, with its per-stage
                device times (gns_ex_stage_times) from one more call
  rollup_t1     (a) gns_ex_hist_rollup as of T1 alone
  two_rollups   (b) the device route without the new call: gns_ex_hist_rollup as of T0 and as
                of T1 into two handles (the subtraction is not even counted)
  host_route    (c) per window, at the same layout: snapshot_arrays(T0), snapshot_arrays(T1), a
                numpy join by key, the subtraction, ExactAggregator.merge; --host-reps calls
  movers        gns_ex_movers with limit 10 and 1000 on the finished SrcIP table of the window,
                and gns_ex_heavy_hitters with the same limits on the same table

Every destination is created outside the timed region with room for the rows it receives.  The
changed flows / packets / bytes of `between` are asserted equal to the difference of the two
tables' totals.  Times are medians over --reps calls after --warmup, with the smallest and the
largest.  One JSON per size goes to profiles/exact_history_delta_<flows>.json.

    python tools/exact_history_delta_bench.py [--flows 4194304] [--out profiles]
"""
import argparse
import ctypes as ct
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
CASES = [("SrcIP", ["SrcIP"], None), ("SrcIP_24", ["SrcIP"], {"SrcIP": (24, 64)}), ("same_layout", FIVE, None)]


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--flows", type=int, nargs="+", default=[1 << 22])
    ap.add_argument("--packets-per-flow", type=int, default=12)
    ap.add_argument("--delta", type=float, default=0.10, help="fraction of the flows a delta window touches")
    ap.add_argument("--deltas", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=5, help="timed calls of the host route (seconds each at 2^22 flows)")
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "calls": len(ms)}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def host_delta(np, a, b):
    """table(b) - table(a) joined by key on the host: rows of the changed and new flows."""
    K = a[0].shape[1]
    keys = np.concatenate([b[0], a[0]])
    nb = len(b[0])
    void = np.ascontiguousarray(keys).view(np.dtype((np.void, K))).reshape(-1)
    order = np.argsort(void, kind="stable")  # b's row of a key before a's
    sv = void[order]
    first = np.ones(len(sv), bool)
    first[1:] = sv[1:] != sv[:-1]
    starts = np.nonzero(first)[0]
    sign = np.where(order < nb, 1, -1).astype(np.int64)
    pk = np.concatenate([b[3], a[3]]).view(np.int64)[order] * sign
    by = np.concatenate([b[4], a[4]]).view(np.int64)[order] * sign
    dpk, dby = np.add.reduceat(pk, starts), np.add.reduceat(by, starts)
    lead = order[starts]  # the key's row in b when it has one
    keep = (dpk != 0) & (lead < nb)
    lead = lead[keep]
    return (b[0][lead], b[1][lead], b[2][lead], dpk[keep].view(np.uint64), dby[keep].view(np.uint64))


def child(args, target):
    import numpy as np
    import torch
    from go2netspectra_amd import ExactAggregator, ExactHistory, SyntheticTraffic, _lib, make_filter, make_prefix, signed
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host alone"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    L = _lib.load()
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
    rows = hist.stats()["rows"]
    res = {"reps": args.reps, "warmup": args.warmup, "host_reps": args.host_reps, "stats": hist.stats(), "cases": {}, "host_route": {}}
    windows = [("last", times[-2], None), ("middle", times[len(times) // 2], None), ("no_start", None, None)]
    every = make_filter()
    total = lambda a: (lambda s: (s.flows, s.packets, s.bytes))(a.aggregate([every])[0])
    i64 = lambda t: None if t is None else ct.byref(ct.c_int64(t))

    def between(dst, T0, T1, prefix):
        out = (ct.c_uint64 * 2)()
        px = make_prefix(prefix) if prefix is not None else None
        _lib.check(L.gns_ex_hist_rollup_between(dst._h, hist._h, i64(T0), i64(T1), ct.byref(px) if px is not None else None, out))
        return int(out[0]), int(out[1])

    def staged(fn, fields, room):
        dst = ExactAggregator(fields, max_flows=room, device=args.device)
        dst.set_timing(True)
        fn(dst)
        st = {k: {"ms": v[0], "launches": v[1]} for k, v in dst.stage_times().items() if v[1]}
        dst.close()
        return st

    for wname, T0, T1 in windows:
        live1 = hist.aggregate([every], end_time=T1)[0]
        live0 = hist.aggregate([every], end_time=T0)[0] if T0 is not None else None
        for cname, fields, prefix in CASES:
            btw, one, two, selected, groups = [], [], [], None, None
            for rep in range(args.warmup + args.reps):
                dst = ExactAggregator(fields, max_flows=live1.flows, device=args.device)
                out, ms = clock(lambda: between(dst, T0, T1, prefix))
                selected = out[0]
                if cname == "same_layout":  # the changed rows are the difference of the two tables
                    s = dst.aggregate([every])[0]
                    p0, b0 = (live0.packets, live0.bytes) if live0 else (0, 0)
                    assert (signed(s.packets), signed(s.bytes)) == (live1.packets - p0, live1.bytes - b0), (wname, s)
                groups = total(dst)[0]
                if cname == "SrcIP" and rep == args.warmup + args.reps - 1:
                    mv = {}
                    for limit in (10, 1000):
                        m_ms, h_ms = [], []
                        for r2 in range(args.warmup + args.reps):
                            got, a_ms = clock(lambda: dst.movers(1, 0, 1, limit))
                            _, b_ms = clock(lambda: dst.heavy_hitters(1, 1, limit))
                            assert len(got[1]) == min(limit, groups), (limit, len(got[1]), groups)
                            if r2 >= args.warmup:
                                m_ms.append(a_ms); h_ms.append(b_ms)
                        mv[f"limit_{limit}"] = {"movers": stats(m_ms), "heavy_hitters": stats(h_ms)}
                    res["cases"].setdefault(f"movers@{wname}", {"groups": groups, **mv})
                dst.close()
                dst = ExactAggregator(fields, max_flows=live1.flows, device=args.device)
                o1, a_ms = clock(lambda: dst.rollup_from_history(hist, end_time=T1, prefix=prefix))
                if T0 is None:
                    assert o1[0] == selected, (o1, selected)
                dst.close()
                b_ms = None
                if T0 is not None:
                    d0 = ExactAggregator(fields, max_flows=live1.flows, device=args.device)
                    d1 = ExactAggregator(fields, max_flows=live1.flows, device=args.device)
                    _, b_ms = clock(lambda: (d0.rollup_from_history(hist, end_time=T0, prefix=prefix),
                                             d1.rollup_from_history(hist, end_time=T1, prefix=prefix)))
                    d0.close()
                    d1.close()
                if rep >= args.warmup:
                    btw.append(ms); one.append(a_ms)
                    if b_ms is not None:
                        two.append(b_ms)
            case = {"log_rows": rows, "rows_selected": selected, "groups": groups, "between": stats(btw), "rollup_t1": stats(one),
                    "between_stages": staged(lambda d: between(d, T0, T1, prefix), fields, live1.flows),
                    "rollup_t1_stages": staged(lambda d: d.rollup_from_history(hist, end_time=T1, prefix=prefix), fields, live1.flows)}
            if two:
                case["two_rollups"] = stats(two)
            res["cases"][f"{cname}@{wname}"] = case
        if T0 is not None and args.host_reps:
            tot, parts = [], []
            for rep in range(1 + args.host_reps if args.host_reps > 1 else 1):
                a, e0 = clock(lambda: hist.snapshot_arrays(end_time=T0))
                b, e1 = clock(lambda: hist.snapshot_arrays(end_time=T1))
                d, j = clock(lambda: host_delta(np, a, b))
                tmp = ExactAggregator(FIVE, max_flows=max(len(d[3]), 64), device=args.device)
                _, m = clock(lambda: tmp.merge(*d))
                s = tmp.aggregate([every])[0]
                assert (signed(s.packets), signed(s.bytes)) == (live1.packets - live0.packets, live1.bytes - live0.bytes)
                tmp.close()
                del a, b, d
                if rep >= 1 or args.host_reps == 1:
                    tot.append(e0 + e1 + j + m); parts.append((e0 + e1, j, m))
            res["host_route"][wname] = {"total": stats(tot), "export_ms": sorted(p[0] for p in parts), "join_ms": sorted(p[1] for p in parts),
                                        "merge_ms": sorted(p[2] for p in parts)}
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
               "--warmup", str(args.warmup), "--host-reps", str(args.host_reps), "--device", str(args.device)]
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
        with open(os.path.join(args.out, f"exact_history_delta_{target}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
