#!/usr/bin/env python3
"""The exact engine's snapshot view against the export it stands beside, on one GPU.

For each table size (resident five-tuple flows; default 2^20 and 2^22) a handle is filled
with the synthetic stream (SyntheticTraffic(flows=N, zipf_s=0.2), 12 packets per flow, so
practically every flow is resident).  Three steps follow, each in a fresh child process
under its own time limit (a step that fails or runs out of time ends the run: nothing
more is started on the GPU):

  refresh   device time of view.refresh(0) (every flow) and of view.refresh(cursor) after
            one window of --window packets (Zipf --window-zipf over the same flows): the
            handle's "view" stage, HIP events on the ingest stream around the count, scan
            and write passes
  snapshot  host-visible time of view.snapshot_arrays() against ExactAggregator.
            snapshot_arrays() on the same table, the arrays asserted equal
  ingest    exact ingest rate over --windows windows: alone; with a reader thread taking
            one full view snapshot per window (refresh on the ingest thread at the window's
            end, export on the reader while the next window is inserted); and with a
            serial snapshot_arrays() after every window

One JSON per size goes to profiles/exact_view_<flows>.json.

    python tools/exact_view_bench.py [--flows 1048576 4194304] [--window 100000000] [--out profiles]
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
STEPS = ("refresh", "snapshot", "ingest")


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--flows", type=int, nargs="+", default=[1 << 20, 1 << 22])
    ap.add_argument("--packets-per-flow", type=int, default=12)
    ap.add_argument("--window", type=int, default=100_000_000)
    ap.add_argument("--window-zipf", type=float, default=1.1)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", choices=STEPS, help=argparse.SUPPRESS)
    return ap.parse_args()


def filled(args, target):
    """(torch, device, aggregator holding `target` flows)"""
    import torch
    from go2netspectra_amd import ExactAggregator, SyntheticTraffic
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    syn = SyntheticTraffic(flows=target, zipf_s=0.2, device=args.device)
    agg = ExactAggregator(FIVE, max_flows=target, device=args.device)
    total, win, done = target * args.packets_per_flow, 1 << 23, 0
    hdr = torch.empty((min(win, total), 64), dtype=torch.uint8, device=dev)
    wl = torch.empty((min(win, total),), dtype=torch.int32, device=dev)
    while done < total:
        m = min(win, total - done)
        syn.fill(hdr[:m], wl[:m], done)
        ts = torch.arange(done, done + m, dtype=torch.int64, device=dev) * 1000 + 1_700_000_000_000_000_000
        agg.insert_headers(hdr[:m], wl[:m], ts)
        agg.flush()
        done += m
    syn.close()
    return torch, dev, agg


class Windows:
    """Fresh windows of the ingest stream, generated outside the timed regions."""

    def __init__(self, args, torch, dev, target):
        from go2netspectra_amd import SyntheticTraffic
        self.torch, self.n, self.k = torch, args.window, 0
        self.syn = SyntheticTraffic(flows=target, zipf_s=args.window_zipf, device=args.device)
        self.hdr = torch.empty((self.n, 64), dtype=torch.uint8, device=dev)
        self.wl = torch.empty((self.n,), dtype=torch.int32, device=dev)
        self.ts = torch.empty((self.n,), dtype=torch.int64, device=dev)

    def next(self):
        k, n = self.k, self.n
        self.k += 1
        self.syn.fill(self.hdr, self.wl, first=k * n)
        self.torch.arange(k * n, (k + 1) * n, dtype=self.torch.int64, device=self.hdr.device, out=self.ts)
        self.ts.mul_(100).add_(1_800_000_000_000_000_000)
        self.torch.cuda.synchronize()
        return self.hdr, self.wl, self.ts


def step_refresh(args, target):
    from go2netspectra_amd import make_filter
    torch, dev, agg = filled(args, target)
    view = agg.view()
    agg.set_timing(True, stages=["view"])

    def timed(since):
        for _ in range(args.warmup):
            view.refresh(since)
        agg.flush()
        agg.stage_times(reset=True)
        for _ in range(args.reps):
            cur = view.refresh(since)
        agg.flush()
        ms, launches = agg.stage_times(reset=True)["view"]
        assert launches == args.reps
        return ms / args.reps, view.aggregate([make_filter()])[0].flows, cur

    st = agg.dict_stats()
    res = {"slots": st["slots"], "key_bytes": agg.key_bytes, "reps": args.reps, "warmup": args.warmup}
    res["refresh_full_device_ms"], res["rows_full"], cursor = timed(0)
    w = Windows(args, torch, dev, target)
    hdr, wl, ts = w.next()
    agg.insert_headers(hdr, wl, ts)
    agg.flush()
    res["refresh_delta_device_ms"], res["rows_delta"], cur2 = timed(cursor)
    assert cur2 == cursor + args.window
    res["window_packets"], res["window_zipf_s"] = args.window, args.window_zipf
    res["rows_after_window"] = agg.aggregate([make_filter()])[0].flows
    view.close()
    agg.close()
    return res


def step_snapshot(args, target):
    import numpy as np
    torch, dev, agg = filled(args, target)
    view = agg.view()
    view.refresh()
    agg.flush()

    def wall(fn, reps=3):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        return out, (time.perf_counter() - t0) / reps * 1e3

    got, view_ms = wall(view.snapshot_arrays)
    want, snap_ms = wall(agg.snapshot_arrays)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b), "view rows differ from snapshot_arrays()"
    res = {"flows_resident": int(len(want[3])), "view_snapshot_wall_ms": view_ms, "snapshot_arrays_wall_ms": snap_ms,
           "snapshot_speedup_wall": snap_ms / view_ms}
    view.close()
    agg.close()
    return res


def step_ingest(args, target):
    import queue
    import threading
    torch, dev, agg = filled(args, target)
    w = Windows(args, torch, dev, target)
    view = agg.view()

    def run(after_insert):
        elapsed = 0.0
        for _ in range(args.windows):
            hdr, wl, ts = w.next()
            t0 = time.perf_counter()
            agg.insert_headers(hdr, wl, ts)
            after_insert()
            agg.flush()
            elapsed += time.perf_counter() - t0
        return args.window * args.windows / elapsed / 1e6

    for _ in range(2):  # warm-up windows
        hdr, wl, ts = w.next()
        agg.insert_headers(hdr, wl, ts)
        agg.flush()
    res = {"window_packets": args.window, "windows": args.windows, "window_zipf_s": args.window_zipf}
    res["ingest_alone_Mpps"] = run(lambda: None)
    res["window_ms_alone"] = args.window / res["ingest_alone_Mpps"] / 1e3

    todo, rows, errors = queue.Queue(), [], []

    def reader():
        try:
            while todo.get():
                t0 = time.perf_counter()
                n = len(view.snapshot_arrays()[3])
                rows.append((n, (time.perf_counter() - t0) * 1e3))
        except Exception as e:  # reported by the main thread
            errors.append(e)

    th = threading.Thread(target=reader)
    th.start()

    def hand_over():
        view.refresh()  # waits for the reader's export of the previous window, if it still runs
        todo.put(True)

    try:
        res["ingest_with_view_reader_Mpps"] = run(hand_over)
    finally:
        todo.put(False)
        th.join()
    assert not errors and len(rows) == args.windows, (errors, rows)
    res["reader_rows"] = [r[0] for r in rows]
    res["reader_snapshot_wall_ms"] = [round(r[1], 3) for r in rows]
    res["ingest_with_serial_snapshot_Mpps"] = run(lambda: agg.snapshot_arrays())
    res["view_reader_vs_alone"] = res["ingest_with_view_reader_Mpps"] / res["ingest_alone_Mpps"]
    res["serial_snapshot_vs_alone"] = res["ingest_with_serial_snapshot_Mpps"] / res["ingest_alone_Mpps"]
    view.close()
    agg.close()
    return res


def main() -> int:
    args = parse_args()
    if args.child:
        res = {"refresh": step_refresh, "snapshot": step_snapshot, "ingest": step_ingest}[args.child](args, args.flows[0])
        print(json.dumps(res), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    for target in args.flows:
        res = {"flows_target": target, "packets_filled": target * args.packets_per_flow}
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--flows", str(target),
                   "--packets-per-flow", str(args.packets_per_flow), "--window", str(args.window),
                   "--window-zipf", str(args.window_zipf), "--windows", str(args.windows), "--reps", str(args.reps),
                   "--warmup", str(args.warmup), "--device", str(args.device)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"{target} flows, step {step}: no result within {args.step_timeout} s; stopping", file=sys.stderr)
                return 2
            if out.returncode != 0:
                print(f"{target} flows, step {step}: exit {out.returncode}; stopping\n{out.stdout}\n{out.stderr}",
                      file=sys.stderr)
                return 2
            res[step] = json.loads(out.stdout.strip().splitlines()[-1])
            print(f"{target} {step}: {json.dumps(res[step])}", flush=True)
        with open(os.path.join(args.out, f"exact_view_{target}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
