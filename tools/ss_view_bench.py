#!/usr/bin/env python3
"""SuperSpread's snapshot view against the handle calls it stands beside, on one GPU.

For each geometry (configs[2]'s d=2 w=32768, and the default d=3 w=2^20; m=128, size 5,
flow SrcIP, element DstIP) a handle ingests bench.py's configs[2] stream
(SyntheticTraffic(fanout=2^20)) in device-resident windows of --window packets.  Three
steps follow, each in a fresh child process under its own time limit (a step that fails
or runs out of time ends the run: nothing more is started on the GPU):

  refresh  device time of view.refresh() and view.refresh(state=True): the handle's
           "view" stage (HIP events on the ingest stream around the snapshot kernel and,
           with state, the three device copies)
  calls    host-visible time of view.heavy_hitters_arrays() against the handle's
           heavy_hitters_arrays(), and of view.export_state() against the handle's
           export_state(), on the same state in the same run, the results asserted equal
  ingest   ingest rate over --windows windows in periods of --period windows: alone; with a
           reader thread listing once per period (refresh on the ingest thread at the
           period's end, the list on the reader while the next period is inserted); with a
           reader thread exporting the whole state once per period; and with the serial
           handle calls on the ingest thread (heavy_hitters_arrays(), export_state()) at
           every period's end.  The cases run --rounds times, alternating; medians are
           reported beside every round's value and the spread of "alone"

One JSON per geometry goes to profiles/ss_view_<cells>.json.

    python tools/ss_view_bench.py [--geometry 2x32768 3x1048576] [--window 100000000] [--out profiles]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("refresh", "calls", "ingest")
SS_M, SS_THR, SS_FANOUT = 128, 4096, 1 << 20
SS_HLL, SS_RNG = 0x0123456789ABCDEF, 0x0DDBA11CAFEF00D5


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--geometry", nargs="+", default=["2x32768", "3x1048576"], help="depth x width")
    ap.add_argument("--window", type=int, default=100_000_000)
    ap.add_argument("--windows", type=int, default=96, help="windows per ingest case")
    ap.add_argument("--period", type=int, default=16, help="windows per snapshot period (one hand-over each)")
    ap.add_argument("--rounds", type=int, default=3, help="times the ingest cases are run, alternating")
    ap.add_argument("--warm-windows", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", choices=STEPS, help=argparse.SUPPRESS)
    return ap.parse_args()


def row_seeds(d):  # bench.py's
    import numpy as np
    s, out = 0x9747B28C, []
    for _ in range(d):
        s = (s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        out.append((z ^ (z >> 31)) & 0xFFFFFFFF)
    return np.array(out, np.uint32)


class Stream:
    """Fresh windows of the configs[2] stream, generated outside the timed regions."""

    def __init__(self, args, torch, dev):
        from go2netspectra_amd import SyntheticTraffic
        self.torch, self.n, self.k = torch, args.window, 0
        self.syn = SyntheticTraffic(device=args.device, fanout=SS_FANOUT)
        self.hdr = torch.empty((self.n, 64), dtype=torch.uint8, device=dev)
        self.wl = torch.empty((self.n,), dtype=torch.int32, device=dev)

    def next(self):
        self.syn.fill(self.hdr, self.wl, first=self.k * self.n)
        self.k += 1
        self.torch.cuda.synchronize()
        return self.hdr, self.wl


def warmed(args, geometry):
    """(torch, handle after --warm-windows windows, the stream)"""
    import torch
    from go2netspectra_amd import SuperSpread
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    d, w = (int(x) for x in geometry.split("x"))
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    ss = SuperSpread(w, d, SS_THR, SS_M, 5, 0.5, 1.08, flow_fields=["SrcIP"], elem_fields=["DstIP"],
                     seeds=row_seeds(d), hll_master=SS_HLL, rng_seed=SS_RNG, batch_packets=args.window,
                     device=args.device)
    st = Stream(args, torch, dev)
    for _ in range(args.warm_windows):
        ss.insert_headers(*st.next())
        ss.flush()
    return torch, ss, st


def step_refresh(args, geometry):
    torch, ss, st = warmed(args, geometry)
    view = ss.view()
    ss.set_timing(True, stages=["view"])
    res = {"reps": args.reps, "warmup": args.warmup}
    for name, state in (("refresh_device_ms", False), ("refresh_state_device_ms", True)):
        for _ in range(args.warmup):
            view.refresh(state=state)
        ss.flush()
        ss.stage_times(reset=True)
        for _ in range(args.reps):
            view.refresh(state=state)
        ss.flush()
        ms, launches = ss.stage_times(reset=True)["view"]
        assert launches == args.reps
        res[name] = ms / args.reps
    cells, kw = ss.depth * ss.width, (ss.flow_bytes + 3) // 4
    res["view_bytes"] = cells * (4 + 4 * kw)
    res["view_state_bytes"] = cells * (ss.m + 8)
    view.close()
    ss.close()
    return res


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return out, (time.perf_counter() - t0) / reps * 1e3


def step_calls(args, geometry):
    import numpy as np
    torch, ss, st = warmed(args, geometry)
    view = ss.view()
    view.refresh(state=True)
    ss.flush()
    res = {"reps": args.reps}
    got, res["view_heavy_hitters_wall_ms"] = wall(view.heavy_hitters_arrays, args.reps)
    want, res["handle_heavy_hitters_wall_ms"] = wall(ss.heavy_hitters_arrays, args.reps)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), "view list differs from the handle's"
    res["heavy_hitters"] = int(len(want[1]))
    got, res["view_export_state_wall_ms"] = wall(view.export_state, 3)
    want, res["handle_export_state_wall_ms"] = wall(ss.export_state, 3)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), "view state differs"
    res["export_state_bytes"] = int(sum(a.nbytes for a in want))
    view.close()
    ss.close()
    return res


def step_ingest(args, geometry):
    import queue
    import statistics
    import threading
    torch, ss, st = warmed(args, geometry)
    view = ss.view()

    def run(at_period_end):
        """--windows windows, a hand-over (or a serial call) after every --period of them; the
        ingest thread's time in insert, hand-over and flush over the packets (window generation
        is outside the sum; a reader thread keeps running through it)."""
        elapsed = 0.0
        for k in range(args.windows):
            hdr, wl = st.next()
            t0 = time.perf_counter()
            ss.insert_headers(hdr, wl)
            if (k + 1) % args.period == 0:
                at_period_end()
            ss.flush()
            elapsed += time.perf_counter() - t0
        return args.window * args.windows / elapsed / 1e9

    def with_reader(state, read, walls):
        todo, errors = queue.Queue(), []

        def reader():
            try:
                while todo.get():
                    t0 = time.perf_counter()
                    read()
                    walls.append(round((time.perf_counter() - t0) * 1e3, 3))
            except Exception as e:  # reported by the main thread
                errors.append(e)

        th = threading.Thread(target=reader)
        th.start()

        def hand_over():
            view.refresh(state=state)  # waits for the reader's call of the previous period, if it still runs
            todo.put(True)

        try:
            rate = run(hand_over)
        finally:
            todo.put(False)
            th.join()
        assert not errors, errors
        return rate

    view.refresh(state=True)  # warm both kinds of refresh and the readers' buffers
    view.heavy_hitters_arrays()
    view.export_state()
    ss.heavy_hitters_arrays()
    list_ms, export_ms = [], []
    cases = {
        "alone": lambda: run(lambda: None),
        "reader_list": lambda: with_reader(False, view.heavy_hitters_arrays, list_ms),
        "reader_export": lambda: with_reader(True, view.export_state, export_ms),
        "serial_list": lambda: run(ss.heavy_hitters_arrays),
        "serial_export": lambda: run(ss.export_state),
    }
    rates = {k: [] for k in cases}
    for _ in range(args.rounds):  # the cases alternate, so clock and neighbour drift hit all of them
        for k, fn in cases.items():
            rates[k].append(fn())
    res = {"window_packets": args.window, "windows": args.windows, "windows_per_period": args.period,
           "rounds": args.rounds, "reader_list_wall_ms": list_ms, "reader_export_wall_ms": export_ms}
    for k, v in rates.items():
        res[f"ingest_{k}_Gpps_rounds"] = [round(x, 3) for x in v]
        res[f"ingest_{k}_Gpps"] = statistics.median(v)
    alone = res["ingest_alone_Gpps"]
    res["alone_spread"] = (max(rates["alone"]) - min(rates["alone"])) / alone
    for k in cases:
        if k != "alone":
            res[f"cost_{k}_share_of_alone"] = 1.0 - res[f"ingest_{k}_Gpps"] / alone
    view.close()
    ss.close()
    return res


def main() -> int:
    args = parse_args()
    if args.child:
        fn = {"refresh": step_refresh, "calls": step_calls, "ingest": step_ingest}[args.child]
        print(json.dumps(fn(args, args.geometry[0])), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    for geometry in args.geometry:
        d, w = (int(x) for x in geometry.split("x"))
        res = {"depth": d, "width": w, "cells": d * w, "m": SS_M, "threshold": SS_THR, "window_packets": args.window}
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--geometry", geometry,
                   "--window", str(args.window), "--windows", str(args.windows), "--period", str(args.period),
                   "--rounds", str(args.rounds), "--warm-windows", str(args.warm_windows),
                   "--reps", str(args.reps), "--warmup", str(args.warmup), "--device", str(args.device)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"{geometry}, step {step}: no result within {args.step_timeout} s; stopping", file=sys.stderr)
                return 2
            if out.returncode != 0:
                print(f"{geometry}, step {step}: exit {out.returncode}; stopping\n{out.stdout}\n{out.stderr}",
                      file=sys.stderr)
                return 2
            res[step] = json.loads(out.stdout.strip().splitlines()[-1])
            print(f"{geometry} {step}: {json.dumps(res[step])}", flush=True)
        with open(os.path.join(args.out, f"ss_view_{d * w}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
