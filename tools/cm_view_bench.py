#!/usr/bin/env python3
"""Count-Min's detached snapshot view against the plain view and the serial window cycle, on one GPU.

For each geometry (the headline d=4 w=2^20, and configs[4]'s d=8 w=2^24; 5-tuple flows, K=37)
a handle ingests bench.py's stream (SyntheticTraffic, a Zipf mix over 2^20 flows) in
device-resident windows of --window packets.  Two steps follow, each in a fresh child
process under its own time limit (a step that fails or runs out of time ends the run:
nothing more is started on the GPU):

  refresh  device time of view.refresh() and of view.refresh(detach=True): HIP events on
           the handle's stream (gns_cm_stream) around the call, after warm-up calls (the
           first detached refresh allocates its buffers); with them the live flows, the
           dictionary slots and the view's bytes.  The detached view's lists are asserted
           equal to the handle's at the same point first.
  cycle    the window cycle's time on the ingest thread, per window, both forms interleaved
           in one process, --rounds pairs of --windows windows each:
             serial    insert the window, heavy hitters on the handle, reset
             detached  insert the window, view.refresh(detach=True), reset; a reader
                       thread lists the view while the next window is inserted
           Window generation is outside the sums.  The condition recorded is that in
           every pair the detached form's time per window is below the serial form's.

One JSON per geometry goes to profiles/cm_view_<depth>x<width>.json.

    python tools/cm_view_bench.py [--geometry 4x1048576 8x16777216] [--window 100000000] [--out profiles]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("refresh", "cycle")
FIELDS = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
SIZE_THR, COUNT_THR = 1 << 20, 1000  # bench.py's


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--geometry", nargs="+", default=["4x1048576", "8x16777216"], help="depth x width")
    ap.add_argument("--window", type=int, default=100_000_000)
    ap.add_argument("--windows", type=int, default=12, help="windows per form of a pair")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved pairs")
    ap.add_argument("--max-flows", type=int, default=1 << 22)
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
    """Fresh windows of the stream, generated outside the timed regions."""

    def __init__(self, args, torch, dev):
        from go2netspectra_amd import SyntheticTraffic
        self.torch, self.n, self.k = torch, args.window, 0
        self.syn = SyntheticTraffic(device=args.device)
        self.hdr = torch.empty((self.n, 64), dtype=torch.uint8, device=dev)
        self.wl = torch.empty((self.n,), dtype=torch.int32, device=dev)

    def next(self):
        self.syn.fill(self.hdr, self.wl, first=self.k * self.n)
        self.k += 1
        self.torch.cuda.synchronize()
        return self.hdr, self.wl


def opened(args, geometry):
    """(torch, device, handle, stream)"""
    import torch
    from go2netspectra_amd import CountMin
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    d, w = (int(x) for x in geometry.split("x"))
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    cm = CountMin(w, d, SIZE_THR, COUNT_THR, flow_fields=FIELDS, seeds=row_seeds(d), max_flows=args.max_flows,
                  batch_packets=args.window, device=args.device)
    return torch, dev, cm, Stream(args, torch, dev)


def step_refresh(args, geometry):
    import numpy as np
    torch, dev, cm, st = opened(args, geometry)
    cm.insert_headers(*st.next())
    cm.flush()
    view = cm.view()
    view.refresh(detach=True)
    got, want = view.heavy_hitters_arrays(), cm.heavy_hitters_arrays()
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), "detached view's lists differ from the handle's"
    ext = torch.cuda.ExternalStream(cm.stream(), device=dev)  # the handle's own stream
    res = {"reps": args.reps, "warmup": args.warmup, "heavy_hitters": [int(len(want[1])), int(len(want[3]))]}
    for name, detach in (("refresh_plain_device_ms", False), ("refresh_detached_device_ms", True)):
        for _ in range(args.warmup):
            view.refresh(detach=detach)
        cm.flush()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            view.refresh(detach=detach)
            e1.record(ext)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res[name] = float(np.median(ms))
        res[name + "_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
    ds = cm.dict_stats()
    cells = cm.depth * cm.width
    res["dict_slots"], res["claimed_slots"] = int(ds["slots"]), int(ds["claimed"])
    cm.reclaim()  # what it keeps is what the buckets name: the rows of a detached view's table
    res["live_flows"] = int(cm.dict_stats()["live"])
    res["view_bucket_bytes"] = 16 * cells
    res["view_slot_word_bytes"] = 4 * res["dict_slots"]
    res["view_table_bytes_live"] = 64 * res["live_flows"]
    res["view_bytes"] = res["view_bucket_bytes"] + res["view_slot_word_bytes"] + res["view_table_bytes_live"]
    view.close()
    cm.close()
    return res


def step_cycle(args, geometry):
    import queue
    import statistics
    import threading
    torch, dev, cm, st = opened(args, geometry)
    view = cm.view()
    list_ms, list_len, errors = [], [], []
    todo = queue.Queue()

    def reader():
        try:
            while todo.get():
                t0 = time.perf_counter()
                hh = view.heavy_hitters_arrays()
                list_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
                list_len.append([int(len(hh[1])), int(len(hh[3]))])
        except Exception as e:  # reported by the main thread
            errors.append(e)

    def serial(windows):
        elapsed, lens = 0.0, []
        for _ in range(windows):
            hdr, wl = st.next()
            t0 = time.perf_counter()
            cm.insert_headers(hdr, wl)
            hh = cm.heavy_hitters_arrays()
            cm.reset()  # synchronizes the handle's stream
            elapsed += time.perf_counter() - t0
            lens.append([int(len(hh[1])), int(len(hh[3]))])
        return elapsed / windows * 1e3, lens

    def detached(windows):
        elapsed = 0.0
        for _ in range(windows):
            hdr, wl = st.next()
            t0 = time.perf_counter()
            cm.insert_headers(hdr, wl)
            view.refresh(detach=True)  # waits for the reader's list of the previous window, if it still runs
            cm.reset()
            elapsed += time.perf_counter() - t0
            todo.put(True)
        return elapsed / windows * 1e3

    th = threading.Thread(target=reader)
    th.start()
    pairs, serial_lens = [], []
    try:
        serial(2)  # warm both forms: the lists' buffers, the view's table
        detached(2)
        for _ in range(args.rounds):
            s_ms, lens = serial(args.windows)
            d_ms = detached(args.windows)
            pairs.append({"serial_ms_per_window": round(s_ms, 4), "detached_ms_per_window": round(d_ms, 4)})
            serial_lens = lens
    finally:
        todo.put(False)
        th.join()
    assert not errors, errors
    res = {"window_packets": args.window, "windows": args.windows, "rounds": args.rounds, "pairs": pairs,
           "serial_ms_per_window": statistics.median(p["serial_ms_per_window"] for p in pairs),
           "detached_ms_per_window": statistics.median(p["detached_ms_per_window"] for p in pairs),
           "detached_below_serial_in_every_pair": all(p["detached_ms_per_window"] < p["serial_ms_per_window"]
                                                      for p in pairs),
           "reader_list_wall_ms_median": statistics.median(list_ms), "reader_list_wall_ms_max": max(list_ms),
           "reader_lists": len(list_ms), "list_lengths_last_serial_window": serial_lens[-1],
           "list_lengths_last_reader_window": list_len[-1]}
    view.close()
    cm.close()
    return res


def main() -> int:
    args = parse_args()
    if args.child:
        fn = {"refresh": step_refresh, "cycle": step_cycle}[args.child]
        print(json.dumps(fn(args, args.geometry[0])), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    for geometry in args.geometry:
        d, w = (int(x) for x in geometry.split("x"))
        res = {"depth": d, "width": w, "cells": d * w, "key_bytes": 37, "size_threshold": SIZE_THR,
               "count_threshold": COUNT_THR, "window_packets": args.window, "max_flows": args.max_flows}
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--geometry", geometry,
                   "--window", str(args.window), "--windows", str(args.windows), "--rounds", str(args.rounds),
                   "--max-flows", str(args.max_flows), "--reps", str(args.reps), "--warmup", str(args.warmup),
                   "--device", str(args.device)]
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
        with open(os.path.join(args.out, f"cm_view_{d}x{w}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
