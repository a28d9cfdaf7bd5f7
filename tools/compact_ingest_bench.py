#!/usr/bin/env python3
"""What compact records (16 bytes + the wire length, or 16 bytes alone) buy SuperSpread, the
exact spread engine and the exact aggregator, beside the 64-byte header records.

Per engine, on the stream the README quotes for it (SuperSpread and exact spread: configs[2],
SyntheticTraffic(fanout=2^20), flow SrcIP, element DstIP; exact aggregator: the Zipf(1.1)
5-tuple stream, five-tuple key), in windows of --packets:

  device   insert + flush of a device-resident window as headers (twice: two handles fed the
           same windows, whose difference is the run-to-run spread of a repeated form), as
           compact records (20 B/packet) and as compact16 (16 B/packet; 24 with the exact
           aggregator's timestamps); SuperSpread's compact forms under both GNS_SS_PIPE
           settings (1: the pipelined S1 k_ss_extract_rec; 0: the generic instantiation, which
           is also what an unset GNS_SS_PIPE selects for compact records; one of them twice)
  host     the same three forms from pinned host memory, after a reset, over the same windows

Every form has its own handle, every handle sees every window, and within a window the forms
run one after the other in an order that rotates from window to window.  The conversion to
the compact forms (compact_headers) and the copies into the pinned buffers are not timed here.
Count-Min's insert_compact from pinned host memory runs in the same process on the 5-tuple
stream: its bytes per second over the bus are the yardstick for the host-fed rates.

A Manager with the reference's default three tasks (configs/config.yaml: cm_src_left,
ss_src_dst, per_five_tuple) is fed device windows as headers to each task, and as one
compact_headers conversion (timed) followed by compact records to each task.

Results: profiles/compact_ingest_<packets>.json (one line) and the same line on stdout.

    python tools/compact_ingest_bench.py [--packets 25000000] [--steps 3] [--warmup 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
SS_FANOUT = 1 << 20
MANAGER_CFG = """
aggregator:
  types: ["sketch", "exact"]
  sketch:
    tasks:
      - {name: ss_src_dst, skt_type: 1, flow_fields: [SrcIP], element_fields: [DstIP], width: 32768, depth: 2,
         count_thereshold: 1, m: 128, size: 5, b: 1.08, base: 0.5}
      - {name: cm_src_left, skt_type: 0, flow_fields: [SrcIP], element_fields: [DstIP, SrcPort, DstPort, Protocol],
         width: 32768, depth: 2, size_thereshold: 4096000, count_thereshold: 4096}
  exact:
    tasks:
      - {name: per_five_tuple, key_fields: [SrcIP, DstIP, SrcPort, DstPort, Protocol], num_shards: 128}
"""


def main() -> int:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packets", type=int, default=25_000_000, help="packets per window")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(root, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from go2netspectra_amd import (CountMin, ExactSpread, HeaderBatch, Manager, SuperSpread,
                                   SyntheticTraffic, compact_headers, parse_config)
    from go2netspectra_amd.exact import ExactAggregator

    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    os.makedirs(args.out, exist_ok=True)
    n, nwin = args.packets, args.warmup + args.steps
    hdr = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    wl = torch.empty((n,), dtype=torch.int32, device=dev)
    ts = torch.arange(n, dtype=torch.int64, device=dev)

    def pinned(t):
        return torch.empty(t.shape, dtype=t.dtype, pin_memory=True)

    pin = {"hdr": pinned(hdr), "wl": pinned(wl), "ts": pinned(ts), "rec": pinned(hdr[:, :16]), "rec16": pinned(hdr[:, :16])}
    pin["ts"].copy_(ts)

    def window(syn, w, host):
        """Window w of the stream in every form: device tensors, and the pinned copies when host."""
        syn.fill(hdr, wl, first=w * n)
        f = {"hdr": hdr, "wl": wl}
        f["rec"], f["side"] = compact_headers(hdr, wl)
        f["rec16"], f["side16"] = compact_headers(hdr, wl, rec_len=True)
        if host:
            for k in ("hdr", "wl", "rec", "rec16"):
                pin[k].copy_(f[k])
            f["hside"] = f["side"].cpu().numpy()  # the escapes' records: a sliver of the stream, staged once per call
            f["hside16"] = f["side16"].cpu().numpy()
        torch.cuda.synchronize(dev)
        return f

    def insert(h, form, f, host, with_ts):
        """One window into handle h in the given form."""
        if host:
            t = (pin["ts"].numpy(),) if with_ts else ()
            if form == "headers":
                h.insert_headers(pin["hdr"].numpy(), pin["wl"].numpy().view(np.uint32), *t)
            elif form == "compact":
                h.insert_compact(pin["rec"].numpy(), pin["wl"].numpy().view(np.uint32), *t, f["hside"])
            else:
                h.insert_compact(pin["rec16"].numpy(), None, *t, f["hside16"])
        else:
            t = (ts,) if with_ts else ()
            if form == "headers":
                h.insert_headers(f["hdr"], f["wl"], *t)
            elif form == "compact":
                h.insert_compact(f["rec"], f["wl"], *t, f["side"])
            else:
                h.insert_compact(f["rec16"], None, *t, f["side16"])
        h.flush()

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def summary(times):
        """Gpackets/s of the timed windows: median, best, every window."""
        rates = [n / t / 1e9 for t in times]
        return {"gpps_median": round(statistics.median(rates), 3), "gpps_best": round(max(rates), 3),
                "gpps": [round(r, 3) for r in rates]}

    def run_engine(name, syn, handles, with_ts, bytes_per_packet):
        """handles: {label: (handle, form)}.  Device phase, reset, host phase over the same windows."""
        out = {"device": {}, "host": {}}
        labels = list(handles)
        for phase in ("device", "host"):
            host = phase == "host"
            use = [k for k in labels if not (host and k.endswith("_repeat"))]
            times = {k: [] for k in use}
            before = {k: handles[k][0].counters() for k in use}
            for w in range(nwin):
                f = window(syn, w, host)
                order = use[w % len(use):] + use[:w % len(use)]  # the forms alternate inside the process
                for k in order:
                    h, form = handles[k]
                    t = timed(lambda: insert(h, form, f, host, with_ts))
                    if w >= args.warmup:
                        times[k].append(t)
            for k in use:
                out[phase][k] = summary(times[k])
                if host:
                    bpp = bytes_per_packet[handles[k][1]]
                    out[phase][k]["bytes_per_packet"] = bpp
                    out[phase][k]["bus_gb_s"] = round(out[phase][k]["gpps_median"] * bpp, 1)
            names = ("inserted", "dropped", "unsupported")
            counters = {k: {x: handles[k][0].counters()[x] - before[k][x] for x in names} for k in use}
            first = counters[use[0]]
            out[phase]["counters_agree"] = bool(all(c == first for c in counters.values()) and first["inserted"] == n * nwin)
            for h, _ in handles.values():
                h.reset()
        a, b = out["device"]["headers"]["gpps_median"], out["device"]["headers_repeat"]["gpps_median"]
        out["spread_of_repeated_form"] = round(abs(a - b) / max(a, b), 4)
        print(f"# {name}: {json.dumps(out)}", file=sys.stderr, flush=True)
        return out

    res = {"tool": "compact_ingest_bench", "packets_per_window": n, "steps": args.steps, "warmup": args.warmup,
           "timing": "wall clock around insert + flush, device idle before and after; one handle per form, "
                     "forms rotated inside every window; conversion and pinned copies untimed"}

    # --- SuperSpread: configs[2] ---------------------------------------------------------------
    def new_ss(pipe):
        os.environ["GNS_SS_PIPE"] = pipe  # read when the handle is created
        h = SuperSpread(32768, 2, 4096, 128, 5, 0.5, 1.08, flow_fields=["SrcIP"], elem_fields=["DstIP"],
                        hll_master=0x0123456789ABCDEF, rng_seed=0x0DDBA11CAFEF00D5, batch_packets=n, device=args.device)
        os.environ.pop("GNS_SS_PIPE")
        return h

    syn_ss = SyntheticTraffic(device=args.device, fanout=SS_FANOUT)
    bpp = {"headers": 68, "compact": 20, "compact16": 16}
    ss_handles = {"headers": (new_ss("1"), "headers"), "headers_repeat": (new_ss("1"), "headers"),
                  "compact_pipe1": (new_ss("1"), "compact"), "compact16_pipe1": (new_ss("1"), "compact16"),
                  "headers_pipe0": (new_ss("0"), "headers"), "compact_pipe0": (new_ss("0"), "compact"),
                  "compact16_pipe0": (new_ss("0"), "compact16"), "compact_pipe0_repeat": (new_ss("0"), "compact")}
    res["superspread"] = run_engine("superspread", syn_ss, ss_handles, False, bpp)
    res["superspread"]["stream"] = "configs[2]: SyntheticTraffic(fanout=2^20), flow SrcIP, element DstIP, d=2 w=32768 m=128"
    for h, _ in ss_handles.values():
        h.close()
    del ss_handles

    # --- exact spread: the same stream, tables sized for it ----------------------------------------
    def new_exs():
        return ExactSpread(["SrcIP"], ["DstIP"], max_flows=1 << 21, max_pairs=1 << 26, batch_packets=n, device=args.device)

    exs_handles = {"headers": (new_exs(), "headers"), "headers_repeat": (new_exs(), "headers"),
                   "compact": (new_exs(), "compact"), "compact16": (new_exs(), "compact16")}
    res["exact_spread"] = run_engine("exact_spread", syn_ss, exs_handles, False, bpp)
    res["exact_spread"]["stream"] = "configs[2] stream, distinct DstIP per SrcIP, max_pairs 2^26, max_flows 2^21"
    for h, _ in exs_handles.values():
        h.close()
    del exs_handles

    # --- exact aggregator: the Zipf 5-tuple stream ---------------------------------------------------
    syn_ex = SyntheticTraffic(device=args.device)

    def new_ex():
        return ExactAggregator(FIVE, max_flows=1 << 21, batch_packets=n, device=args.device)

    ex_handles = {"headers": (new_ex(), "headers"), "headers_repeat": (new_ex(), "headers"),
                  "compact": (new_ex(), "compact"), "compact16": (new_ex(), "compact16")}
    res["exact"] = run_engine("exact", syn_ex, ex_handles, True, {"headers": 76, "compact": 28, "compact16": 24})
    res["exact"]["stream"] = "SyntheticTraffic() Zipf(1.1) over 2^20 5-tuples, five-tuple key, timestamps"
    for h, _ in ex_handles.values():
        h.close()
    del ex_handles

    # --- the PCIe yardstick: Count-Min's compact ingest from pinned host memory ----------------------
    cms = {"compact": CountMin(1 << 20, 4, 512 * 1024, 512, flow_fields=FIVE, batch_packets=n, device=args.device),
           "compact16": CountMin(1 << 20, 4, 512 * 1024, 512, flow_fields=FIVE, batch_packets=n, device=args.device)}
    times = {k: [] for k in cms}
    for w in range(nwin):
        f = window(syn_ex, w, True)
        for k in (list(cms) if w % 2 == 0 else list(cms)[::-1]):
            t = timed(lambda: insert(cms[k], k, f, True, False))
            if w >= args.warmup:
                times[k].append(t)
    res["count_min_host"] = {}
    for k in cms:
        s = summary(times[k])
        s["bytes_per_packet"] = bpp[k]
        s["bus_gb_s"] = round(s["gpps_median"] * bpp[k], 1)
        res["count_min_host"][k] = s
        cms[k].close()
    res["count_min_host"]["stream"] = "the 5-tuple stream, d=4 w=2^20, five-tuple key"
    print(f"# count_min_host: {json.dumps(res['count_min_host'])}", file=sys.stderr, flush=True)

    # --- Manager, the reference's default three tasks ---------------------------------------------------
    cfg = parse_config(MANAGER_CFG)

    def new_mgr():
        m = Manager(cfg, batch_packets=n, max_flows=1 << 21, hll_master=0x0123456789ABCDEF, rng_seed=0x0DDBA11CAFEF00D5,
                    device=args.device)
        m.start()
        return m

    def flush(m):
        for t in m.tasks():
            t.flush()

    def feed_headers(m):
        m.process(HeaderBatch(hdr, wl, ts))
        flush(m)

    def feed_compact(m, rec_len):
        m.process(HeaderBatch(hdr, wl, ts).compact(rec_len=rec_len))  # the conversion is inside the timed call
        flush(m)

    mgrs = {"headers_to_each": (new_mgr(), feed_headers), "headers_to_each_repeat": (new_mgr(), feed_headers),
            "compact_once": (new_mgr(), lambda m: feed_compact(m, False)),
            "compact16_once": (new_mgr(), lambda m: feed_compact(m, True))}
    times = {k: [] for k in mgrs}
    labels = list(mgrs)
    for w in range(nwin):
        syn_ex.fill(hdr, wl, first=w * n)
        for k in labels[w % len(labels):] + labels[:w % len(labels)]:
            m, fn = mgrs[k]
            t = timed(lambda: fn(m))
            if w >= args.warmup:
                times[k].append(t)
    res["manager"] = {k: summary(times[k]) for k in mgrs}

    def outcome(m):
        """Per task: the record counters, and the heavy list (sketches) or the flow count (exact)."""
        out = {}
        for t in m.tasks():
            eng = t.sketch if hasattr(t, "sketch") else t.agg
            c = eng.counters()
            what = [(h.Flow, h.Count) for h in t.snapshot().Count] if hasattr(t, "sketch") else c["flows"]
            out[t.name()] = ([c[x] for x in ("inserted", "dropped", "unsupported")], what)
        return out

    # one further window, task by task: where a form's time goes (the conversion on its own)
    syn_ex.fill(hdr, wl, first=nwin * n)
    per_task = {}
    for k, (m, _) in mgrs.items():
        if k.endswith("_repeat"):
            continue
        box, ms = {}, {}
        if k == "headers_to_each":
            box["b"] = HeaderBatch(hdr, wl, ts)
        else:
            ms["compact_headers"] = timed(lambda: box.update(b=HeaderBatch(hdr, wl, ts).compact(rec_len=k == "compact16_once")))
        for t in m.tasks():
            ms[t.name()] = timed(lambda: (t.process_packets(box["b"]), t.flush()))
        per_task[k] = {x: round(v * 1e3, 3) for x, v in ms.items()}
    res["manager"]["per_task_ms"] = per_task
    outs = {k: outcome(m) for k, (m, _) in mgrs.items() if not k.endswith("_repeat")}
    res["manager"]["snapshots_agree"] = bool(all(o == outs["headers_to_each"] for o in outs.values()))
    a, b = res["manager"]["headers_to_each"]["gpps_median"], res["manager"]["headers_to_each_repeat"]["gpps_median"]
    res["manager"]["spread_of_repeated_form"] = round(abs(a - b) / max(a, b), 4)
    res["manager"]["stream"] = "the 5-tuple stream; tasks cm_src_left, ss_src_dst, per_five_tuple (configs/config.yaml)"
    res["manager"]["note"] = "Gpackets/s of the window through all three tasks; the compact forms include compact_headers"

    ok = all(res[e][p]["counters_agree"] for e in ("superspread", "exact_spread", "exact") for p in ("device", "host"))
    res["check"] = "green" if ok and res["manager"]["snapshots_agree"] else "RED"
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(args.out, f"compact_ingest_{n}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["check"] == "green" else 1


if __name__ == "__main__":
    sys.exit(main())
