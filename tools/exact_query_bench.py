#!/usr/bin/env python3
"""The exact engine's query plane against the path it replaces, on one GPU.

For each table size (resident five-tuple flows; default 2^20 and 2^22) a handle is filled
with the synthetic stream (SyntheticTraffic(flows=N, zipf_s=0.2), 12 packets per flow, so
practically every flow is resident), then, after a warm-up of every shape timed:

  aggregate      gns_ex_aggregate at nf = 1 (the unfiltered totals), 4, 16 and 64 (single-field
                 filters taken from the heaviest flows: SrcIP, DstPort, Protocol)
  heavy_hitters  gns_ex_heavy_hitters(limit=100), PacketCount and ByteCount
  snapshot       the path both replace: snapshot_arrays() (every flow to the host) plus the
                 numpy reduction of the totals / the top-100 selection

Device times are the handle's "query" stage (HIP events around the device work of a call, the
host round trip between heavy_hitters' two phases included); wall times are a host clock
around the synchronous calls.  The byte model of the scan is per table slot: the record's tag
and key words plus four 8-byte state words (pkts, bytes, start, end); `hbm_fraction` is that
over the device time over 8 TB/s.  The device answers are checked against the snapshot path
in the same run.  One JSON per size goes to profiles/exact_query_<flows>.json.

    python tools/exact_query_bench.py [--flows 1048576 4194304] [--reps 20] [--out profiles]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
HBM_BYTES_PER_S = 8e12


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--flows", type=int, nargs="+", default=[1 << 20, 1 << 22])
    ap.add_argument("--packets-per-flow", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from go2netspectra_amd import ExactAggregator, SyntheticTraffic, make_filter
    from go2netspectra_amd.task import go_ip_string

    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    os.makedirs(args.out, exist_ok=True)

    for target in args.flows:
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
        slots = agg.dict_stats()["slots"]
        nkw = (agg.key_bytes + 3) // 4
        model_bytes = slots * (4 * (1 + nkw) + 32)
        agg.set_timing(True, stages=["query"])

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            agg.flush()
            agg.stage_times(reset=True)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                out = fn()
            wall = (time.perf_counter() - t0) / args.reps
            agg.flush()
            ms, _ = agg.stage_times(reset=True)["query"]
            return out, {"device_ms": ms / args.reps, "wall_ms": wall * 1e3}

        res = {"flows_target": target, "packets": total, "slots": slots, "key_bytes": agg.key_bytes,
               "model_bytes_per_scan": model_bytes, "reps": args.reps, "warmup": args.warmup}
        # filters from the heaviest flows: they match
        hk, _ = agg.heavy_hitters(0, 0, 64)
        flt = [make_filter()]
        for i, k in enumerate(hk):
            k = bytes(k)
            flt.append([make_filter(src_ip=go_ip_string(k[0:16])),
                        make_filter(dst_port=int.from_bytes(k[34:36], "big")),
                        make_filter(protocol=k[36])][i % 3])
        agg_out = {}
        for nf in (1, 4, 16, 64):
            out, t = timed(lambda: agg.aggregate(flt[:nf]))
            t["hbm_fraction"] = model_bytes / (t["device_ms"] * 1e-3) / HBM_BYTES_PER_S
            t["model_GBps"] = model_bytes / (t["device_ms"] * 1e-3) / 1e9
            res[f"aggregate_nf{nf}"] = t
            agg_out[nf] = out
        # 64 filters that each name one flow's source address: the cost of testing a batch
        # without the cost of merging what dense filters match
        sel = [make_filter(src_ip=go_ip_string(bytes(k)[0:16])) for k in hk]
        sel_out, t = timed(lambda: agg.aggregate(sel))
        t["hbm_fraction"] = model_bytes / (t["device_ms"] * 1e-3) / HBM_BYTES_PER_S
        res[f"aggregate_nf{len(sel)}_selective"] = t
        res["matched_flows_nf64"] = sum(s.flows for s in agg_out[64])
        res["matched_flows_nf64_selective"] = sum(s.flows for s in sel_out)
        hh_out = {}
        for metric, name in ((0, "packets"), (1, "bytes")):
            hh_out[metric], res[f"heavy_hitters_{name}_limit100"] = timed(lambda: agg.heavy_hitters(metric, 0, 100))

        # the path they replace: every flow to the host, then numpy
        def snapshot_totals():
            keys, st, en, pk, by = agg.snapshot_arrays()
            return (len(pk), int(pk.sum()), int(by.sum()), int(st.min()), int(en.max()), int(pk.max()), int(by.max()))

        def snapshot_top100(metric):
            keys, st, en, pk, by = agg.snapshot_arrays()
            v = by if metric else pk
            cut = np.partition(v, len(v) - 100)[len(v) - 100]
            cand = np.flatnonzero(v >= cut)
            rows = sorted(((-int(v[i]), bytes(keys[i])) for i in cand))[:100]
            return [(k, -nv) for nv, k in rows]

        agg.set_timing(False)
        snap_reps = max(2, args.reps // 5)

        def wall(fn):
            fn()
            t0 = time.perf_counter()
            for _ in range(snap_reps):
                out = fn()
            return out, {"wall_ms": (time.perf_counter() - t0) / snap_reps * 1e3, "reps": snap_reps}

        tot, res["snapshot_totals"] = wall(snapshot_totals)
        top, res["snapshot_top100_packets"] = wall(lambda: snapshot_top100(0))
        s = agg_out[1][0]
        res["flows_resident"] = s.flows
        assert (s.flows, s.packets, s.bytes, s.first_ns, s.last_ns, s.max_packets, s.max_bytes) == tot, (s, tot)
        assert agg_out[64][:16] == agg_out[16] and agg_out[16][0] == s
        assert [(bytes(k), int(v)) for k, v in zip(*hh_out[0])] == top
        assert [(bytes(k), int(v)) for k, v in zip(*hh_out[1])] == snapshot_top100(1)
        res["speedup_totals_wall"] = res["snapshot_totals"]["wall_ms"] / res["aggregate_nf1"]["wall_ms"]
        res["speedup_top100_wall"] = res["snapshot_top100_packets"]["wall_ms"] / res["heavy_hitters_packets_limit100"]["wall_ms"]
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(args.out, f"exact_query_{target}.json"), "w") as f:
            f.write(line + "\n")
        agg.close()
        syn.close()
        del hdr, wl
    return 0


if __name__ == "__main__":
    sys.exit(main())
