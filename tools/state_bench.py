#!/usr/bin/env python3
"""What restoring engine state costs, beside the only other route to that state.

Per Count-Min geometry (default: the headline d=4, w=2^20 and d=8, w=2^24, five-tuple keys)
a handle ingests the synthetic Zipf stream from device memory, then:

  reingest   the ingest itself (insert + flush of device-resident windows, generation excluded):
             replaying the stream is the only way to that state without an import
  export     gns_cm_export_state (wall)
  h2d        the exported bytes copied host -> device once (torch, pageable memory as the import's)
  import     gns_cm_import_state into a fresh handle: wall, and by HIP events the host-to-device
             staging ("extract" stage) and the resolve rounds ("resolve" stage; launches = rounds),
             the flows claimed (the distinct fingerprints, + 1 if a cell holds the all-zero key)
             and the table growths; the re-export is checked against the export
  exact      gns_ex_merge of a --exact-flows snapshot into a fresh table (host rows): wall and
             resolve rounds, checked against the source table's unfiltered aggregate

One JSON per geometry goes to profiles/state_import_d<d>_w<w>.json.  A geometry whose arrays
do not fit (host or device memory) is reported as skipped.

    python tools/state_bench.py [--geometries 4x1048576 8x16777216] [--packets 100000000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIVE = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]


def main() -> int:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--geometries", nargs="+", default=["4x1048576", "8x16777216"], help="depth x width")
    ap.add_argument("--packets", type=int, default=100_000_000)
    ap.add_argument("--exact-flows", type=int, default=1 << 22)
    ap.add_argument("--out", default=os.path.join(root, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from go2netspectra_amd import CountMin, ExactAggregator, GnsError, SyntheticTraffic, make_filter

    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    os.makedirs(args.out, exist_ok=True)
    win = 1 << 23

    def ingest(put, flush, syn, total, with_ts=False):
        """Windows generated on the device; returns the seconds spent in put + flush."""
        hdr = torch.empty((min(win, total), 64), dtype=torch.uint8, device=dev)
        wl = torch.empty((min(win, total),), dtype=torch.int32, device=dev)
        done, spent = 0, 0.0
        while done < total:
            m = min(win, total - done)
            syn.fill(hdr[:m], wl[:m], done)
            extra = ()
            if with_ts:
                extra = (torch.arange(done, done + m, dtype=torch.int64, device=dev) * 1000 + 1_700_000_000_000_000_000,)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            put(hdr[:m], wl[:m], *extra)
            flush()
            spent += time.perf_counter() - t0
            done += m
        return spent

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t0) * 1e3

    # the exact merge, once
    exact = {}
    if args.exact_flows:
        syn = SyntheticTraffic(flows=args.exact_flows, zipf_s=0.2, device=args.device)
        src = ExactAggregator(FIVE, max_flows=args.exact_flows, device=args.device)
        total = args.exact_flows * 12
        exact["reingest_ms"] = ingest(src.insert_headers, src.flush, syn, total, with_ts=True) * 1e3
        rows, exact["snapshot_ms"] = wall(src.snapshot_arrays)
        dst = ExactAggregator(FIVE, max_flows=args.exact_flows, device=args.device)
        dst.set_timing(True, stages=["resolve"])
        _, exact["merge_ms"] = wall(lambda: dst.merge(*rows))
        ms, rounds = dst.stage_times()["resolve"]
        exact.update(rows=len(rows[3]), packets=total, resolve_ms=ms, resolve_rounds=rounds,
                     growths=dst.dict_stats()["growths"], row_bytes=sum(a.nbytes for a in rows))
        assert dst.aggregate([make_filter()]) == src.aggregate([make_filter()])
        src.close(), dst.close(), syn.close()
        del rows
        print(json.dumps({"exact_merge": exact}), flush=True)

    for geo in args.geometries:
        d, w = (int(x) for x in geo.lower().split("x"))
        res = {"depth": d, "width": w, "key_bytes": 37, "packets": args.packets, "exact_merge": exact}
        path = os.path.join(args.out, f"state_import_d{d}_w{w}.json")
        try:
            syn = SyntheticTraffic(device=args.device)
            cm = CountMin(w, d, flow_fields=FIVE, device=args.device)
            res["reingest_ms"] = ingest(cm.insert_headers, cm.flush, syn, args.packets) * 1e3
            state, res["export_ms"] = wall(cm.export_state)
            state = [np.ascontiguousarray(a) for a in state]
            res["state_bytes"] = sum(a.nbytes for a in state)

            def h2d():
                t = [torch.from_numpy(a).to(dev) for a in state]
                torch.cuda.synchronize(dev)
                del t

            h2d()
            _, res["h2d_ms"] = wall(h2d)
            fresh = CountMin(w, d, flow_fields=FIVE, device=args.device)
            fresh.set_timing(True, stages=["extract", "resolve"])
            c = cm.counters()
            _, res["import_ms"] = wall(lambda: fresh.import_state(*state, counters=[c["inserted"], c["dropped"],
                                                                                   c["unsupported"]]))
            st = fresh.stage_times()
            ds = fresh.dict_stats()
            res.update(import_h2d_stage_ms=st["extract"][0], import_resolve_ms=st["resolve"][0],
                       resolve_rounds=st["resolve"][1], flows_claimed=ds["claimed"], growths=ds["growths"],
                       dict_slots=ds["slots"])
            fresh.set_timing(False)
            again = fresh.export_state()
            assert all(np.array_equal(a, b) for a, b in zip(again, state)), "re-export differs from the export"
            res["import_over_reingest"] = res["import_ms"] / res["reingest_ms"]
            res["import_over_h2d"] = res["import_ms"] / res["h2d_ms"]
            cm.close(), fresh.close(), syn.close()
            del state, again
        except (MemoryError, GnsError, RuntimeError) as e:  # the arrays do not fit this machine
            res["skipped"] = f"{type(e).__name__}: {e}"[:200]
        line = json.dumps(res)
        print(line, flush=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
