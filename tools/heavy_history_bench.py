#!/usr/bin/env python3
"""The heavy-hitter history (gns_hh_hist_*) on one GPU, next to the host route it replaces.

Default shape: K = 37; 256 snapshots of one 65,536-row list each (type 0); flows drawn from a
seeded population so that half of each list repeats earlier flows -- about 16.8M rows and 8.4M
flows.  Lists are built on the device (packed rows [flow | u32]), as the engines hand them over.
In ONE child process under a time limit (a child that fails or runs out of time ends the run:
nothing more is started on the GPU):

  append    wall time of every history.append (the call ends in a synchronise): the median,
            smallest and largest over the appends that grew nothing, and apart from them the
            appends during which the key index or the log grew
  list      history.heavy_hitters as of the newest and as of the middle snapshot: limit 10,
            limit 1000, and limit 0 with a threshold that keeps about 1% of the rows
            (median / min / max over --reps calls after --warmup)
  export    export_log once; save and restore into a fresh history once, the restored answers
            asserted equal
  host      the route without the store, on the same data in the same run: the exported log, a
            numpy latest-per-key, a sort by (value desc, flow bytes asc); its first 10 rows and
            its 1% list asserted equal to the device's

One JSON goes to profiles/heavy_history_<rows>.json.

    python tools/heavy_history_bench.py [--snapshots 256] [--list-rows 65536] [--out profiles]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--key-bytes", type=int, default=37)
    ap.add_argument("--snapshots", type=int, default=256)
    ap.add_argument("--list-rows", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20240)
    ap.add_argument("--timeout", type=int, default=840, help="seconds for the child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)} if ms else {"n": 0}


def timed(args, fn):
    for _ in range(args.warmup):
        fn()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, spread(ms)


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def child(args):
    import numpy as np
    import torch
    from go2netspectra_amd import HeavyHistory
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host alone"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    K, S, n = args.key_bytes, args.snapshots, args.list_rows
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    mult = torch.tensor([(2654435761 * (2 * j + 1)) % (1 << 31) | 1 for j in range(K)], dtype=torch.int64, device=dev)

    def rows_of(ids):
        """ids (int64, distinct) -> packed rows: bytes 0..3 the id itself (so flows are distinct),
        the others a mix of it; a uniform u32 value."""
        m = ids.shape[0]
        rows = torch.empty((m, K + 4), dtype=torch.uint8, device=dev)
        mixed = ((ids[:, None] * mult[None, :]) >> 11) & 255
        rows[:, :K] = mixed.to(torch.uint8)
        for b in range(min(4, K)):
            rows[:, b] = ((ids >> (8 * b)) & 255).to(torch.uint8)
        vals = torch.randint(0, 1 << 32, (m,), dtype=torch.int64, device=dev, generator=gen)
        for b in range(4):
            rows[:, K + b] = ((vals >> (8 * b)) & 255).to(torch.uint8)
        return rows

    hist = HeavyHistory(K, device=args.device)
    res = {"key_bytes": K, "snapshots": S, "list_rows": n, "reps": args.reps, "warmup": args.warmup}
    appends, known = [], 0
    prev = hist.stats()
    for s in range(S):
        n_old = min(n // 2, known)
        old = torch.randperm(known, device=dev, generator=gen)[:n_old] if n_old else torch.zeros(0, dtype=torch.int64, device=dev)
        ids = torch.cat([old, torch.arange(known, known + n - n_old, dtype=torch.int64, device=dev)])
        rows = rows_of(ids[torch.randperm(n, device=dev, generator=gen)])
        torch.cuda.synchronize(dev)
        out, ms = once(lambda: hist.append(1000 * (s + 1), {0: rows}))
        known += n - n_old
        st = hist.stats()
        appends.append({"ms": ms, "rows": out[0], "new": out[1],
                        "index_grew": st["index_growths"] != prev["index_growths"], "log_grew": st["log_growths"] != prev["log_growths"]})
        prev = st
        assert out == (n, n - n_old), out
    plain = [a["ms"] for a in appends[1:] if not (a["index_grew"] or a["log_grew"])]
    res["append_plain"] = spread(plain)
    res["append_first_ms"] = appends[0]["ms"]  # (allocates the lane, the staging and the resolve scratch)
    res["append_with_growth"] = [{"snapshot": i, "ms": a["ms"], "index_grew": a["index_grew"], "log_grew": a["log_grew"]}
                                 for i, a in enumerate(appends) if a["index_grew"] or a["log_grew"]]
    res["stats"] = hist.stats()
    total = res["stats"]["rows"]

    thr = int(0.99 * (1 << 32))
    mid = 1000 * (S // 2)
    lists = {}
    for name, T in (("newest", None), ("middle", mid)):
        q = {}
        for what, kw in (("limit_10", dict(limit=10)), ("limit_1000", dict(limit=1000)), ("threshold_1pct", dict(threshold=thr))):
            out, t = timed(args, lambda: hist.heavy_hitters(0, end_time=T, **kw))
            q[what] = dict(t, rows=int(len(out[1])))
        lists[name] = q
    res["list"] = lists

    # --- export, save, restore ---
    log, ms = once(hist.export_log)
    res["export_log_ms"] = ms
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "h.npz")
        _, res["save_ms"] = once(lambda: hist.save(path))
        res["file_mb"] = os.path.getsize(path) / 1e6
        back = HeavyHistory(K, device=args.device)
        _, res["restore_ms"] = once(lambda: back.restore(path))
    for T in (None, mid):
        for kw in (dict(limit=1000), dict(threshold=thr)):
            a, b = hist.heavy_hitters(0, end_time=T, **kw), back.heavy_hitters(0, end_time=T, **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the restored history answers differently"
    assert back.times() == hist.times() and back.stats()["rows"] == total
    back.close()

    # --- the host route: latest per key over the exported log, then the order ---
    ty, fl, va, wr, ts = log

    def host_route():
        kv = np.ascontiguousarray(fl[::-1]).view(np.dtype((np.void, K))).reshape(-1)
        _, first = np.unique(kv, return_index=True)  # the first from the end: the flow's latest row (one type, log order)
        lf, lv = fl[::-1][first], va[::-1][first]
        order = np.lexsort((np.arange(len(lv)), -lv.astype(np.int64)))  # (unique sorted the flows: index order is byte order)
        return lf[order], lv[order]
    (hf, hv), ms = once(host_route)
    res["host_latest_and_sort_ms"] = ms
    res["host_route_ms"] = res["export_log_ms"] + ms
    res["live_rows"] = int(len(hv))
    d10 = hist.heavy_hitters(0, limit=10)
    assert np.array_equal(d10[0], hf[:10]) and np.array_equal(d10[1], hv[:10].astype(np.uint64)), "limit 10 differs from the host route"
    dth = hist.heavy_hitters(0, threshold=thr)
    keep = hv >= thr
    assert np.array_equal(dth[0], hf[keep]) and np.array_equal(dth[1], hv[keep].astype(np.uint64)), "the 1% list differs from the host route"
    hist.close()
    return res


def main() -> int:
    args = parse_args()
    if args.child:
        print(json.dumps(child(args)), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--key-bytes", str(args.key_bytes), "--snapshots",
           str(args.snapshots), "--list-rows", str(args.list_rows), "--reps", str(args.reps), "--warmup", str(args.warmup),
           "--seed", str(args.seed), "--device", str(args.device)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s; stopping", file=sys.stderr)
        return 2
    if out.returncode != 0:
        print(f"exit {out.returncode}; stopping\n{out.stdout}\n{out.stderr}", file=sys.stderr)
        return 2
    res = json.loads(out.stdout.strip().splitlines()[-1])
    rows = res["stats"]["rows"]
    print(json.dumps(res), flush=True)
    with open(os.path.join(args.out, f"heavy_history_{rows}.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
