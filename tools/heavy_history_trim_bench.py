#!/usr/bin/env python3
"""The life cycle of a heavy-hitter history (gns_hh_hist_trim, gns_hh_hist_query, record_heavy
with ``retain``) on one GPU, next to a copy floor and the host route a user would otherwise run.

The setup is that of heavy_history_bench.py: K = 37; 256 snapshots of one 65,536-row list each
(type 0), half of each list repeating earlier flows -- about 16.8M rows and 8.4M flows.  Its log
is exported once; every trim starts from a fresh history restored from that log, so each of the
--reps timed calls after --warmup sees the same 256 snapshots.  All in ONE child process under a
time limit (a child that fails or runs out of time ends the run: nothing more is started on the
GPU).

  trim     fold the oldest 128 snapshots, fold all of them, drop the oldest 128
  floor    a device-to-device copy of as many bytes as that trim reads plus writes
  host     the route without trim, per trim: export_log, a numpy filter (drop) or latest-per-key
           (fold) of the expired rows, a fresh history fed snapshot by snapshot (each phase timed
           once); its exported log asserted equal to the trimmed history's
  query    history.query of 1, 1,024 and 65,536 flows (host rows, and device rows) as of the
           newest and as of the middle snapshot, half of the flows listed by then
  host     the point query without the store: the exported list, a numpy latest-per-key as of
           the time, a binary search of the flows; the answers asserted equal
  record   SketchTask.record_heavy of 65,536-row lists with retain=16 against record_heavy
           without it, two tasks fed the same lists (the lists come from a stand-in view)

One JSON goes to profiles/heavy_history_lifecycle_<rows>.json.

    python tools/heavy_history_trim_bench.py [--snapshots 256] [--list-rows 65536] [--out profiles]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--key-bytes", type=int, default=37)
    ap.add_argument("--snapshots", type=int, default=256)
    ap.add_argument("--list-rows", type=int, default=65536)
    ap.add_argument("--retain", type=int, default=16)
    ap.add_argument("--record-intervals", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20240)
    ap.add_argument("--timeout", type=int, default=1080, help="seconds for the child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def timed(args, fn, setup=None):
    """(last result, {median, min, max} ms) of fn over --reps calls after --warmup; setup() runs
    untimed before each call and its result is fn's argument (closed after the call)."""
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
    from go2netspectra_amd import HeavyHistory, SketchTask
    from go2netspectra_amd.heavy_history import pack_rows
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the host alone"
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    K, S, n = args.key_bytes, args.snapshots, args.list_rows
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    mult = torch.tensor([(2654435761 * (2 * j + 1)) % (1 << 31) | 1 for j in range(K)], dtype=torch.int64, device=dev)

    def rows_of(ids):
        """heavy_history_bench.py's rows: bytes 0..3 the id itself, the others a mix of it; a uniform u32 value."""
        m = ids.shape[0]
        rows = torch.empty((m, K + 4), dtype=torch.uint8, device=dev)
        rows[:, :K] = (((ids[:, None] * mult[None, :]) >> 11) & 255).to(torch.uint8)
        for b in range(min(4, K)):
            rows[:, b] = ((ids >> (8 * b)) & 255).to(torch.uint8)
        vals = torch.randint(0, 1 << 32, (m,), dtype=torch.int64, device=dev, generator=gen)
        for b in range(4):
            rows[:, K + b] = ((vals >> (8 * b)) & 255).to(torch.uint8)
        return rows

    known = [0]

    def next_list():
        n_old = min(n // 2, known[0])
        old = torch.randperm(known[0], device=dev, generator=gen)[:n_old] if n_old else torch.zeros(0, dtype=torch.int64, device=dev)
        ids = torch.cat([old, torch.arange(known[0], known[0] + n - n_old, dtype=torch.int64, device=dev)])
        known[0] += n - n_old
        rows = rows_of(ids[torch.randperm(n, device=dev, generator=gen)])
        torch.cuda.synchronize(dev)
        return rows

    hist = HeavyHistory(K, device=args.device)
    for s in range(S):
        hist.append(1000 * (s + 1), {0: next_list()})
    st = hist.stats()
    total, keys, slots = st["rows"], st["keys"], st["index_slots"]
    res = {"key_bytes": K, "snapshots": S, "list_rows": n, "reps": args.reps, "warmup": args.warmup, "stats": st}
    words = 1 + (K + 3) // 4
    rec_bytes = 4 * (4 if words <= 4 else 8 if words <= 8 else 16)
    times = hist.times()
    half, mid = S // 2, times[S // 2 - 1]

    # --- the exported log, and a fresh history from it ---
    (ty, fl, va, wr, ts), res["export_log"] = timed(args, hist.export_log)
    packed = pack_rows(fl, va, K)  # one type: log order is snapshot order
    bounds = np.searchsorted(wr, np.arange(S + 1))

    def fresh():
        h = HeavyHistory(K, max_rows=total, max_flows=keys, device=args.device)
        for s, t in enumerate(ts.tolist()):
            h.append(t, {0: packed[bounds[s]:bounds[s + 1]]})
        return h
    h0, res["restore"] = timed(args, fresh)
    assert h0.stats()["rows"] == total and h0.stats()["keys"] == keys, h0.stats()
    slots = h0.stats()["index_slots"]  # (of the histories the trims run on)
    h0.close()

    def copy_floor(nbytes):
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)

        def run():
            b.copy_(a)
            torch.cuda.synchronize(dev)
        out = timed(args, run)[1]
        del a, b
        return out

    # --- trims, each on a freshly restored history, and the host route of each ---
    def host_route(c, fold):
        (ty, fl, va, wr, ts), ms_export = once(hist.export_log)

        def filt():
            pre = int(bounds[c])
            if fold:
                kv = np.ascontiguousarray(fl[:pre][::-1]).view(np.dtype((np.void, K))).reshape(-1)
                _, first = np.unique(kv, return_index=True)  # the first from the end: the flow's latest row
                idx = np.concatenate([np.sort(pre - 1 - first), np.arange(pre, len(wr))])
                d = c - 1
            else:
                idx, d = np.arange(pre, len(wr)), c
            wn = np.maximum(wr[idx].astype(np.int64), d) - d
            return pack_rows(fl[idx], va[idx], K), wn, ts[d:]
        (rows, wn, tn), ms_filter = once(filt)

        def restore():
            h = HeavyHistory(K, max_rows=len(wn), max_flows=keys, device=args.device)
            b = np.searchsorted(wn, np.arange(len(tn) + 1))
            for s, t in enumerate(tn.tolist()):
                h.append(t, {0: rows[b[s]:b[s + 1]]})
            return h
        h, ms_restore = once(restore)
        return h, {"export_ms": ms_export, "numpy_filter_ms": ms_filter, "fresh_history_appends_ms": ms_restore,
                   "total_ms": ms_export + ms_filter + ms_restore}

    trims = {}
    for name, c, fold in (("fold_oldest_128", half, True), ("fold_all", S, True), ("drop_oldest_128", half, False)):
        before = times[c - 1] + 1
        out, ms = timed(args, lambda h: h.trim(before, fold=fold), setup=fresh)
        R, kept = int(bounds[c]), out["rows"]
        new_slots = slots
        terms = {"count_prefix_rows": 16 * R if fold else 0,  # the superseded words lie 16 bytes apart: whole rows cross the bus
                 "move_read": 16 * (total if fold else total - R), "move_write": 16 * kept, "heads_read_new_log": 16 * kept,
                 "head_words": 4 * slots * 3 + 4 * kept,  # cleared, old and new read for the forgotten count, one store per open row
                 "mark_list": 4 * slots * 3}  # cleared, read by the named count, the new heads read to fill it
        if out["pairs_forgotten"]:
            ht = fresh()
            ht.trim(before, fold=fold)
            new_slots = ht.stats()["index_slots"]
            ht.close()
            # the rebuild reads the marked table twice (count, stage), clears and fills the new one; the
            # head words and the new log's slot column follow the records
            terms["index_rebuild"] = 2 * rec_bytes * slots + rec_bytes * new_slots + 2 * rec_bytes * (keys - out["pairs_forgotten"])
            terms["permute_and_reslot"] = 8 * slots + 8 * new_slots + 8 * kept
        nbytes = sum(terms.values())
        floor = copy_floor(nbytes)
        hh, host = host_route(c, fold)
        ht = fresh()
        ht.trim(before, fold=fold)
        assert all(np.array_equal(x, y) for x, y in zip(hh.export_log(), ht.export_log())), "host route and device trim differ"
        for T in (None, times[c - 1], times[-1] - 1):
            a, b = hh.heavy_hitters(0, limit=1000, end_time=T), ht.heavy_hitters(0, limit=1000, end_time=T)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), T
        trims[name] = dict(ms, out=out, prefix_rows=R, index_slots_after=new_slots, bytes_read_plus_written=nbytes,
                           byte_terms=terms, copy_floor=floor, ratio_to_floor=ms["median_ms"] / floor["median_ms"],
                           host_route=host, host_route_over_trim=host["total_ms"] / ms["median_ms"],
                           stats_after=ht.stats())
        hh.close()
        ht.close()
    res["trim"] = trims

    # --- point queries, and the exported list searched with numpy ---
    rng = np.random.default_rng(args.seed)
    queries = {}
    host_tables = {}
    for name, T, s_of in (("newest", None, S - 1), ("middle", mid, half - 1)):
        def table():
            pre = int(bounds[s_of + 1])
            kv = np.ascontiguousarray(fl[:pre][::-1]).view(np.dtype((np.void, K))).reshape(-1)
            uk, first = np.unique(kv, return_index=True)
            return uk, va[:pre][::-1][first]
        (uk, uv), ms_table = once(table)
        host_tables[name] = ms_table
        q = {"host_latest_per_key_ms": ms_table}
        for m in (1, 1024, 65536):
            # half of the batch from the rows stored by then, half from the rows stored later (newest: never listed)
            pre = int(bounds[s_of + 1])
            a = fl[rng.integers(0, pre, m - m // 2)]
            b = fl[rng.integers(pre, total, m // 2)] if pre < total else (255 - fl[rng.integers(0, total, m // 2)])
            flows = np.ascontiguousarray(np.concatenate([a, b])[rng.permutation(m)])
            (v, f), t_host = timed(args, lambda: hist.query(0, flows, end_time=T))
            dflows = torch.from_numpy(flows).to(dev)
            torch.cuda.synchronize(dev)

            def dq():
                out = hist.query_device(0, dflows, end_time=T)
                torch.cuda.synchronize(dev)
                return out
            (dv, df), t_dev = timed(args, dq)

            def search():
                qv = flows.view(np.dtype((np.void, K))).reshape(-1)
                pos = np.minimum(np.searchsorted(uk, qv), len(uk) - 1)
                hit = uk[pos] == qv
                return np.where(hit, uv[pos], 0).astype(np.uint64), hit
            (sv, sf), ms_search = once(search)
            assert np.array_equal(v, sv) and np.array_equal(f, sf), "the point query differs from the host route"
            assert np.array_equal(dv.cpu().numpy().view(np.uint64), sv) and np.array_equal(df.cpu().numpy(), sf)
            q[f"flows_{m}"] = {"host_rows": t_host, "device_rows": t_dev, "found": int(f.sum()), "numpy_search_ms": ms_search,
                               "host_route_ms": res["export_log"]["median_ms"] + ms_table + ms_search}
        queries[name] = q
    res["query"] = queries

    # --- record_heavy with retain and without ---
    class View:  # stands in for a sketch's view: the lists are this tool's own
        rows = None

        def refresh(self):
            pass

        def heavy_hitters_rows_device(self):
            return self.rows

    class Sketch:
        device = args.device

        def view(self):
            return View()
    tasks = {}
    for name, kw in (("without_retain", {}), (f"retain_{args.retain}", dict(retain=args.retain)),
                     (f"retain_{args.retain}_drop", dict(retain=args.retain, drop=True))):
        t = SketchTask.__new__(SketchTask)
        t.name_, t.sketch, t.flow_size, t.flow_fields = name, Sketch(), K, []
        t.keep_heavy_history(**kw)
        tasks[name] = (t, [])
    known[0] = 0
    for i in range(args.record_intervals):
        rows = next_list()
        for name, (t, ms) in tasks.items():
            t._heavy_view.rows = rows
            ms.append(once(lambda: t.record_heavy(1000 * (i + 1)))[1])
    rec = {}
    for name, (t, ms) in tasks.items():
        rec[name] = dict(spread(ms[args.retain + 1:]), first_intervals=spread(ms[1:args.retain + 1]), stats=t.heavy_history.stats())
    a, b = (tasks[k][0].heavy_history.heavy_hitters(2, limit=1000) for k in ("without_retain", f"retain_{args.retain}"))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "a folded window answers differently at the newest time"
    res["record_heavy"] = rec
    for t, _ in tasks.values():
        t.heavy_history.close()
    hist.close()
    return res


def main() -> int:
    args = parse_args()
    if args.child:
        print(json.dumps(child(args)), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--key-bytes", str(args.key_bytes), "--snapshots",
           str(args.snapshots), "--list-rows", str(args.list_rows), "--retain", str(args.retain), "--record-intervals",
           str(args.record_intervals), "--reps", str(args.reps), "--warmup", str(args.warmup), "--seed", str(args.seed),
           "--device", str(args.device)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s; stopping", file=sys.stderr)
        return 2
    if out.returncode != 0:
        print(f"exit {out.returncode}; stopping\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}", file=sys.stderr)
        return 2
    res = json.loads(out.stdout.strip().splitlines()[-1])
    rows = res["stats"]["rows"]
    print(json.dumps(res), flush=True)
    with open(os.path.join(args.out, f"heavy_history_lifecycle_{rows}.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
