#!/usr/bin/env python3
"""Timings of the group query (pf_recommend_group) at full size: the seeded 1,632,803-user corpus of
bench.py, MEAN, top-10, seeds = the first G uids of bench.py's seed-2 query stream, G = 1, 4, 16, 64
and 256.  In one process, per G:

  (a) the route without the group scan: G x fas_pairs(seed, every user), the sequential double sum
      and the sort on the host (calls the engine had before the group query: the baseline);
  (b) G one-query record-stream scans (set_scan_kernel(PF_SCAN_STREAM)), their last_scan_ms summed:
      the no-reuse floor, the record stream read G times;
  (c) recommend_group: wall clock, and device time by the HIP events around its launches
      (last_scan_ms), with group_plan's passes and bytes and the achieved stream bandwidth
      passes x stream bytes / device time.

Medians over --reps repetitions after a warm-up; (a) stops early once a G has run --a-seconds (never
below 3 repetitions; the count is recorded).  PF_DEBUG group_lds=BYTES (a pass's LDS budget) is read
once per process, so --only-c runs (c) alone for A/B runs under another budget.

    python tools/group_bench.py [--users N --reps R --out FILE --only-c --gs 16,64]

Reads nothing outside the repository; writes FILE (default profiles/group_bench.json; --only-c
prints its result line and writes nothing unless --out is given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK = 10
GS = (1, 4, 16, 64, 256)


def median(x):
    return float(np.median(np.asarray(x, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--a-seconds", type=float, default=45.0, help="time after which route (a) stops repeating one G")
    ap.add_argument("--only-c", action="store_true")
    ap.add_argument("--gs", default=",".join(str(g) for g in GS), help="the group sizes, comma-separated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "recommendation-system-pokec_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    import pokec_fas as pf
    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    eng = pf.FasEngine(corpus.desc_ptr(), 0)
    rng = np.random.default_rng(2)  # bench.py's cfg-2 query stream
    stream = rng.integers(1, args.users + 1, size=(max(max(GS), max(int(g) for g in args.gs.split(","))), 1)).astype(np.int32)[:, 0]
    all_u = np.arange(1, args.users + 1, dtype=np.int32)
    lay = eng.layout()
    rows = []
    gs = [int(g) for g in args.gs.split(",")]
    for G in gs:
        seeds = [int(u) for u in stream[:G]]
        plan = eng.group_plan(seeds)
        row = {"G": G, "kept_seeds": plan.n_seeds, "passes": plan.n_passes, "global_images": plan.n_global,
               "stream_bytes": int(plan.stream_bytes)}
        # (c)
        ids_c, sc_c = eng.recommend_group(seeds, TOPK)
        wall, dev = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eng.recommend_group(seeds, TOPK)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(eng.last_scan_ms)
        row["c_wall_ms"], row["c_device_ms"] = median(wall), median(dev)
        row["c_stream_GBps"] = plan.stream_bytes / (row["c_device_ms"] * 1e-3) / 1e9
        if not args.only_c:
            # (b)
            eng.set_scan_kernel(pf.PF_SCAN_STREAM)
            tot = []
            for r in range(args.reps + 1):
                ms = 0.0
                for u in seeds:
                    eng.recommend_interest_all([u], TOPK)
                    ms += eng.last_scan_ms
                if r:
                    tot.append(ms)
            eng.set_scan_kernel(pf.PF_SCAN_AUTO)
            row["b_device_ms"] = median(tot)
            row["b_over_c"] = row["b_device_ms"] / row["c_device_ms"]
            # (a)
            kept = list(dict.fromkeys(seeds))
            wall, ids_a, t_begin = [], None, time.perf_counter()
            for r in range(args.reps + 1):
                t0 = time.perf_counter()
                acc = np.zeros(len(all_u), np.float64)
                for u in kept:
                    acc += eng.fas_pairs(np.full(len(all_u), u, np.int32), all_u).astype(np.float64)
                sc = (acc / np.float64(len(kept))).astype(np.float32)
                sc[np.asarray(kept) - 1] = -np.inf
                top = np.argpartition(-sc, TOPK)[:TOPK]
                top = top[np.lexsort((all_u[top], -sc[top].astype(np.float64)))]
                dt = (time.perf_counter() - t0) * 1e3
                if r:
                    wall.append(dt)
                ids_a, sc_a = all_u[top], sc[top]
                if len(wall) >= 3 and time.perf_counter() - t_begin > args.a_seconds:
                    break
            row["a_wall_ms"], row["a_reps"] = median(wall), len(wall)
            row["a_over_c"] = row["a_wall_ms"] / row["c_wall_ms"]
            row["a_equals_c"] = bool(list(ids_a) == list(ids_c) and
                                     np.array_equal(sc_a.view(np.uint32), np.asarray(sc_c, np.float32).view(np.uint32)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    _, fixed, budget = eng.group_image_lds([int(stream[0])])
    res = {"tool": "tools/group_bench.py", "users": args.users, "topk": TOPK, "agg": "mean", "reps": args.reps,
           "debug": os.environ.get("PF_DEBUG", ""), "lds_budget": budget, "lds_fixed": fixed,
           "layout_stream_bytes": int(lay.stream_bytes), "layout_header_bytes": int(lay.header_bytes),
           "what": "a = G x fas_pairs over every user + host sum + sort (wall ms); b = G one-query record-stream scans "
                   "(summed device ms); c = recommend_group (wall ms, device ms by HIP events around its launches)",
           "rows": rows}
    eng.close()
    print("result " + json.dumps(res), flush=True)
    out = args.out or (None if args.only_c else os.path.join(ROOT, "profiles", "group_bench.json"))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
