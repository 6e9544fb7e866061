#!/usr/bin/env python3
"""Timings of the windowed all-candidates scan (pf_set_scan_window) at full size: one-query scans by
uid at top-10 over the seeded 1,632,803-user corpus, on bench.py's seed-2 query stream, timed with
pf_profile_reset / pf_profile_read (the scan kernel's device time, every launch) and with the host
clock around the synchronous calls.
  floors   no window, then a floor at the query's own 10th, 64th and 1,000th score (taken beforehand
           from an unwindowed topk = 1000 call, which is also timed: the alternative to a count);
  counts   the same three floors with PF_WIN_COUNT (theta held at the floor);
  pages    pages 1, 2, 10 and 100 at k = 64 (the cursors from one unwindowed topk = 6400 call).
Two child processes, because the engine reads PF_DEBUG once: the timings with no PF_DEBUG, and the
pruning counters (dropped share, blocks begun cold) under k5_prune_stats=1.  Reported, not gated.

    python tools/window_bench.py [--users N --steps K --out FILE --commit ID]

Reads nothing outside the repository; writes FILE (default profiles/window_bench.json)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommendation-system-pokec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TOPK = 10
RANKS = (10, 64, 1000)
PAGES = (1, 2, 10, 100)
PAGE_K = 64


def child(args):
    import synth
    import pokec_fas as pf
    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    eng = pf.FasEngine(corpus.desc_ptr(), 0)
    stats_on = "k5_prune_stats=1" in os.environ.get("PF_DEBUG", "")
    rng = np.random.default_rng(2)  # bench.py's cfg-2 query stream
    qs = [int(x) for x in rng.integers(1, args.users + 1, size=args.steps)]
    W = pf.ScanWindow.make
    # each query's own scores at ranks 10, 64 and 1,000: the job pipeline's topk = 1000 call
    eng.recommend_interest([qs[0]], RANKS[-1], pf.PF_MODE_ALL, 0)  # warm
    t = time.perf_counter()
    deep = [eng.recommend_interest([u], RANKS[-1], pf.PF_MODE_ALL, 0)[0] for u in qs]
    deep_ms = (time.perf_counter() - t) * 1e3 / len(qs)
    floors = {r: [float(sc[min(r, len(sc)) - 1]) if len(sc) else 0.0 for _, sc in deep] for r in RANKS}

    def timed(name, window_of, users=qs, k=TOPK):
        for u in users[:8]:
            eng.recommend_interest_all([u], k, window=window_of(u, 0))  # warm this instantiation
        if stats_on:
            eng.k5_prune_stats(reset=True)
        eng.profile_reset()
        got, totals = 0, 0
        t0 = time.perf_counter()
        for i, u in enumerate(users):
            w = window_of(u, i)
            got += len(eng.recommend_interest_all([u], k, window=w)[0][0])
            if w is not None and w.fields & pf.PF_WIN_COUNT:
                totals += int(eng.scan_window_totals()[0])
        host_ms = (time.perf_counter() - t0) * 1e3 / len(users)
        dev_ms, launches = eng.profile_read()
        row = {"case": name, "queries": len(users), "topk": k, "kernel_ms_per_scan": dev_ms / max(launches, 1), "launches": launches,
               "host_ms_per_call": host_ms, "results": got, "sum_of_totals": totals}
        if stats_on:
            st = eng.k5_prune_stats(reset=True)
            row["prune"] = st
            row["dropped_share"] = (st["dead_block_start"] + st["dead_round_end"]) / max(st["seen"], 1)
            row["cold_block_share"] = st["cold_blocks"] / max(st["blocks"], 1)
        return row

    rows = [timed("no window", lambda u, i: None)]
    for r in RANKS:
        rows.append(timed("floor at the query's %dth score" % r, lambda u, i, r=r: W(min_score=floors[r][i])))
    for r in RANKS:
        rows.append(timed("counted floor at the %dth score" % r, lambda u, i, r=r: W(min_score=floors[r][i], count=True)))
    # pages: the cursors of a few queries from one unwindowed deep call
    pq = qs[:args.page_queries]
    far = [eng.recommend_interest([u], PAGE_K * (PAGES[-1] - 1), pf.PF_MODE_ALL, 0)[0] for u in pq]
    for p in PAGES:
        def cursor(u, i, p=p):
            if p == 1:
                return None
            ids, sc = far[i]
            j = min(PAGE_K * (p - 1), len(ids)) - 1
            return W(after=(sc[j], int(ids[j])))
        rows.append(timed("page %d at k = %d" % (p, PAGE_K), cursor, users=pq, k=PAGE_K))
    out = {"pf_debug": os.environ.get("PF_DEBUG", ""), "scan_kernel": "K5" if eng.layout().scan_kernel == 2 else "K1",
           "users": args.users, "steps": args.steps, "topk1000_job_pipeline_host_ms_per_call": deep_ms, "rows": rows}
    eng.close()
    print("result " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--page-queries", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_bench.json"))
    ap.add_argument("--commit", default="unknown", help="the parent commit the tree was measured against")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for dbg in ("", "k5_prune_stats=1"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--users", str(args.users), "--steps", str(args.steps),
               "--page-queries", str(args.page_queries)]
        r = subprocess.run(cmd, env={**os.environ, "PF_DEBUG": dbg}, capture_output=True, text=True, timeout=1100)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("result ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            return 1
        runs.append(json.loads(line[0][7:]))
        print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "tools/window_bench.py", "parent_commit": args.commit,
           "what": "synchronous one-query scans by uid under score windows; kernel ms = pf_profile_read's summed device time "
                   "over its launches, host ms = wall clock per call; run 0 = timings, run 1 = pruning counters (k5_prune_stats=1)",
           "runs": runs}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
