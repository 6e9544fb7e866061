#!/usr/bin/env python3
"""What collecting a score window costs (pf_set_scan_collect) at full size: one-query scans by uid over
the seeded 1,632,803-user corpus on bench.py's seed-2 query stream, and one group of 16 seeds.
  floors   at each query's own 64th, 1,000th, 10,000th and 100,000th score, taken from one deep call
           per query: a collecting call with no window (everybody, ranked).  A tree without the
           collector reads them from the file the other run wrote (--floors);
  counted  a counted scan at each floor: the scan kernel's device time (pf_profile_read) and the host
           clock per call.  Run on the parent too (--parent: only what the parent has), the difference
           in kernel time is the price of the append;
  collect  the same scan with a collector of the exact size: the kernel's time, the host clock of the
           whole call (scan, count copy, sort, list copy) and of scan_collected (the decode); the sort's
           device time is the call's host time minus the counted call's, less the copy (reported as
           finish_ms_per_call, host clock: the sort runs on the context's stream between two
           synchronisations of the call);
  pages    pages(call, 64) to the same depth: what a collect replaces;
  group    recommend_group at G = 16, a floor at the aggregate's 10,000th score (from pages of 64 read
           once), counted, collected and paged.
Reported, not gated.

    python tools/collect_bench.py [--users N --steps K --out FILE --commit ID] [--floors FILE [--parent]]

Reads nothing outside the repository; writes FILE (default profiles/collect_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommendation-system-pokec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RANKS = (64, 1000, 10000, 100000)
PAGE_K = 64
GROUP_RANK = 10000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--page-queries", type=int, default=4, help="queries paged to each depth (a deep one is thousands of scans)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect_bench.json"))
    ap.add_argument("--commit", default="unknown", help="the commit measured")
    ap.add_argument("--floors", default=None, help="the floors' file: written by a full run, read by a --parent run")
    ap.add_argument("--parent", action="store_true", help="a tree without the collector: counted scans and pages only")
    args = ap.parse_args()
    import synth
    import pokec_fas as pf
    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    eng = pf.FasEngine(corpus.desc_ptr(), 0)
    rng = np.random.default_rng(2)  # bench.py's cfg-2 query stream
    qs = [int(x) for x in rng.integers(1, args.users + 1, size=args.steps)]
    W = pf.ScanWindow.make
    if args.parent:
        with open(args.floors) as f:
            saved = json.load(f)
        assert saved["queries"] == qs, "the floors' file is another query stream's"
        floors, deep_ms = {int(r): v for r, v in saved["floors"].items()}, None
    else:
        floors = {r: [] for r in RANKS}
        eng.recommend_interest_all([qs[0]], 10, collect=args.users)  # warm
        t = time.perf_counter()
        for u in qs:
            eng.recommend_interest_all([u], 10, collect=args.users)
            sc = eng.scan_collected()[1]
            for r in RANKS:
                floors[r].append(float(sc[min(r, len(sc)) - 1]))
        deep_ms = (time.perf_counter() - t) * 1e3 / len(qs)
        if args.floors:
            with open(args.floors, "w") as f:
                json.dump({"queries": qs, "floors": floors}, f)
    rows = []

    def timed(name, fn, users, after=None):
        """fn(i, u) makes one call; after(i, u) (untimed in host_ms, timed apart) reads its result."""
        for i, u in enumerate(users[:3]):
            fn(i, u)
        eng.profile_reset()
        t0 = time.perf_counter()
        n_out = 0
        read_s = 0.0
        for i, u in enumerate(users):
            fn(i, u)
            if after is not None:
                t1 = time.perf_counter()
                n_out += after(i, u)
                read_s += time.perf_counter() - t1
        host_ms = ((time.perf_counter() - t0) - read_s) * 1e3 / len(users)
        dev_ms, launches = eng.profile_read()
        row = {"case": name, "queries": len(users), "kernel_ms_per_scan": dev_ms / max(launches, 1), "launches": launches,
               "host_ms_per_call": host_ms, "read_ms_per_call": read_s * 1e3 / len(users), "entries": n_out}
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    for r in RANKS:
        c = timed("counted floor at the %dth score" % r, lambda i, u, r=r: eng.recommend_interest_all([u], 10, window=W(min_score=floors[r][i], count=True)),
                  qs, after=lambda i, u: int(eng.scan_window_totals()[0]))
        if not args.parent:
            totals = []
            k = timed("collected floor at the %dth score" % r,
                      lambda i, u, r=r: eng.recommend_interest_all([u], 10, window=W(min_score=floors[r][i]), collect=max(r * 2, 1024)),
                      qs, after=lambda i, u: totals.append(eng.scan_collected()[2]) or totals[-1])
            k["finish_ms_per_call"] = k["host_ms_per_call"] - c["host_ms_per_call"]
            k["append_kernel_ms"] = k["kernel_ms_per_scan"] - c["kernel_ms_per_scan"]
            k["overflows"] = sum(1 for x in totals if x > max(r * 2, 1024))
        pq = qs[:args.page_queries]

        def page_all(i, u, r=r):
            n = 0
            for ids, _ in pf.pages(lambda k_, w: eng.recommend_interest_all([u], k_, window=w)[0], PAGE_K, W(min_score=floors[r][i])):
                n += len(ids)
            page_all.n = n
        p = timed("pages of %d to the %dth score" % (PAGE_K, r), page_all, pq if r > 1000 else qs, after=lambda i, u: page_all.n)
        p["host_ms_per_call"] = p["host_ms_per_call"]  # (per query: every page of it)

    # a group of 16 seeds: the floor at its 10,000th aggregate score, read once by paging
    seeds = qs[:16]
    got = 0
    floor_g = 0.0
    t = time.perf_counter()
    for ids, sc in pf.pages(lambda k_, w: eng.recommend_group(seeds, k_, "mean", window=w), PAGE_K):
        got += len(ids)
        floor_g = float(sc[-1])
        if got >= GROUP_RANK:
            break
    paged_ms = (time.perf_counter() - t) * 1e3
    rows.append({"case": "group G = 16: pages of %d to rank %d" % (PAGE_K, got), "host_ms_total": paged_ms, "pages": (got + PAGE_K - 1) // PAGE_K,
                 "host_ms_per_page": paged_ms / max(1, (got + PAGE_K - 1) // PAGE_K)})
    print(json.dumps(rows[-1]), flush=True)
    g5 = [0] * 5
    c = timed("group G = 16: counted floor at rank %d" % got, lambda i, u: eng.recommend_group(seeds, 10, "mean", window=W(min_score=floor_g, count=True)),
              g5, after=lambda i, u: int(eng.scan_window_totals()[0]))
    if not args.parent:
        k = timed("group G = 16: collected floor at rank %d" % got,
                  lambda i, u: eng.recommend_group(seeds, 10, "mean", window=W(min_score=floor_g), collect=4 * GROUP_RANK),
                  g5, after=lambda i, u: eng.scan_collected()[2])
        k["finish_ms_per_call"] = k["host_ms_per_call"] - c["host_ms_per_call"]
        k["append_kernel_ms"] = k["kernel_ms_per_scan"] - c["kernel_ms_per_scan"]
    res = {"tool": "tools/collect_bench.py", "commit": args.commit, "parent_tree": bool(args.parent),
           "scan_kernel": "K5" if eng.layout().scan_kernel == 2 else "K1", "users": args.users, "steps": args.steps,
           "collect_everybody_host_ms_per_call": deep_ms,
           "what": "kernel ms = pf_profile_read's summed device time over its launches; host ms = wall clock per call without "
                   "reading the result; read ms = scan_window_totals / scan_collected (decode and copy) per call; pages rows: "
                   "host ms per query for all its pages", "rows": rows}
    eng.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
