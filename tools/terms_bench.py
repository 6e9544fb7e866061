#!/usr/bin/env python3
"""Timings of the FAS score breakdown at full size, over the benchmark's seeded 1,632,803-user
corpus:

  pairs    pf_fas_pairs_terms against pf_fas_pairs on the same seeded pairs, n = 10, 100, 10^4 and
           10^6 (whole calls: grouping by query, image building, upload, the kernel, the copy back
           and the scatter into the caller's arrays);
  explain  recommend_interest_all with and without explain=True at k = 10 (the scan kernels) and
           k = 100 (the job pipeline), one query per call.

Every figure is the median of repeated calls after warm-up calls of the same shape, on a host clock
around calls that end in a stream synchronise; the two sides of a comparison alternate.  explain=True
costs one more launch and one more copy by construction: the row "extra_ms" is what that costs.
Reported, not gated.

    python tools/terms_bench.py [--users N --repeats R --warmup W --queries Q --out FILE --commit ID]

Reads nothing outside the repository; writes FILE (default profiles/terms_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommendation-system-pokec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PAIR_SIZES = (10, 100, 10**4, 10**6)
TOPKS = (10, 100)


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=40, help="queries of each explain setting (one call each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terms_bench.json"))
    ap.add_argument("--commit", default="unknown", help="the parent commit the tree was measured against")
    args = ap.parse_args()
    import synth
    import pokec_fas as pf
    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    eng = pf.FasEngine(corpus.desc_ptr(), 0)
    T = eng.num_cols
    rows = []
    rng = np.random.default_rng(5)
    for n in PAIR_SIZES:
        a = rng.integers(1, args.users + 1, n).astype(np.int32)
        b = rng.integers(1, args.users + 1, n).astype(np.int32)
        reps = args.repeats if n < 10**6 else max(3, args.repeats // 2)
        for _ in range(args.warmup):
            eng.fas_pairs(a, b)
            eng.fas_pairs_terms(a, b)
        plain, terms = [], []
        for _ in range(reps):  # alternating
            plain.append(timed(lambda: eng.fas_pairs(a, b)))
            terms.append(timed(lambda: eng.fas_pairs_terms(a, b)))
        pt = eng.fas_pairs_terms(a, b)
        same = bool(np.array_equal(pt.score.view(np.uint32), eng.fas_pairs(a, b).view(np.uint32)))
        rows.append({"what": "pairs", "n": n, "distinct_queries": int(len(np.unique(a))), "fas_pairs": spread(plain),
                     "fas_pairs_terms": spread(terms), "ratio_of_medians": float(np.median(terms) / np.median(plain)),
                     "output_bytes_plain": 4 * n, "output_bytes_terms": n * (16 + 8 * (7 + T)),
                     "scores_bit_equal": same, "mean_used": float(pt.used.mean())})
        print(json.dumps(rows[-1]), flush=True)
    qs = np.random.default_rng(2).integers(1, args.users + 1, args.warmup + args.queries).astype(np.int32)  # bench.py's cfg-2 stream
    for k in TOPKS:
        for q in qs[:args.warmup]:
            eng.recommend_interest_all([int(q)], k)
            eng.recommend_interest_all([int(q)], k, explain=True)
        plain, expl, same = [], [], True
        for q in qs[args.warmup:]:  # alternating
            r = {}
            plain.append(timed(lambda: r.setdefault("p", eng.recommend_interest_all([int(q)], k)[0])))
            expl.append(timed(lambda: r.setdefault("e", eng.recommend_interest_all([int(q)], k, explain=True)[0])))
            same = same and list(r["p"][0]) == list(r["e"][0]) and np.array_equal(r["p"][1].view(np.uint32), r["e"][1].view(np.uint32))
        rows.append({"what": "explain", "topk": k, "path": "scan kernel" if k <= pf.MAX_TOPK_DEVICE else "job pipeline",
                     "explain_false": spread(plain), "explain_true": spread(expl),
                     "extra_ms": float(np.median(expl) - np.median(plain)), "lists_bit_equal": bool(same)})
        print(json.dumps(rows[-1]), flush=True)
    kernel = eng.layout().scan_kernel
    eng.close()
    res = {"tool": "tools/terms_bench.py", "parent_commit": args.commit, "users": args.users, "n_cols": T,
           "scan_kernel": "K5" if kernel == 2 else "K1", "warmup_calls": args.warmup,
           "what": "whole-call host-clock times (ms) of the score breakdown against the calls it extends; medians of "
                   "alternating repeated calls after warm-up",
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
