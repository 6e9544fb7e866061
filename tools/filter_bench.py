#!/usr/bin/env python3
"""Timings of the filtered all-candidates scan (pf_set_scan_filter) at full size: one-query
scan_keys_async steps on a caller's stream, as bench.py's cfg 2 runs them, over the seeded
1,632,803-user corpus, with no filter and with filters that pass about 50 %, 5 % and 0.5 % of the
corpus (picked from the corpus's own gender / age distribution; the fraction each really passes is
reported with pf_scan_filter_count's figure).  Each setting runs in a child process of its own,
because the engine reads PF_DEBUG once: the default build of the path, and k5_filter_blockout=0
(blocks in which no candidate passes run to their end).  For the 0.5 % filter the first child also
times what a caller had to do before the filter existed: topk 4,096 through the job pipeline's
all-candidates jobs, then a filter on the host, and counts how often that gave the 10 the filtered
scan gives.  Reported, not gated.

    python tools/filter_bench.py [--users N --steps K --warmup W --out FILE --commit ID]

Reads nothing outside the repository; writes FILE (default profiles/k5f_filter_bench.json)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

TOPK = 10
WORKAROUND_TOPK = 4096


def np_pass(c, f):
    ok = np.ones(len(c.uid), bool)
    if f.fields & 1:
        ok &= (c.gen >= 0) & (c.gen == f.gender)
    if f.fields & 4:
        ok &= (c.age > 0) & (c.age >= f.age_min) & (c.age <= f.age_max)
    return ok


def pick_filters(pf, c):
    """Per target fraction the gender / age-window / gender-and-age-window filter passing closest to it."""
    n = len(c.uid)
    gvals = [int(g) for g in np.unique(c.gen[c.gen >= 0])]
    ages = c.age[c.age > 0]
    mode = int(np.bincount(ages).argmax())
    cands = [dict(gender=g) for g in gvals]
    for w in range(0, 64):
        for lo, hi in ((mode - w, mode + w), (mode, mode + w), (mode + 20, mode + 20 + w)):
            cands.append(dict(age=(max(1, lo), hi)))
            cands += [dict(gender=g, age=(max(1, lo), hi)) for g in gvals]
    fr = [(float(np_pass(c, pf.CandFilter.make(**kw)).sum()) / n, kw) for kw in cands]
    out = []
    for target in (0.5, 0.05, 0.005):
        frac, kw = min(fr, key=lambda x: abs(x[0] - target))
        out.append((f"{target * 100:g}%", kw, frac))
    return out


def child(args):
    import synth
    import torch
    import pokec_fas as pf
    import pokec_testlib as tl
    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    desc = corpus.desc_ptr()
    c = tl.corpus_from_desc(desc)
    eng = pf.FasEngine(desc, 0)
    kernel = eng.layout().scan_kernel
    rng = np.random.default_rng(2)  # bench.py's cfg-2 query stream
    qs = rng.integers(1, args.users + 1, size=(args.warmup + args.steps, 1)).astype(np.int32)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sptr = stream.cuda_stream
    keys = torch.empty((args.warmup + args.steps, TOPK), dtype=torch.int64, device="cuda")

    def timed(f):
        eng.set_scan_filter(f)
        count = eng.scan_filter_count()
        for i in range(args.warmup):
            eng.scan_keys_async(qs[i], TOPK, keys[i].data_ptr(), sptr)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(args.warmup, args.warmup + args.steps):
            eng.scan_keys_async(qs[i], TOPK, keys[i].data_ptr(), sptr)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3 / args.steps
        eng.clear_scan_filter()
        return ms, count

    rows = []
    ms, count = timed(None)
    rows.append({"filter": "none", "spec": None, "pass_fraction": 1.0, "pass_count": count, "ms_per_step": ms})
    picked = pick_filters(pf, c)
    for name, kw, frac in picked:
        ms, count = timed(pf.CandFilter.make(**kw))
        rows.append({"filter": name, "spec": {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()},
                     "pass_fraction": frac, "pass_count": count, "ms_per_step": ms})
    out = {"pf_debug": os.environ.get("PF_DEBUG", ""), "scan_kernel": "K5" if kernel == 2 else "K1", "users": args.users,
           "steps": args.steps, "warmup": args.warmup, "topk": TOPK, "rows": rows}
    if args.workaround:
        # today's workaround for the most selective filter: over-fetch through the job pipeline, filter on the host
        name, kw, frac = picked[-1]
        f = pf.CandFilter.make(**kw)
        mask = np_pass(c, f)
        pos = np.full(int(c.uid.max()) + 1, -1, np.int64)
        pos[c.uid] = np.arange(len(c.uid))
        n = args.workaround
        filt = [eng.recommend_interest_all([int(q[0])], TOPK, filter=f)[0] for q in qs[:n]]
        eng.recommend_interest([int(qs[0][0])], WORKAROUND_TOPK, pf.PF_MODE_ALL, 0)  # warm
        t = time.perf_counter()
        got = []
        for q in qs[:n]:
            ids, sc = eng.recommend_interest([int(q[0])], WORKAROUND_TOPK, pf.PF_MODE_ALL, 0)[0]
            m = mask[pos[ids]]
            got.append((ids[m][:TOPK], sc[m][:TOPK]))
        ms = (time.perf_counter() - t) * 1e3 / n
        agree = sum(1 for a, b in zip(got, filt) if list(a[0]) == list(b[0]) and
                    np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))
        short = sum(1 for a in got if len(a[0]) < TOPK)
        out["workaround"] = {"filter": name, "topk": WORKAROUND_TOPK, "queries": n, "ms_per_query": ms,
                             "lists_equal_to_filtered_scan": agree, "lists_short_of_topk": short,
                             "note": "synchronous pf_recommend_interest(PF_MODE_ALL, topk 4096) + numpy filter, per query"}
    eng.close()
    print("result " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workaround", type=int, default=0, help="(child) queries of the over-fetch workaround to time")
    ap.add_argument("--workaround-queries", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k5f_filter_bench.json"))
    ap.add_argument("--commit", default="unknown", help="the parent commit the tree was measured against")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for i, dbg in enumerate(("", "k5_filter_blockout=0")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--users", str(args.users), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--workaround", str(args.workaround_queries if i == 0 else 0)]
        r = subprocess.run(cmd, env={**os.environ, "PF_DEBUG": dbg}, capture_output=True, text=True, timeout=1100)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("result ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            return 1
        runs.append(json.loads(line[0][7:]))
        print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "tools/filter_bench.py", "parent_commit": args.commit,
           "what": "one-query scan_keys_async steps (cfg 2's step) under candidate filters; ms per step, host clock over "
                   "the timed steps; run 0 = the default path (whole-block early-out on), run 1 = k5_filter_blockout=0",
           "runs": runs}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
