#!/usr/bin/env python3
"""What a query by profile costs at full size, next to the by-uid query it stands in for.

On the seeded 1,632,803-user corpus (bench.py's), for a sample of stored users, top-10:
  by_uid      recommend_interest_all([u], 10): one launch from the user's resident image
  adhoc_one   the same user as a QueryProfile copy (exclude = adj[u] + {u}), nq = 1: the image is
              built on the host and uploaded with the launch (the stale-image path's route)
  adhoc_batch 256 such copies in one call: the batch scan over the staged images
Each call's wall time (a host clock around a call that ends in a stream synchronise) is reported next
to pf_last_scan_ms (device events around the scan kernel); their difference is the host side of the
call: argument checks, the image build, the upload, the launch, the wait, the key copy and decode.
By-uid calls have no image build and no image upload, so adhoc_one's host side minus by_uid's is what
building and uploading the image adds per query.  The clone's results are compared with the by-uid
call's before anything is timed.  Reported, not gated.

    python tools/profile_query_timing.py [--users N --queries Q --warmup W --out FILE]

Reads nothing outside the repository; writes FILE (default profiles/qprof_timing.json).  Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK = 10
BATCH = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qprof_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "recommendation-system-pokec_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    import pokec_fas as pf
    import pokec_testlib as tl

    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    desc = corpus.desc_ptr()
    d = tl.PfCorpusDesc.from_address(desc)
    n, T = d.n_users, d.n_cols

    def view(p, ct, count):
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape=(max(count, 1),))
    i32, i64, u32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
    uid = view(d.user_id, i32, n)
    pub, comp, gen, age = (view(p, i32, n) for p in (d.public_flag, d.completion, d.gender, d.age))
    reg = view(d.region, i32, 3 * n)
    co, fo, to = view(d.club_off, i64, n + 1), view(d.friend_off, i64, n + 1), view(d.tok_off, i64, n * T + 1)
    clubs, friends = view(d.club_ids, u32, int(co[n])), view(d.friend_ids, u32, int(fo[n]))
    tid, tf = view(d.tok_tid, i32, int(to[n * T])), view(d.tok_tf, i32, int(to[n * T]))
    adj_uid, ao = view(d.adj_uid, i32, d.n_adj), view(d.adj_off, i64, d.n_adj + 1)
    adj_nbr = view(d.adj_nbr, i32, int(ao[d.n_adj]))
    adj_row = {int(u): j for j, u in enumerate(adj_uid[:d.n_adj])}
    where = {int(u): i for i, u in enumerate(uid)}

    def clone(u):
        i = where[u]
        j = adj_row.get(u)
        excl = ([int(x) for x in adj_nbr[ao[j]:ao[j + 1]]] if j is not None else []) + [u]
        toks = {t: list(zip(tid[to[i * T + t]:to[i * T + t + 1]].tolist(), tf[to[i * T + t]:to[i * T + t + 1]].tolist()))
                for t in range(T) if to[i * T + t + 1] > to[i * T + t]}
        return pf.QueryProfile.make(public_flag=None if pub[i] < 0 else int(pub[i]), gender=None if gen[i] < 0 else int(gen[i]),
                                    completion=int(comp[i]) if comp[i] > 0 else None, age=int(age[i]) if age[i] > 0 else None,
                                    region=[None if x < 0 else int(x) for x in reg[3 * i:3 * i + 3]],
                                    clubs=clubs[co[i]:co[i + 1]].tolist(), friends=friends[fo[i]:fo[i + 1]].tolist(),
                                    tokens=toks, exclude=excl, n_cols=T)

    t0 = time.perf_counter()
    eng = pf.FasEngine(desc, 0)
    open_s = time.perf_counter() - t0
    rng = np.random.default_rng(2)  # bench.py's cfg-2 query stream
    total = args.warmup + args.queries
    qs = [int(u) for u in rng.integers(1, args.users + 1, size=max(total, BATCH))]
    profs = [clone(u) for u in qs]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for u, p in list(zip(qs, profs))[:8]:  # the clone is the by-uid query
        a, b = eng.recommend_interest_all([u], TOPK)[0], eng.recommend_profile(p, TOPK)[0]
        assert list(a[0]) == list(b[0]) and np.array_equal(bits(a[1]), bits(b[1])), u

    def timed(call, items):
        for x in items[:args.warmup]:
            call(x)
        wall, dev = [], []
        for x in items[args.warmup:]:
            t = time.perf_counter()
            call(x)   # ends in a stream synchronise (the keys are copied back and decoded)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(float(eng.last_scan_ms))
        wall, dev = np.array(wall), np.array(dev)
        return {"calls": len(wall), "wall_ms_median": float(np.median(wall)), "wall_ms_mean": float(wall.mean()),
                "wall_ms_p90": float(np.percentile(wall, 90)), "scan_ms_median": float(np.median(dev)),
                "scan_ms_mean": float(dev.mean()), "host_ms_median": float(np.median(wall - dev)),
                "host_ms_mean": float((wall - dev).mean())}

    rows = {}
    for rnd in range(2):  # the two forms in alternation, twice: the spread shows in the rows
        rows["by_uid_%d" % rnd] = timed(lambda u: eng.recommend_interest_all([u], TOPK), qs[:total])
        rows["adhoc_one_%d" % rnd] = timed(lambda p: eng.recommend_profile(p, TOPK), profs[:total])
    batch = profs[:BATCH]
    reps = [batch] * (args.warmup // 10 + 1 + 10)
    saved = args.warmup
    args.warmup = args.warmup // 10 + 1
    rows["adhoc_batch_256"] = timed(lambda b: eng.recommend_profile(b, TOPK), reps)
    rows["by_uid_batch_256"] = timed(lambda b: eng.recommend_interest_all(b, TOPK), [qs[:BATCH]] * len(reps))
    args.warmup = saved
    for k in ("adhoc_batch_256", "by_uid_batch_256"):
        rows[k]["wall_ms_per_query"] = rows[k]["wall_ms_median"] / BATCH
    extra = [rows["adhoc_one_%d" % r]["host_ms_median"] - rows["by_uid_%d" % r]["host_ms_median"] for r in range(2)]
    out = {"tool": "tools/profile_query_timing.py", "users": args.users, "topk": TOPK, "queries": args.queries,
           "warmup": saved, "pf_open_s": open_s, "scan_kernel": "K5" if eng.layout().scan_kernel == 2 else "K1",
           "what": "ms per call; wall = host clock around a synchronous call; scan = pf_last_scan_ms (device events around "
                   "the scan kernel; a batch's first launch to its last); host = wall - scan",
           "adhoc_one_extra_host_ms": extra, "rows": rows}
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
