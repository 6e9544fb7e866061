#!/usr/bin/env python3
"""What diverse top-k costs at full size (pf_recommend_diverse_interest / _profile / _group): queries over
the seeded 1,632,803-user corpus on bench.py's seed-2 query stream, and one group of 16 seeds, at
(pool, topk) = (100, 10), (200, 20) and (1024, 64), under a floor at each query's own 10,000th score (a
collector of 65,536 keys).

Per case and variant, host clock of the whole call:
  call      eng.recommend_diverse_*(..., k, lam=0.7, pool=M, window=floor);
  scan      the collecting scan call alone (recommend_interest_all(..., collect=cap) and its profile / group
            forms: scan, count copy, sort, key copy): what the call runs underneath;
  matrix    eng.diverse_rerank of the pool with topk = 1: the M x M matrix (M image builds, one pair launch,
            the scores copied back) and a stage of one pick;
  rerank    eng.diverse_rerank of the pool with the case's topk (the matrix and the stage, no scan);
            rerank - matrix is the stage's remaining picks (tools/probe/diverse sweep times the stage alone);
  host      the same list assembled the way a caller had to before: that collecting call, scan_collected(),
            then topk sequential eng.fas_pairs(picked, pool) calls inside the numpy loop of the definition.
            Its list is compared with the call's: ids, float32 bits, float64 bits.
Each figure is the median over the queries after three warm-up calls, the variants alternating per query;
min and max are reported beside it.  Reported, not gated.

    python tools/diverse_bench.py [--users N --steps K --out FILE --commit ID]

Reads nothing outside the repository; writes FILE (default profiles/diverse_bench.json)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommendation-system-pokec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((100, 10), (200, 20), (1024, 64))
LAM = 0.7
CAP = 65536
f32, f64 = np.float32, np.float64


def host_diverse(eng, ids, sc, pool, k, lam):
    """The definition through the public API as it stood: k sequential pair calls, one per pick."""
    m = min(pool, len(ids))
    u, r = np.ascontiguousarray(ids[:m], np.int32), np.asarray(sc[:m], f32)
    pen, picked = np.zeros(m, f32), np.zeros(m, bool)
    dl = f64(f32(lam))
    om = f64(1.0) - dl
    a = dl * r.astype(f64)
    out = []
    for _ in range(min(k, m)):
        p = om * pen.astype(f64)
        v = a - p
        v[picked] = -np.inf
        s = int(np.argmax(v))  # the first of the equals
        out.append((int(u[s]), r[s], pen[s], v[s]))
        picked[s] = True
        row = eng.fas_pairs(np.full(m, u[s], np.int32), u)
        pen = np.where(row > pen, row, pen).astype(f32)
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], f32), np.array([o[2] for o in out], f32),
            np.array([o[3] for o in out], f64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_bench.json"))
    ap.add_argument("--commit", default="unknown", help="the commit measured")
    args = ap.parse_args()
    import synth
    import pokec_fas as pf
    import pokec_testlib as tl
    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    ptr = corpus.desc_ptr()
    d = tl.PfCorpusDesc.from_address(ptr)
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

    def clone(u):  # the by-uid query as a profile given by value
        i = int(np.searchsorted(uid[:n], u))
        j = adj_row.get(u)
        excl = ([int(x) for x in adj_nbr[ao[j]:ao[j + 1]]] if j is not None else []) + [u]
        toks = {t: list(zip(tid[to[i * T + t]:to[i * T + t + 1]].tolist(), tf[to[i * T + t]:to[i * T + t + 1]].tolist()))
                for t in range(T) if to[i * T + t + 1] > to[i * T + t]}
        return pf.QueryProfile.make(public_flag=None if pub[i] < 0 else int(pub[i]), gender=None if gen[i] < 0 else int(gen[i]),
                                    completion=int(comp[i]) if comp[i] > 0 else None, age=int(age[i]) if age[i] > 0 else None,
                                    region=[None if x < 0 else int(x) for x in reg[3 * i:3 * i + 3]],
                                    clubs=clubs[co[i]:co[i + 1]].tolist(), friends=friends[fo[i]:fo[i + 1]].tolist(),
                                    tokens=toks, exclude=excl, n_cols=T)

    eng = pf.FasEngine(ptr, 0)
    rng = np.random.default_rng(2)  # bench.py's cfg-2 query stream
    qs = [int(x) for x in rng.integers(1, args.users + 1, size=args.steps)]
    W = pf.ScanWindow.make
    floors = []
    for u in qs:
        eng.recommend_interest_all([u], 10, collect=args.users)
        sc = eng.scan_collected()[1]
        floors.append(float(sc[min(10000, len(sc)) - 1]))
    profs = [clone(u) for u in qs]
    seeds = qs[:16]
    eng.recommend_group(seeds, 1, "mean", collect=args.users)
    gsc = eng.scan_collected()[1]
    gfloor = float(gsc[min(10000, len(gsc)) - 1])
    rows = []

    def case(name, items, pool, k, call, scan):
        """items: per step (query, window); the variants alternate per step."""
        t = {x: [] for x in ("call", "scan", "matrix", "rerank", "host")}
        totals, mismatches = [], 0
        for q, w in items[:3]:  # warm-up
            call(q, w)
            scan(q, w)

        def clock(key, fn):
            t0 = time.perf_counter()
            res = fn()
            t[key].append((time.perf_counter() - t0) * 1e3)
            return res
        for q, w in items:
            got = clock("call", lambda: call(q, w))
            clock("scan", lambda: scan(q, w))

            def host():
                scan(q, w)
                ids, sc, total = eng.scan_collected()
                return host_diverse(eng, ids, sc, pool, k, LAM), ids, sc, total
            ref, ids, sc, total = clock("host", host)
            m = min(pool, len(ids))
            pu = np.ascontiguousarray(ids[:m], np.int32)
            clock("matrix", lambda: eng.diverse_rerank(pu, sc[:m], 1, LAM))
            clock("rerank", lambda: eng.diverse_rerank(pu, sc[:m], k, LAM))
            totals.append(int(total))
            same = (list(got[0]) == list(ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)) and
                    np.array_equal(got[2]["pen"].view(np.uint32), ref[2].view(np.uint32)) and
                    np.array_equal(got[2]["value"].view(np.uint64), ref[3].view(np.uint64)))
            mismatches += not same

        def stat(v):
            return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        row = {"case": name, "pool": pool, "topk": k, "steps": len(items), "window_median": float(np.median(totals)),
               "call_ms": stat(t["call"]), "scan_ms": stat(t["scan"]), "matrix_ms": stat(t["matrix"]), "rerank_ms": stat(t["rerank"]),
               "host_loop_ms": stat(t["host"]), "lists_differing_from_host": mismatches}
        rows.append(row)
        print(json.dumps(row), flush=True)

    for pool, k in SHAPES:
        case("by uid", [(u, W(min_score=floors[i])) for i, u in enumerate(qs)], pool, k,
             lambda u, w: eng.recommend_diverse_interest(u, k, lam=LAM, pool=pool, window=w, cap=CAP),
             lambda u, w: eng.recommend_interest_all([u], 1, window=w, collect=CAP))
        case("by profile", [(p, W(min_score=floors[i])) for i, p in enumerate(profs)], pool, k,
             lambda p, w: eng.recommend_diverse_profile(p, k, lam=LAM, pool=pool, window=w, cap=CAP),
             lambda p, w: eng.recommend_profile(p, 1, window=w, collect=CAP))
        case("group G = 16", [(0, W(min_score=gfloor))] * max(6, args.steps // 2), pool, k,
             lambda _, w: eng.recommend_diverse_group(seeds, k, "mean", lam=LAM, pool=pool, window=w, cap=CAP),
             lambda _, w: eng.recommend_group(seeds, 1, "mean", window=w, collect=CAP))
    out = {"commit": args.commit, "users": args.users, "queries": qs, "lambda": LAM, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
