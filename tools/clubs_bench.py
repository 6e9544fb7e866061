#!/usr/bin/env python3
"""What clubs by interest costs at full size (pf_recommend_clubs_interest / _group): by-uid queries over
the seeded 1,632,803-user corpus on bench.py's seed-2 query stream, and one group of 16 seeds.

Per case (a floor at each query's own 100th / 10,000th score, read from one deep collecting call):
  call      eng.recommend_clubs_interest(u, 10, window=floor): host clock of the whole call;
  collect   the collecting scan call alone (recommend_interest_all(..., collect=cap): scan, count copy, sort,
            key copy): what the club call runs underneath.  call - collect = the stage (own bitmap, count,
            place, emit, sort, sum, rank and its three synchronisations), host clock;
  host      the same answer assembled the way a caller had to before: that collecting call, scan_collected()
            and a host loop over the dataset's club lists (numpy: a CSR gather and np.add.at, which adds in
            index order, so the sums are the definition's), then a sort of the clubs.  Its list is compared
            with the call's, bit for bit.
Each case is the median over the queries after three warm-up calls, alternating the three variants per
query; min and max are reported beside it.  Reported, not gated.

    python tools/clubs_bench.py [--users N --steps K --out FILE --commit ID]

Reads nothing outside the repository; writes FILE (default profiles/clubs_bench.json)."""
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

RANKS = (100, 10000)


class Desc(ctypes.Structure):  # the head of pf_corpus_desc (include/pokec_fas.h), up to the club arrays
    P = ctypes.c_void_p
    _fields_ = [("n_users", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("user_id", P), ("public_flag", P), ("completion", P),
                ("gender", P), ("age", P), ("region", P), ("club_off", P), ("club_ids", P)]


def club_csr(ptr):
    d = Desc.from_address(ptr)
    n = d.n_users
    uid = np.ctypeslib.as_array(ctypes.cast(d.user_id, ctypes.POINTER(ctypes.c_int32)), shape=(n,)).copy()
    off = np.ctypeslib.as_array(ctypes.cast(d.club_off, ctypes.POINTER(ctypes.c_int64)), shape=(n + 1,)).copy()
    ids = np.ctypeslib.as_array(ctypes.cast(d.club_ids, ctypes.POINTER(ctypes.c_uint32)), shape=(int(off[-1]),)).copy()
    return uid, off, ids.astype(np.int64)


def host_clubs(uid, off, clubs, ids, sc, own, topk):
    """The definition on the host from a collected ranking: (club ids, float32 scores)."""
    keep = sc > 0
    idx = np.searchsorted(uid, ids[keep])
    w = sc[keep].astype(np.float64)
    lens = off[idx + 1] - off[idx]
    if int(lens.sum()) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    # every neighbour's club range, in rank order and profile order
    starts = np.repeat(off[idx], lens)
    within = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    cl = clubs[starts + within]
    ww = np.repeat(w, lens)
    m = ~np.isin(cl, own)
    cl, ww = cl[m], ww[m]
    uniq, inv = np.unique(cl, return_inverse=True)
    acc = np.zeros(len(uniq), np.float64)
    np.add.at(acc, inv, ww)  # unbuffered: one add after the other, in index (= rank) order
    s32 = acc.astype(np.float32)
    order = np.lexsort((uniq, -s32.astype(np.float64)))[:topk]
    return uniq[order], s32[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clubs_bench.json"))
    ap.add_argument("--commit", default="unknown", help="the commit measured")
    args = ap.parse_args()
    import synth
    import pokec_fas as pf
    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    ptr = corpus.desc_ptr()
    uid, off, clubs = club_csr(ptr)
    eng = pf.FasEngine(ptr, 0)
    rng = np.random.default_rng(2)  # bench.py's cfg-2 query stream
    qs = [int(x) for x in rng.integers(1, args.users + 1, size=args.steps)]
    W = pf.ScanWindow.make
    floors = {r: [] for r in RANKS}
    for u in qs:
        eng.recommend_interest_all([u], 10, collect=args.users)
        sc = eng.scan_collected()[1]
        for r in RANKS:
            floors[r].append(float(sc[min(r, len(sc)) - 1]))
    rows = []

    def own_of(users):
        idx = np.searchsorted(uid, np.asarray(users))
        return np.unique(np.concatenate([clubs[off[i]:off[i + 1]] for i in idx] + [np.zeros(0, np.int64)]))

    def case(name, items, club_call, collect_call, own_users):
        """items: per step the window; the three variants alternate per step."""
        t_call, t_coll, t_host, neighbours, contribs, mismatches = [], [], [], [], [], 0
        for i, (u, w) in enumerate(items[:3]):  # warm-up
            club_call(u, w)
            collect_call(u, w)
        for i, (u, w) in enumerate(items):
            t = time.perf_counter()
            got = club_call(u, w)
            t_call.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            collect_call(u, w)
            t_coll.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            collect_call(u, w)
            ids, sc, total = eng.scan_collected()
            ref = host_clubs(uid, off, clubs, ids, sc, own_of(own_users(u)), 10)
            t_host.append((time.perf_counter() - t) * 1e3)
            neighbours.append(int(total))
            contribs.append(int(got[2]["contributions"]))
            if list(got[0]) != [int(x) for x in ref[0]] or not np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)):
                mismatches += 1

        def stat(v):
            return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        stage = [a - b for a, b in zip(t_call, t_coll)]
        row = {"case": name, "steps": len(items), "neighbours_median": float(np.median(neighbours)),
               "contributions_median": float(np.median(contribs)), "call_ms": stat(t_call), "collect_call_ms": stat(t_coll),
               "stage_ms": stat(stage), "host_assembly_ms": stat(t_host), "lists_differing_from_host": mismatches}
        rows.append(row)
        print(json.dumps(row), flush=True)

    for r in RANKS:
        cap = max(4 * r, 1024)
        case("by uid, floor at the %dth score" % r, [(u, W(min_score=floors[r][i])) for i, u in enumerate(qs)],
             lambda u, w, cap=cap: eng.recommend_clubs_interest(u, 10, window=w, cap=cap),
             lambda u, w, cap=cap: eng.recommend_interest_all([u], 1, window=w, collect=cap), lambda u: [u])
    # a group of 16 seeds: the floor at its 10,000th aggregate score, from one collecting call
    seeds = qs[:16]
    eng.recommend_group(seeds, 1, "mean", collect=args.users)
    gsc = eng.scan_collected()[1]
    gfloor = float(gsc[min(10000, len(gsc)) - 1])
    case("group G = 16, floor at the 10000th score", [(0, W(min_score=gfloor))] * max(6, args.steps // 4),
         lambda u, w: eng.recommend_clubs_group(seeds, 10, "mean", window=w, cap=65536),
         lambda u, w: eng.recommend_group(seeds, 1, "mean", window=w, collect=65536), lambda u: seeds)
    out = {"commit": args.commit, "users": args.users, "queries": qs, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
