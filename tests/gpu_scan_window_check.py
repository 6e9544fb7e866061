"""Child process of test_gpu_scan_window: the engine reads PF_DEBUG once per process, so each launch
shape runs in its own.  argv[1] picks the check:
  full      the one-query scan (K5, or K1 under PF_DEBUG scan=stream): the guard facts, paging at
            k = 7 / 64 / 1, cursors that are not members, floors with counts, floor and cursor together
  path      what every path repeats: paging(7) of query 441, floors with counts on 441, 1 and 30, a
            floor and a cursor together; argv[2] = one | batch (8 queries in one call) | wide (the wide
            store) and whatever PF_DEBUG the parent set
  state     a candidate filter, a field selection, three shards merged on the host, explain=True
  profile   recommend_profile, E's own users given by value: paged past 64, floored and counted
  group     recommend_group: G = 5 mean / min / max paged to 200 results, floored and counted; G = 1
  async     scan_keys_async on a caller's stream, a different window before each call
  seed      under k5_prune_stats=1: a floor at 0.2 begins no block cold
  small     E cut to 2, 511, 512, 513 and 1025 users: paging(3) of user 0
  sticks    nothing sticks to the context; the refusals

The oracle has no window.  The expected list of (query, window, k) is the oracle's whole ranking of
the query (Oracle.interest([u], n_users, PF_MODE_ALL, 0)) cut in numpy to the window, then to its
first k; ids and float32 bits must be equal and the totals exact.  Exits non-zero on any mismatch."""
import json
import os
import sys
import tempfile

import numpy as np

import edge_corpus as ec
import gpu_scan_filter_check as fchk
import pokec_testlib as tl

pf = tl.product()
W = pf.ScanWindow.make
f32 = np.float32
TIE_441, TIE_1, TIE_30 = f32(0.35457027), f32(0.14928986), f32(0.10361052)
# idx -> (candidates, users scoring >= 0.125, (tie value, its first rank, its length))
GUARDS = {441: (1393, 1311, (TIE_441, 0, 599)), 1: (1395, 1190, (TIE_1, 187, 601)), 30: (1393, 506, (TIE_30, 645, 599)),
          ec.EMPTY_USER: (1399, 0, (f32(0.0), 0, 1399)), ec.EXCL_CLONES_Q: (874, 791, (TIE_441, 0, 75))}
Q_IDX = (441, 1, 30, ec.EMPTY_USER, ec.EXCL_CLONES_Q)
SEEN_TOTALS = []


def fail(*a):
    print("mismatch", *a, file=sys.stderr)
    return 1


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def down(x):
    return np.nextafter(f32(x), f32(-np.inf))


def same(g, r):
    return list(g[0]) == list(r[0]) and np.array_equal(np.asarray(g[1], np.float32).view(np.uint32),
                                                       np.asarray(r[1], np.float32).view(np.uint32))


def cut(rank, w):
    """A whole ranking (ids, scores) cut to the window: the tuple comparison of include/pokec_fas.h."""
    ids, sc = np.asarray(rank[0]), np.asarray(rank[1], np.float32)
    m = np.ones(len(ids), bool)
    if w is not None and w.fields & pf.PF_WIN_MIN:
        m &= sc >= f32(w.min_score)
    if w is not None and w.fields & pf.PF_WIN_AFTER:
        a = f32(w.after_score)
        m &= (sc < a) | ((sc == a) & (ids.astype(np.int64) > int(w.after_uid)))
    return ids[m], sc[m]


class Subject:
    """One ranked list the engine can be asked for under a window: call(k, window) -> (ids, scores),
    total() -> the count of the call just made, rank = the reference's whole ranking."""

    def __init__(self, name, call, total, rank):
        self.name, self.call, self.total, self.rank = name, call, total, (np.asarray(rank[0]), np.asarray(rank[1], np.float32))


def by_uid(eng, ref, u, name=None, **kw):
    return Subject(name or "uid %d" % u, lambda k, w: eng.recommend_interest_all([u], k, window=w, **kw)[0],
                   lambda: int(eng.scan_window_totals()[0]), ref.ranking(u)[:2])


def check_window(S, w, k):
    got = S.call(k, w)
    ids, sc = cut(S.rank, w)
    if not same(got, (ids[:k], sc[:k])):
        return fail(S.name, "window", w.fields, w.min_score, w.after_score, w.after_uid, "k", k, "got", list(got[0][:4]),
                    len(got[0]), "want", list(ids[:4]), min(k, len(ids)))
    if w.fields & pf.PF_WIN_COUNT:
        t = S.total()
        SEEN_TOTALS.append((t, k))
        if t != len(ids):
            return fail(S.name, "total", t, "numpy", len(ids), "floor", w.min_score, "after", w.after_score, w.after_uid)
    return 0


def check_paging(S, k, base=None, limit=None):
    """Pages of k chained by the cursor until a short page (or `limit` results): concatenated they
    are the reference's ranking inside `base`."""
    ids, sc = cut(S.rank, base)
    gi, gs, pages = [], [], 0
    for i, s in pf.pages(S.call, k, base):
        gi += [int(x) for x in i]
        gs += [f32(x) for x in s]
        pages += 1
        if limit is not None and len(gi) >= limit:
            break
        if pages > len(ids) // k + 2:
            return fail(S.name, "paging", k, "does not end")
    n = len(gi)
    if (limit is None and n != len(ids)) or (limit is not None and n < min(limit, len(ids))):
        return fail(S.name, "paging", k, "returned", n, "of", len(ids))
    if not same((gi, gs), (ids[:n], sc[:n])):
        bad = next((j for j in range(n) if gi[j] != int(ids[j])), -1)
        return fail(S.name, "paging", k, "first difference at rank", bad)
    return 0


def floors_of(S, extra=()):
    sc = S.rank[1]
    fl = [sc[j] for j in (0, 9, 10, 63) if j < len(sc)]
    fl += [f32(0.125), up(0.125), down(0.125), f32(0.36), f32(0.0), f32(-0.0), f32(-1.0), f32(1.0)]
    for t in extra:
        fl += [f32(t), up(t), down(t)]
    return fl


def check_floors(S, floors, ks=(10, 64)):
    for fl in floors:
        for k in ks:
            if check_window(S, W(min_score=fl, count=True), k):
                return 1
    return 0


def check_guards(ref):
    for i in Q_IDX:
        ids, sc, _ = ref.ranking(ec.uid_of(i))
        n, ge, (tv, t0, tn) = GUARDS[i]
        tie = np.nonzero(sc == tv)[0]
        if len(ids) != n or int((sc >= f32(0.125)).sum()) != ge or len(tie) != tn or int(tie[0]) != t0 or int(tie[-1]) != t0 + tn - 1:
            return fail("guard", i, len(ids), int((sc >= f32(0.125)).sum()), len(tie), int(tie[0]) if len(tie) else -1)
    if ref.ranking(ec.uid_of(ec.EMPTY_USER))[1].any():
        return fail("guard: EMPTY_USER's scores are not all 0.0")
    return 0


def open_e(c=None, want_kernel=None):
    c = tl.golden_corpus("E") if c is None else c
    eng, orc = tl.engine(c), tl.Oracle(c)
    if want_kernel is None:
        want_kernel = 1 if "scan=stream" in os.environ.get("PF_DEBUG", "") else 2
    if eng.layout().scan_kernel != want_kernel:
        raise SystemExit("scan kernel %d, wanted %d" % (eng.layout().scan_kernel, want_kernel))
    return c, eng, orc, fchk.Ref(c, orc)


def check_full():
    c, eng, orc, ref = open_e()
    try:
        if check_guards(ref):
            return 1
        subs = {i: by_uid(eng, ref, ec.uid_of(i)) for i in Q_IDX}
        # paging: through ties that span pages, waves and the 512-candidate block edges
        for i in Q_IDX:
            for k in (7, 64):
                if check_paging(subs[i], k):
                    return 1
        if check_paging(subs[441], 1, limit=130):
            return 1
        # cursors that are not members (E's uids are 7 or more apart: uid + 3 is nobody)
        for i, tv in ((441, TIE_441), (1, TIE_1)):
            S = subs[i]
            ids, sc = S.rank
            tie = ids[sc == tv]
            mid = int(np.sort(tie)[len(tie) // 2])
            below = f32((float(sc[sc < tv].max()) + float(tv)) / 2)   # between two scores
            cursors = [(tv, mid + 3), (tv, 0), (tv, -2**31), (tv, 2**31 - 1), (tv, ec.UID_MAX), (below, mid), (below, -2**31),
                       (f32(0.9), 5), (f32(np.inf), 2**31 - 1), (up(tv), -2**31), (down(tv), 2**31 - 1),
                       (sc[-1], int(ids[-1])), (sc[-1], 2**31 - 1), (f32(-1.0), 0), (f32(-0.0), -2**31), (f32(0.0), 2**31 - 1)]
            for a in cursors:
                for k in (10, 64):
                    if check_window(S, W(after=a, count=True), k):
                        return 1
            if not (below < tv and below > sc[sc < tv].max()):
                return fail("no float between the tie and the next score", i)
            # past the last candidate: nothing, and a count of 0
            if len(S.call(10, W(after=(sc[-1], int(ids[-1])), count=True))[0]) != 0 or S.total() != 0:
                return fail("cursor past the last candidate", i)
        # floors, each with a count
        if check_floors(subs[441], floors_of(subs[441], (TIE_441,))) or check_floors(subs[1], floors_of(subs[1], (TIE_1,))):
            return 1
        if check_floors(subs[30], floors_of(subs[30], (TIE_30,))):  # 0.10361052 is below the histogram: unseeded
            return 1
        if check_floors(subs[ec.EMPTY_USER], floors_of(subs[ec.EMPTY_USER])) or check_floors(subs[ec.EXCL_CLONES_Q], floors_of(subs[ec.EXCL_CLONES_Q])):
            return 1
        S = subs[441]
        S.call(10, W(min_score=0.36, count=True))
        if S.total() != 0 or len(S.call(64, W(min_score=0.36))[0]) != 0:
            return fail("floor above everybody")
        for fl in (0.0, -1.0):
            S.call(10, W(min_score=fl, count=True))
            if S.total() != len(S.rank[0]):
                return fail("floor", fl, "total", S.total())
        ts = [t for t, _ in SEEN_TOTALS]
        if not (any(t > 64 for t in ts) and any(0 < t < k for t, k in SEEN_TOTALS) and any(t == 0 for t in ts)):
            return fail("the floors' totals do not cover > 64, 0 < t < k and 0")
        # floor and cursor together: paging inside [floor, best]
        for i, fl in ((441, 0.125), (441, TIE_441), (1, TIE_1), (1, 0.15), (1, up(TIE_1))):
            for k in (7, 64):
                if check_paging(subs[i], k, base=W(min_score=fl, count=True)):
                    return 1
        S = subs[1]
        ids, sc = S.rank
        for a in ((TIE_1, int(ids[400])), (sc[100], int(ids[100]))):
            for fl in (TIE_1, down(TIE_1), 0.125):
                if check_window(S, W(min_score=fl, after=a, count=True), 64):
                    return 1
        print("full:", len(SEEN_TOTALS), "counted windows")
        return 0
    finally:
        eng.close()


def path_checks(c, eng, ref, batch):
    q = [ec.uid_of(i) for i in Q_IDX]
    if not batch:
        S = by_uid(eng, ref, q[0])
        if check_paging(S, 7):
            return 1
        for i, u in zip(Q_IDX[:3], q[:3]):
            S = by_uid(eng, ref, u)
            if check_floors(S, [f32(0.125), S.rank[1][9], GUARDS[i][2][0], up(GUARDS[i][2][0]), f32(0.36), f32(0.0)]):
                return 1
        S = by_uid(eng, ref, q[1])
        return check_paging(S, 7, base=W(min_score=TIE_1, count=True)) or check_paging(S, 64, base=W(min_score=0.125))
    # 8 queries in one call: one window serves all of them
    qs = q + [ec.uid_of(i) for i in (511, 700, 1399)]
    ranks = [ref.ranking(u)[:2] for u in qs]

    def call_all(k, w):
        got = eng.recommend_interest_all(qs, k, window=w)
        want = [cut(r, w) for r in ranks]
        for u, g, (ids, sc) in zip(qs, got, want):
            if not same(g, (ids[:k], sc[:k])):
                return fail("batch", u, k, w.fields if w else 0, list(g[0][:4]), list(ids[:4]))
        if w is not None and w.fields & pf.PF_WIN_COUNT:
            t = eng.scan_window_totals()
            if [int(x) for x in t] != [len(ids) for ids, _ in want]:
                return fail("batch totals", list(t), [len(ids) for ids, _ in want])
        return 0
    # query 441's chain of k = 7 cursors, applied to all eight queries
    w, n = None, 0
    while True:
        if call_all(7, w):
            return 1
        ids, sc = cut(ranks[0], w)
        if len(ids) < 7:
            break
        w = W(after=(sc[6], int(ids[6])), count=(n % 3 == 0))
        n += 1
    for fl in (f32(0.125), TIE_441, TIE_1, up(TIE_1), f32(0.36), f32(0.0)):
        for k in (10, 64):
            if call_all(k, W(min_score=fl, count=True)):
                return 1
    ids, sc = ranks[1]
    return call_all(64, W(min_score=0.125, after=(TIE_1, int(ids[300])), count=True))


def check_path(kind):
    import gpu_group_check as ggc
    c, eng, orc, ref = open_e(ggc.wide_e() if kind == "wide" else None)
    try:
        if eng.layout().packed_tokens != (0 if kind == "wide" else 1):
            return fail("store format", kind)
        rc = path_checks(c, eng, ref, kind == "batch")
        if rc == 0 and kind == "wide":  # the wide store's K1 as well
            eng.set_scan_kernel(pf.PF_SCAN_STREAM)
            rc = path_checks(c, eng, ref, False)
        return rc
    finally:
        eng.close()


def check_state():
    import group_ref as gr
    c, eng, orc, ref = open_e()
    try:
        u1, u441 = ec.uid_of(1), ec.uid_of(441)
        # a candidate filter: reference = filter mask and window
        filt = pf.CandFilter.make(gender=1)
        mask = fchk.np_pass(c, filt)
        for u in (u1, u441):
            ids, sc, idx = ref.ranking(u)
            S = by_uid(eng, ref, u, "filter %d" % u, filter=filt)
            S.rank = (ids[mask[idx]], sc[mask[idx]])
            if len(S.rank[0]) < 200:
                return fail("the filter leaves too few candidates", len(S.rank[0]))
            if check_paging(S, 7) or check_floors(S, [f32(0.125), S.rank[1][9], S.rank[1][70], f32(0.36)]):
                return 1
            if check_paging(S, 64, base=W(min_score=0.125, count=True)):
                return 1
        if eng._filter is not None or eng._window is not None:
            return fail("the filter / window in force before the call was not restored")
        # a field selection: reference scores from fas_pairs(select=)
        sel = pf.FieldSelect.make(fixed=0x7F & ~((1 << pf.PF_F_AGE) | (1 << pf.PF_F_CLUBS)),
                                  cols=[t for t in range(ec.N_COLS) if t != ec.COL_L])
        Rs = gr.GroupRef(c, lambda a, b: eng.fas_pairs(a, b, select=sel))
        for u in (u1, u441):
            S = by_uid(eng, ref, u, "select %d" % u, select=sel)
            S.rank = Rs.expect([u], c.n_users, "mean", exclude_adj=True)
            if check_paging(S, 7) or check_floors(S, [f32(0.125), S.rank[1][9], S.rank[1][70], f32(0.0)]):
                return 1
        # three shards merged on the host, the totals summed
        for u in (u1, u441, ec.uid_of(30)):
            rank = ref.ranking(u)[:2]
            wins = [W(min_score=0.125, count=True), W(min_score=rank[1][9], count=True), W(min_score=0.36, count=True),
                    W(after=(rank[1][200], int(rank[0][200])), count=True),
                    W(min_score=0.11, after=(rank[1][100], int(rank[0][100])), count=True)]
            for w in wins:
                for k in (10, 64):
                    parts, tot = [], 0
                    for sh in range(3):
                        eng.set_shard(sh, 3)
                        parts.append(eng.recommend_interest_all([u], k, window=w)[0])
                        tot += int(eng.scan_window_totals()[0])
                    eng.set_shard(0, 1)
                    ids, sc = cut(rank, w)
                    if not same(fchk.merged(parts, k), (list(ids[:k]), sc[:k])) or tot != len(ids):
                        return fail("shards", u, k, tot, len(ids))

            def sharded(k, w):
                parts = []
                for sh in range(3):
                    eng.set_shard(sh, 3)
                    parts.append(eng.recommend_interest_all([u], k, window=w)[0])
                eng.set_shard(0, 1)
                return fchk.merged(parts, k)
            if u == u441 and check_paging(Subject("sharded paging", sharded, None, rank), 7):
                return 1
        # explain=True under a window: the windowed list, each result with its breakdown
        rank = ref.ranking(u1)[:2]
        for w in (W(min_score=0.15), W(after=(rank[1][300], int(rank[0][300]))), W(min_score=0.125, after=(rank[1][64], int(rank[0][64])), count=True)):
            got = eng.recommend_interest_all([u1], 10, window=w, explain=True)[0]
            ids, sc = cut(rank, w)
            if len(got) != 3 or not same(got[:2], (ids[:10], sc[:10])) or len(got[2]) != len(got[0]):
                return fail("explain under a window")
            if not np.array_equal(np.asarray(got[2].score, np.float32).view(np.uint32), np.asarray(got[1], np.float32).view(np.uint32)):
                return fail("explain under a window: the breakdown's scores")
            if w.fields & pf.PF_WIN_COUNT and int(eng.scan_window_totals()[0]) != len(ids):
                return fail("explain under a window: total")
        print("state ok")
        return 0
    finally:
        eng.close()


def check_profile():
    import query_profile_cases as qc
    c, eng, orc, ref = open_e()
    try:
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            for i in (441, 1):
                u = ec.uid_of(i)
                p = qc.clone_profile(pf, c, u)
                S = Subject("profile %d" % u, lambda k, w: eng.recommend_profile(p, k, window=w)[0],
                            lambda: int(eng.scan_window_totals()[0]), ref.ranking(u)[:2])
                if check_paging(S, 64) or check_paging(S, 7, limit=150):  # past result 64
                    return 1
                if check_floors(S, [f32(0.125), S.rank[1][9], GUARDS[i][2][0], f32(0.36), f32(0.0)]):
                    return 1
                if check_paging(S, 64, base=W(min_score=0.125, count=True)):
                    return 1
        eng.set_scan_kernel(pf.PF_SCAN_POSTINGS)
        # a batch of profiles in one call: one window, a total per profile
        us = [ec.uid_of(i) for i in (441, 1, 30)]
        ps = [qc.clone_profile(pf, c, u) for u in us]
        w = W(min_score=0.125, count=True)
        got = eng.recommend_profile(ps, 64, window=w)
        tot = [int(x) for x in eng.scan_window_totals()]
        for u, g, t in zip(us, got, tot):
            ids, sc = cut(ref.ranking(u)[:2], w)
            if not same(g, (ids[:64], sc[:64])) or t != len(ids):
                return fail("profile batch", u, t, len(ids))
        print("profile ok")
        return 0
    finally:
        eng.close()


def check_group():
    import group_ref as gr
    c, eng, orc, ref = open_e(want_kernel=2)
    try:
        R = gr.GroupRef(c, orc.fas_pairs)
        seeds = gr.uids(gr.SEEDS_MIXED)  # G = 5
        for agg in gr.AGGS:
            for ea in (False, True):
                S = Subject("group %s %d" % (agg, ea), lambda k, w: eng.recommend_group(seeds, k, agg, exclude_adj=ea, window=w),
                            lambda: int(eng.scan_window_totals()[0]), R.expect(seeds, c.n_users, agg, exclude_adj=ea))
                if check_paging(S, 64, limit=200) or check_paging(S, 7, limit=200):
                    return 1
                sc = S.rank[1]
                if check_floors(S, [sc[0], sc[9], sc[10], sc[63], sc[200], up(sc[200]), down(sc[200]), f32(0.36), f32(0.0), f32(1.0)]):
                    return 1
                if check_paging(S, 64, base=W(min_score=sc[150], count=True)):
                    return 1
        # G = 1 equals the by-uid scan
        for i in (441, 1):
            u = ec.uid_of(i)
            rank = ref.ranking(u)[:2]
            for w in (W(min_score=0.125, count=True), W(after=(rank[1][90], int(rank[0][90])), count=True),
                      W(min_score=GUARDS[i][2][0], after=(rank[1][250], int(rank[0][250])), count=True)):
                for agg in gr.AGGS:
                    a = eng.recommend_group([u], 64, agg, exclude_adj=True, window=w)
                    ta = int(eng.scan_window_totals()[0])
                    b = eng.recommend_interest_all([u], 64, window=w)[0]
                    tb = int(eng.scan_window_totals()[0])
                    ids, sc = cut(rank, w)
                    if not same(a, b) or not same(a, (ids[:64], sc[:64])) or ta != tb or ta != len(ids):
                        return fail("G = 1", u, agg, ta, tb, len(ids))
        # G = 0: nothing, and a total of 0
        if len(eng.recommend_group(gr.UNKNOWN_UIDS, 10, window=W(min_score=0.0, count=True))[0]) != 0 or \
                [int(x) for x in eng.scan_window_totals()] != [0]:
            return fail("G = 0 under a counted window")
        print("group ok")
        return 0
    finally:
        eng.close()


def check_async():
    """Six one-query scan_keys_async calls on a caller's stream, a different window set before each
    and no synchronisation between them: every row obeys its own window, so it travels by value."""
    import torch
    c, eng, orc, ref = open_e()
    try:
        q = [ec.uid_of(i) for i in (441, 1, 30, ec.EXCL_CLONES_Q, 700, 511)]
        r1 = ref.ranking(q[1])[:2]
        wins = [W(min_score=0.125), W(after=(TIE_441, ec.uid_of(800) + 3)), W(min_score=0.11, after=(r1[1][50], int(r1[0][50]))),
                None, W(min_score=0.36), W(after=(f32(0.2), 0))]
        s = torch.cuda.Stream()
        for k in (10, 64):
            for rot in range(3):
                us = q[rot:] + q[:rot]
                rows = torch.full((6, k), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                for i, (u, w) in enumerate(zip(us, wins)):
                    eng.set_scan_window(w)
                    eng.scan_keys_async([u], k, rows[i].data_ptr(), s.cuda_stream)
                eng.clear_scan_window()
                s.synchronize()
                keys = rows.cpu().numpy().view(np.uint64)
                for i, (u, w) in enumerate(zip(us, wins)):
                    ids, sc = cut(ref.ranking(u)[:2], w)
                    if not same(pf.decode_keys(keys[i]), (ids[:k], sc[:k])):
                        return fail("async", i, u, k)
        # six queries in one asynchronous call (the batch launch) under a cursor
        w = W(after=(TIE_1, ec.uid_of(600)))
        rows = torch.full((6, 64), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.set_scan_window(w)
        eng.scan_keys_async(q, 64, rows.data_ptr(), s.cuda_stream)
        eng.clear_scan_window()
        s.synchronize()
        keys = rows.cpu().numpy().view(np.uint64)
        for i, u in enumerate(q):
            ids, sc = cut(ref.ranking(u)[:2], w)
            if not same(pf.decode_keys(keys[i]), (ids[:64], sc[:64])):
                return fail("async batch", u)
        print("async ok")
        return 0
    finally:
        eng.close()


def check_seed():
    c, eng, orc, ref = open_e()
    try:
        u = ec.uid_of(441)
        S = by_uid(eng, ref, u)
        out = {}
        for fl in (0.2, 0.1):
            eng.k5_prune_stats(reset=True)
            for k in (10, 64):
                if check_window(S, W(min_score=fl), k):
                    return 1
            out["%g" % fl] = eng.k5_prune_stats()
        eng.k5_prune_stats(reset=True)
        if check_window(S, W(min_score=0.2, count=True), 10):
            return 1
        out["0.2 counted"] = eng.k5_prune_stats()
        print("stats " + json.dumps(out))
        return 0
    finally:
        eng.close()


def check_small():
    for n in (2, 511, 512, 513, 1025):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        c, eng, orc, ref = open_e(c)
        try:
            for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
                eng.set_scan_kernel(kind)
                # (at n = 2 user 0's only other user is in its adjacency row: an empty ranking; user 1 has one)
                S = by_uid(eng, ref, ec.uid_of(0))
                if check_paging(S, 3) or check_paging(by_uid(eng, ref, ec.uid_of(1)), 3):
                    return fail("small", n, kind)
                if n > 2 and len(S.rank[0]) < 500:
                    return fail("small", n, "user 0 has too few candidates", len(S.rank[0]))
                if n > 2 and check_floors(S, [S.rank[1][1], f32(0.0), f32(0.36)], ks=(3,)):
                    return 1
        finally:
            eng.close()
    print("small ok")
    return 0


def check_sticks():
    c, eng, orc, ref = open_e()
    try:
        q = [ec.uid_of(i) for i in (1, 62, 466, 515, 1020)]

        def bits(res):
            return [(list(i), list(np.asarray(s, np.float32).view(np.uint32))) for i, s in res]

        def snapshot():
            return [bits(eng.recommend_interest_all(q, 64)), bits(eng.recommend_graph_registration(q, 10)),
                    bits(eng.recommend_collaborative(q, 10)), bits(eng.recommend_clubs_collab(q, 10)),
                    list(np.asarray(eng.fas_pairs(q, list(reversed(q))), np.float32).view(np.uint32)), list(eng.scan_bytes(q))]

        def code(fn):
            try:
                fn()
                return pf.PF_OK
            except pf.FasError as e:
                return e.code
        if code(eng.scan_window_totals) != pf.PF_EINVAL:
            return fail("totals before any counted call")
        before = snapshot()
        for (i, s), r in zip(before[0], orc.interest(q, 64, tl.PF_MODE_ALL, 0)):
            if i != list(r[0]) or s != list(np.asarray(r[1], np.float32).view(np.uint32)):
                return fail("by-uid lists differ from the oracle before any window")
        eng.set_scan_window(min_score=0.2, after=(0.3, 1234), count=True)
        under = snapshot()
        # FoF interest, collab, clubs, the pair call and scan_bytes never see the window; the scan does
        if under[1:] != before[1:]:
            return fail("a call that does not read the window changed under it")
        if under[0] == before[0]:
            return fail("the all-candidates scan ignored the window in force")
        # malformed windows are refused and leave the one in force alone
        bad = [W(min_score=0.1), W(min_score=0.1), W(min_score=float("nan")), W(after=(float("nan"), 3))]
        bad[0].fields |= 8
        bad[1].flags = 1
        for w in bad:
            rc = eng._L.pf_set_scan_window(eng.h, w)
            if rc != pf.PF_EINVAL or bits(eng.recommend_interest_all(q, 64)) != under[0]:
                return fail("malformed window", rc)
        # a NaN in a member its bit does not name is not read
        w = W(min_score=0.2, after=(0.3, 1234), count=True)
        w2 = W(min_score=0.2)
        w2.after_score = float("nan")
        if eng._L.pf_set_scan_window(eng.h, w2) != pf.PF_OK:
            return fail("NaN in an unnamed member refused")
        eng.set_scan_window(w)
        if code(lambda: eng.recommend_interest_all(q[:1], 100)) != pf.PF_EUNSUPP or b"window" not in eng._L.pf_last_error(eng.h):
            return fail("topk 100 under a window")
        import torch
        rows = torch.full((1, 10), -1, dtype=torch.int64, device="cuda")
        if code(lambda: eng.scan_keys_async(q[:1], 10, rows.data_ptr(), 0)) != pf.PF_EUNSUPP or b"COUNT" not in eng._L.pf_last_error(eng.h):
            return fail("a counted scan_keys_async")
        torch.cuda.synchronize()
        eng.clear_scan_window()
        if eng._window is not None or snapshot() != before:
            return fail("a result changed after the window was cleared")
        if len(eng.recommend_interest_all(q[:1], 100)[0][0]) != 100:
            return fail("topk 100 without a window")
        # window= on a call restores the window in force before it
        eng.set_scan_window(min_score=0.2)
        eng.recommend_interest_all(q[:1], 10, window=W(after=(0.1, 5)))
        ids, sc = cut(ref.ranking(q[0])[:2], W(min_score=0.2))
        if eng._window is None or eng._window.fields != pf.PF_WIN_MIN or \
                not same(eng.recommend_interest_all(q[:1], 10)[0], (ids[:10], sc[:10])):
            return fail("window= did not restore the window in force")
        eng.clear_scan_window()
        # an unknown uid in a counted call: no results and a total of 0
        got = eng.recommend_interest_all([q[0], 5, q[1]], 10, window=W(min_score=0.125, count=True))
        tot = [int(x) for x in eng.scan_window_totals()]
        want = [len(cut(ref.ranking(u)[:2], W(min_score=0.125))[0]) for u in (q[0], q[1])]
        if len(got[1][0]) != 0 or tot != [want[0], 0, want[1]]:
            return fail("unknown uid in a counted call", tot, want)
        print("sticks ok")
        return 0
    finally:
        eng.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    rc = {"full": check_full, "path": lambda: check_path(sys.argv[2]), "state": check_state, "profile": check_profile,
          "group": check_group, "async": check_async, "seed": check_seed, "small": check_small, "sticks": check_sticks}[mode]()
    if rc == 0:
        print("ok")
    sys.exit(rc)
