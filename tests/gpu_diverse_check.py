"""Child process of test_gpu_diverse: the engine reads PF_DEBUG once per process, so each scan path
runs in its own.  argv[1] picks the check:
  full      by uid on E: no window and a floor, pool 1 / 64 / 65 / 1024, lambda 0 / 0.5 / 0.7 / 1, topk up to
            the pool; lambda = 1 against recommend_interest_all; topk = 0; an unknown uid
  state     under a candidate filter and under a field selection; overflow (cap = total - 1) and cap = total
  profile   E's users given by value: the by-uid list
  group     G = 5 under mean / min / max, G = 1 (the by-uid list), G = 0
  small     E cut to 2, 512 and 513 users
  big       the seeded 20,000-user synthetic corpus
  rerank    diverse_rerank of a recommend_collaborative result, of a list with unknown and repeated uids,
            under a selection, and its refusals
  sticks    the refusals of the scan calls; the window, collector, totals, scan_collected(), filter and
            selection read back unchanged, a by-uid scan before and after is identical

Expected values never come from the engine's diverse calls: the pool is the oracle's whole ranking
(Ref.ranking, a GroupRef's for a group, SelRef's under a selection) cut in numpy to the filter and the
window; sim is Oracle.fas_pairs(picked, pool); diverse_ref.rerank gives the list.  Ids, float bits, double
bits and info must be equal.  Exits non-zero on any mismatch."""
import ctypes
import sys
import tempfile

import numpy as np

import diverse_ref as dr
import edge_corpus as ec
import gpu_scan_filter_check as fchk
import gpu_scan_window_check as wchk
import pokec_testlib as tl

pf = tl.product()
W = pf.ScanWindow.make
f32 = np.float32
fail, cut = wchk.fail, wchk.cut
N_CASES = [0]
TIES = [0]


class Sim:
    """sim(s, idx) over a pool of uids from a pair scorer, one row per picked user, scored once."""

    def __init__(self, pairs, pool):
        self.pairs, self.pool, self.rows = pairs, np.asarray(pool, np.int32), {}

    def __call__(self, s, idx):
        if s not in self.rows:
            self.rows[s] = np.asarray(self.pairs(np.full(len(self.pool), self.pool[s], np.int32), self.pool), f32)
        return self.rows[s][idx]


def expect(pairs, rank, pool, lam, k, cap=1 << 20, sims=None):
    """(ids, r, pen, value, info) of the definition over a ranking (ids, scores) already cut to the window."""
    ids, sc = np.asarray(rank[0], np.int32), np.asarray(rank[1], f32)
    total = len(ids)
    if k == 0:
        total = 0
    if total == 0 or total > cap or k == 0:
        z = np.zeros(0)
        return z.astype(np.int32), z.astype(f32), z.astype(f32), z, {"total": total, "pool": 0, "pairs": 0}
    m = min(int(pool), total)
    key = (ids[:m].tobytes(), id(pairs))
    if sims is not None and key in sims:
        sim = sims[key]
    else:
        sim = Sim(pairs, ids[:m])
        if sims is not None:
            sims[key] = sim
    got = dr.rerank(ids[:m], sc[:m], sim, lam, k)
    v = dr.value(lam, sc[:m], np.zeros(m, f32))
    TIES[0] += int(len(np.unique(v)) < m)
    return got[0], got[1], got[2], got[3], {"total": total, "pool": m, "pairs": m * m}


def check(tag, got, want):
    """got: the binding's (ids, scores, info); want: expect()'s."""
    N_CASES[0] += 1
    info = got[2]
    if dr.same((got[0], got[1], info["pen"], info["value"]), want[:4]) and \
            {k: int(info[k]) for k in ("total", "pool", "pairs")} == want[4]:
        return 0
    n = 6
    return fail(tag, "got", list(got[0][:n]), [float(x).hex() for x in info["value"][:n]], [float(x).hex() for x in info["pen"][:n]],
                {k: int(info[k]) for k in ("total", "pool", "pairs")}, "want", list(want[0][:n]), [float(x).hex() for x in want[3][:n]],
                [float(x).hex() for x in want[2][:n]], want[4])


LAMS = (0.0, 0.5, 0.7, 1.0)


def sweep(name, call, pairs, rank, windows, pools=(1, 64, 65, 1024), lams=LAMS, ks=(10,)):
    """call(k, lam, pool, window) -> (ids, scores, info) over the windows, pools, lambdas and topk values."""
    sims = {}
    for w in windows:
        r = cut(rank, w)
        for pool in pools:
            for lam in lams:
                for k in ks:
                    kk = pool + 5 if k == "pool" else k
                    if check((name, "floor", None if w is None else float(w.min_score), "pool", pool, "lam", lam, "k", kk),
                             call(kk, lam, pool, w), expect(pairs, r, pool, lam, kk, sims=sims)):
                        return 1
    return 0


def check_full():
    c, eng, orc, ref = wchk.open_e()
    try:
        for i in (441, 1):
            u = ec.uid_of(i)
            ids, sc, _ = ref.ranking(u)
            if sweep("uid %d" % u, lambda k, lam, pool, w: eng.recommend_diverse_interest(u, k, lam=lam, pool=pool, window=w),
                     orc.fas_pairs, (ids, sc), [None, W(min_score=0.125)], ks=(1, 12)):
                return 1
            # every member of a pool picked, and topk past the pool
            if sweep("uid %d whole pool" % u, lambda k, lam, pool, w: eng.recommend_diverse_interest(u, k, lam=lam, pool=pool, window=w),
                     orc.fas_pairs, (ids, sc), [None], pools=(64, 65), lams=(0.7, 0.0), ks=("pool",)):
                return 1
            # lambda = 1 is the plain ranking's head
            for pool in (64, 1024):
                got = eng.recommend_diverse_interest(u, 64, lam=1.0, pool=pool)
                if not wchk.same(got[:2], eng.recommend_interest_all([u], 64)[0]) or not wchk.same(got[:2], (ids[:64], sc[:64])):
                    return fail("lambda = 1 is not the ranking's head", u, pool)
        if TIES[0] == 0:
            return fail("guard: no pool with tied relevances")
        # the 601 byte-identical users: a pool of 1024 holds them, tied in value across waves
        ids, sc, _ = ref.ranking(ec.uid_of(441))
        run = max(int((sc[:1024] == x).sum()) for x in np.unique(sc[:1024]))
        if run < 500:
            return fail("guard: the tied run inside the pool", run)
        u = ec.uid_of(441)
        for k in (0, 1):
            if check(("topk", k), eng.recommend_diverse_interest(u, k), expect(orc.fas_pairs, (ids, sc), 200, 0.7, k)):
                return 1
        # a cursor in the window: the pool is the ranking after it
        w = W(min_score=0.125, after=(sc[100], int(ids[100])))
        if check(("cursor",), eng.recommend_diverse_interest(u, 10, pool=65, window=w), expect(orc.fas_pairs, cut((ids, sc), w), 65, 0.7, 10)):
            return 1
        got = eng.recommend_diverse_interest(5, 10)  # an unknown uid
        if len(got[0]) or {k: int(got[2][k]) for k in ("total", "pool", "pairs")} != {"total": 0, "pool": 0, "pairs": 0}:
            return fail("unknown uid", got)
        print("full:", N_CASES[0], "lists")
        return 0
    finally:
        eng.close()


def check_state():
    import field_select_ref as fsr
    c, eng, orc, ref = wchk.open_e()
    try:
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            filt = pf.CandFilter.make(gender=1)
            mask = fchk.np_pass(c, filt)
            for i in (1, 441):
                u = ec.uid_of(i)
                ids, sc, idx = ref.ranking(u)
                rank = (ids[mask[idx]], sc[mask[idx]])
                if len(rank[0]) < 200:
                    return fail("the filter leaves too few candidates", len(rank[0]))
                if sweep("filter %d" % u, lambda k, lam, pool, w: eng.recommend_diverse_interest(u, k, lam=lam, pool=pool, window=w, filter=filt),
                         orc.fas_pairs, rank, [None, W(min_score=0.125)], pools=(65, 1024), lams=(0.7, 0.0)):
                    return 1
            # a field selection: the ranking and the similarities from the derived oracle
            sel = pf.FieldSelect.make(fixed=0x7F & ~((1 << pf.PF_F_AGE) | (1 << pf.PF_F_CLUBS)),
                                      cols=[t for t in range(ec.N_COLS) if t != ec.COL_L])
            Rs = fsr.SelRef(c, sel)
            for i in (1, 441):
                u = ec.uid_of(i)
                rank = Rs.ranking(u)[:2]
                if sweep("select %d" % u, lambda k, lam, pool, w: eng.recommend_diverse_interest(u, k, lam=lam, pool=pool, window=w, select=sel),
                         Rs.fas_pairs, rank, [None, W(min_score=rank[1][70])], pools=(64, 200), lams=(0.7, 0.0)):
                    return 1
            if eng._filter is not None or eng._select is not None:
                return fail("filter= / select= left something in force")
            u = ec.uid_of(441)
            rank = cut(ref.ranking(u)[:2], W(min_score=0.125))
            total = len(rank[0])
            for cap in (total - 1, total, 1):
                if check(("cap", cap), eng.recommend_diverse_interest(u, 10, cap=cap, window=W(min_score=0.125)),
                         expect(orc.fas_pairs, rank, 200, 0.7, 10, cap=cap)):
                    return 1
        print("state ok", N_CASES[0])
        return 0
    finally:
        eng.close()


def check_profile():
    import query_profile_cases as qc
    c, eng, orc, ref = wchk.open_e()
    try:
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            for i in (441, 1, ec.EMPTY_USER):
                u = ec.uid_of(i)
                p = qc.clone_profile(pf, c, u)  # excludes adj[u] + {u}, by its own exclude list
                ids, sc, _ = ref.ranking(u)
                if sweep("profile %d" % u, lambda k, lam, pool, w: eng.recommend_diverse_profile(p, k, lam=lam, pool=pool, window=w),
                         orc.fas_pairs, (ids, sc), [None, W(min_score=0.125), W(min_score=sc[0])], pools=(1, 65, 1024), lams=(0.7, 0.0)):
                    return 1
        print("profile ok", N_CASES[0])
        return 0
    finally:
        eng.close()


def check_group():
    import group_ref as gr
    c, eng, orc, ref = wchk.open_e(want_kernel=2)
    try:
        R = gr.GroupRef(c, orc.fas_pairs)
        seeds = gr.uids(gr.SEEDS_MIXED)  # G = 5
        for agg in gr.AGGS:
            rank = R.expect(seeds, c.n_users, agg, exclude_adj=True)
            if len(rank[1]) < 800:
                return fail("guard: the group's candidates", len(rank[1]))
            if sweep("group %s" % agg,
                     lambda k, lam, pool, w: eng.recommend_diverse_group(seeds, k, agg, exclude_adj=True, lam=lam, pool=pool, window=w),
                     orc.fas_pairs, rank, [None, W(min_score=rank[1][200])], pools=(65, 1024), lams=(0.7, 0.0)):
                return 1
        u = ec.uid_of(441)  # G = 1 equals the by-uid list
        if sweep("G = 1", lambda k, lam, pool, w: eng.recommend_diverse_group([u], k, "mean", exclude_adj=True, lam=lam, pool=pool, window=w),
                 orc.fas_pairs, ref.ranking(u)[:2], [None], pools=(64,), lams=(0.5,)):
            return 1
        got = eng.recommend_diverse_group(gr.UNKNOWN_UIDS, 10, window=W(min_score=0.0))  # G = 0
        if len(got[0]) or int(got[2]["total"]) or int(got[2]["pool"]) or int(got[2]["pairs"]):
            return fail("G = 0", got)
        print("group ok", N_CASES[0])
        return 0
    finally:
        eng.close()


def check_small():
    for n in (2, 512, 513):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        c, eng, orc, ref = wchk.open_e(c)
        try:
            for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
                eng.set_scan_kernel(kind)
                for i in (0, 1):
                    u = ec.uid_of(i)
                    if sweep("small %d user %d" % (n, i), lambda k, lam, pool, w: eng.recommend_diverse_interest(u, k, lam=lam, pool=pool, window=w),
                             orc.fas_pairs, ref.ranking(u)[:2], [None], pools=(1, 1024), lams=(0.7, 0.0), ks=(3, 20)):
                        return 1
        finally:
            eng.close()
    print("small ok", N_CASES[0])
    return 0


def check_big():
    n = 20000
    sc_ = tl.synth.Corpus(n_users=n, seed=3, edge_cases=1)
    ptr = sc_.desc_ptr()
    c = tl.corpus_from_desc(ptr)
    eng, orc = tl.engine(ptr), tl.Oracle(None, desc_ptr=ptr)
    try:
        ref = fchk.Ref(c, orc)
        for u in (8, 1500):
            ids, sc, _ = ref.ranking(u)
            if len(ids) < n - 1000:
                return fail("guard: the ranking", len(ids))
            if sweep("big %d" % u, lambda k, lam, pool, w: eng.recommend_diverse_interest(u, k, lam=lam, pool=pool, window=w),
                     orc.fas_pairs, (ids, sc), [None, W(min_score=sc[300])], pools=(200, 1024), lams=(0.7, 0.3), ks=(20,)):
                return 1
        print("big ok", N_CASES[0])
        return 0
    finally:
        eng.close()


def check_rerank():
    c, eng, orc, ref = wchk.open_e()
    try:
        index = c.index()

        def one(tag, uids, scores, k, lam, pairs=orc.fas_pairs, select=None):
            N_CASES[0] += 1
            known, seen, kr = [], set(), []
            for x, s in zip(uids, scores):
                if int(x) in index and int(x) not in seen:
                    seen.add(int(x))
                    known.append(int(x))
                    kr.append(s)
            want = dr.rerank(known, kr, Sim(pairs, known), lam, k)
            got = eng.diverse_rerank(uids, scores, k, lam, select=select)
            if not dr.same(got, want):
                return fail(tag, "got", list(got[0][:6]), [float(x).hex() for x in got[3][:6]], "want", list(want[0][:6]),
                            [float(x).hex() for x in want[3][:6]])
            return 0

        q = [ec.uid_of(i) for i in (1, 62, 466, 515, 1020)]
        n_lists = 0
        for (ids, sc) in eng.recommend_collaborative(q, 50):
            if len(ids) >= 5:
                n_lists += 1
                for lam in (0.7, 0.0, 1.0):
                    if one(("collab", lam), ids, sc, 10, lam):
                        return 1
        if n_lists == 0:
            return fail("guard: no collaborative list to re-rank")
        # a collected window in the caller's order; unknown and repeated uids; relevances that are no FAS
        ids, sc, _ = ref.ranking(ec.uid_of(441))
        if one(("head",), ids[:300], sc[:300], 300, 0.5):
            return 1
        mixed = [int(ids[3]), 5, int(ids[7]), int(ids[3]), 123456789, int(ids[9]), int(ids[7]), int(ids[200])]
        rel = [0.5, 9.0, -0.25, 0.9, 1.0, 0.5, 0.1, 0.0]
        for lam in (0.7, 0.0):
            if one(("mixed", lam), mixed, rel, 10, lam):
                return 1
        got = eng.diverse_rerank(mixed, rel, 10, 1.0)
        if list(got[0]) != [int(ids[3]), int(ids[9]), int(ids[200]), int(ids[7])] or list(got[1]) != [f32(0.5), f32(0.5), f32(0.0), f32(-0.25)]:
            return fail("mixed, lambda = 1", got)
        # under a selection of its own; the scan selection in force plays no part
        import field_select_ref as fsr
        sel = pf.FieldSelect.make(fixed=0x7F & ~(1 << pf.PF_F_AGE), cols=[t for t in range(ec.N_COLS) if t != ec.COL_L])
        Rs = fsr.SelRef(c, sel)
        if one(("select",), ids[:100], sc[:100], 12, 0.6, pairs=Rs.fas_pairs, select=sel):
            return 1
        eng.set_scan_select(sel)
        if one(("scan selection in force",), ids[:100], sc[:100], 12, 0.6):
            return 1
        eng.clear_scan_select()
        # empty lists and the refusals
        if len(eng.diverse_rerank([], [], 5, 0.5)[0]) or len(eng.diverse_rerank([5, 6], [1.0, 2.0], 5, 0.5)[0]) or \
                len(eng.diverse_rerank(ids[:5], sc[:5], 0, 0.5)[0]):
            return fail("empty lists")

        def code(fn):
            try:
                fn()
                return pf.PF_OK
            except pf.FasError as e:
                return e.code
        many = ids[:1025]
        for name, fn, want in (("NaN relevance", lambda: eng.diverse_rerank(ids[:3], [0.1, float("nan"), 0.2], 2, 0.5), pf.PF_EINVAL),
                               ("inf relevance", lambda: eng.diverse_rerank(ids[:3], [0.1, float("inf"), 0.2], 2, 0.0), pf.PF_EINVAL),
                               ("-inf relevance", lambda: eng.diverse_rerank(ids[:3], [0.1, 0.3, float("-inf")], 2, 0.5), pf.PF_EINVAL),
                               ("lambda 1.5", lambda: eng.diverse_rerank(ids[:3], sc[:3], 2, 1.5), pf.PF_EINVAL),
                               ("lambda -0.1", lambda: eng.diverse_rerank(ids[:3], sc[:3], 2, -0.1), pf.PF_EINVAL),
                               ("lambda NaN", lambda: eng.diverse_rerank(ids[:3], sc[:3], 2, float("nan")), pf.PF_EINVAL),
                               ("1025 entries", lambda: eng.diverse_rerank(many, np.zeros(1025), 2, 0.5), pf.PF_EUNSUPP),
                               ("1024 entries", lambda: eng.diverse_rerank(list(many[:1024]) + [int(many[0])], np.zeros(1025), 2, 0.5), pf.PF_OK)):
            if code(fn) != want:
                return fail("rerank refusal", name, code(fn))
        L, h = eng._L, eng.h
        u3, s3 = np.asarray(ids[:3], np.int32), np.asarray(sc[:3], f32)
        ou, os_, n = np.zeros(4, np.int32), np.zeros(4, f32), np.zeros(1, np.int32)
        if L.pf_diverse_rerank(h, u3.ctypes.data, s3.ctypes.data, 3, 0.5, -1, None, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data) != pf.PF_EINVAL or \
                L.pf_diverse_rerank(h, u3.ctypes.data, s3.ctypes.data, 3, 0.5, 2, None, None, None, None, None, n.ctypes.data) != pf.PF_EINVAL or \
                L.pf_diverse_rerank(h, u3.ctypes.data, s3.ctypes.data, 3, 0.5, 2, None, ou.ctypes.data, os_.ctypes.data, None, None, None) != pf.PF_EINVAL or \
                L.pf_diverse_rerank(h, None, None, 3, 0.5, 2, None, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data) != pf.PF_EINVAL:
            return fail("rerank raw refusals")
        if L.pf_diverse_rerank(None, u3.ctypes.data, s3.ctypes.data, 3, 0.5, 2, None, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data) != pf.PF_EINVAL:
            return fail("rerank with a NULL context")
        # pen and value may be NULL
        if L.pf_diverse_rerank(h, u3.ctypes.data, s3.ctypes.data, 3, 0.5, 2, None, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data) != pf.PF_OK or n[0] != 2:
            return fail("rerank with NULL pen / value", n[0])
        print("rerank ok", N_CASES[0])
        return 0
    finally:
        eng.close()


def check_sticks():
    c, eng, orc, ref = wchk.open_e()
    try:
        q = [ec.uid_of(i) for i in (1, 62, 466, 515, 1020)]
        u = ec.uid_of(441)

        def bits(res):
            return [(list(i), list(np.asarray(s, np.float32).view(np.uint32))) for i, s in res]

        def code(fn):
            try:
                fn()
                return pf.PF_OK
            except pf.FasError as e:
                return e.code

        eng.recommend_diverse_interest(u, 10)
        if code(eng.scan_collected) != pf.PF_EINVAL:
            return fail("a diverse call left a collected result behind")
        filt = pf.CandFilter.make(gender=1)
        eng.set_scan_window(min_score=0.2, count=True)
        eng.set_scan_collect(700)
        plain = bits(eng.recommend_interest_all(q[:1], 64))
        totals = [int(x) for x in eng.scan_window_totals()]
        coll = eng.scan_collected()
        want = expect(orc.fas_pairs, ref.ranking(u)[:2], 64, 0.7, 10)
        for call in (lambda: eng.recommend_diverse_interest(u, 10, pool=64),
                     lambda: eng.recommend_diverse_interest(u, 10, pool=64, cap=5),            # overflow
                     lambda: eng.recommend_diverse_group(q, 10, window=W(min_score=0.1, count=True)),
                     lambda: eng.recommend_diverse_interest(u, 10, filter=filt),
                     lambda: eng.recommend_diverse_interest(5, 10)):                           # unknown uid
            call()
            after = eng.scan_collected()
            if [int(x) for x in eng.scan_window_totals()] != totals or after[2] != coll[2] or not wchk.same(after[:2], coll[:2]):
                return fail("a diverse call changed the stored totals or the collected result")
            if eng._collect != 700 or eng._window is None or eng._window.fields != (pf.PF_WIN_MIN | pf.PF_WIN_COUNT) or \
                    eng._filter is not None or eng._select is not None:
                return fail("a diverse call changed the binding's state")
        if check(("under a window in force",), eng.recommend_diverse_interest(u, 10, pool=64), want):
            return 1
        if bits(eng.recommend_interest_all(q[:1], 64)) != plain or [int(x) for x in eng.scan_window_totals()] != totals:
            return fail("the plain call after a diverse call differs")
        after = eng.scan_collected()
        if after[2] != coll[2] or not wchk.same(after[:2], coll[:2]):
            return fail("the collector in force does not collect as before")
        eng.clear_scan_collect()
        eng.clear_scan_window()
        base = bits(eng.recommend_interest_all(q, 64))
        eng.recommend_diverse_interest(u, 10)
        eng.diverse_rerank(q, [0.5] * len(q), 3, 0.5)
        if bits(eng.recommend_interest_all(q, 64)) != base:
            return fail("a by-uid scan changed after a diverse call")
        # the refusals
        L, h = eng._L, eng.h
        ou, os_, n = np.zeros(10, np.int32), np.zeros(10, np.float32), np.zeros(1, np.int32)

        def raw(cap=5000, pool=64, lam=0.7, win=None, k=10, out=True, cnt=True, query=True):
            qq = pf.DiverseQuery()
            qq.cap, qq.pool, qq.lam = cap, pool, lam
            qq.window = None if win is None else ctypes.addressof(win)
            return L.pf_recommend_diverse_interest(h, u, ctypes.byref(qq) if query else None, k, ou.ctypes.data if out else None,
                                                   os_.ctypes.data if out else None, None, None, n.ctypes.data if cnt else None, None)
        nan_w = W(min_score=0.5)
        nan_w.min_score = float("nan")
        odd_w = W(min_score=0.5)
        odd_w.fields |= 64
        qq = pf.DiverseQuery()
        qq.cap, qq.pool, qq.lam = 5000, 64, 0.7
        gq = pf.GroupQuery.make(q)
        prof, parr = eng._profile_array(pf.QueryProfile.make(age=25))
        for name, rc in (("interest", L.pf_recommend_diverse_interest(None, u, ctypes.byref(qq), 10, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data, None)),
                         ("profile", L.pf_recommend_diverse_profile(None, ctypes.byref(parr), ctypes.byref(qq), 10, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data, None)),
                         ("group", L.pf_recommend_diverse_group(None, ctypes.byref(gq), ctypes.byref(qq), 10, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data, None)),
                         ("null profile", L.pf_recommend_diverse_profile(h, None, ctypes.byref(qq), 10, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data, None)),
                         ("null group", L.pf_recommend_diverse_group(h, None, ctypes.byref(qq), 10, ou.ctypes.data, os_.ctypes.data, None, None, n.ctypes.data, None))):
            if rc != pf.PF_EINVAL:
                return fail("a NULL context, profile or group", name, rc)
        for name, rc, want_rc in (("cap 0", raw(cap=0), pf.PF_EINVAL), ("cap -1", raw(cap=-1), pf.PF_EINVAL),
                                  ("cap 2^31", raw(cap=2**31), pf.PF_EINVAL), ("pool 0", raw(pool=0), pf.PF_EINVAL),
                                  ("pool -3", raw(pool=-3), pf.PF_EINVAL), ("pool 1025", raw(pool=1025), pf.PF_EUNSUPP),
                                  ("lambda 1.01", raw(lam=1.01), pf.PF_EINVAL), ("lambda -0.5", raw(lam=-0.5), pf.PF_EINVAL),
                                  ("lambda NaN", raw(lam=float("nan")), pf.PF_EINVAL), ("topk -1", raw(k=-1), pf.PF_EINVAL),
                                  ("null outputs", raw(out=False), pf.PF_EINVAL), ("null count", raw(cnt=False), pf.PF_EINVAL),
                                  ("null query", raw(query=False), pf.PF_EINVAL), ("NaN floor", raw(win=nan_w), pf.PF_EINVAL),
                                  ("window bits", raw(win=odd_w), pf.PF_EINVAL)):
            if rc != want_rc:
                return fail("refusal", name, rc)
        if raw(k=0, out=False) != pf.PF_OK or raw() != pf.PF_OK or n[0] != 10:
            return fail("a good call after the refusals", n[0])
        if code(lambda: eng.recommend_diverse_group(q, 10, agg=7)) != pf.PF_EINVAL:
            return fail("the group call's refusals")
        eng.set_shard(0, 2)
        rc = code(lambda: eng.recommend_diverse_interest(u, 10))
        msg = eng._L.pf_last_error(eng.h)
        eng.set_shard(0, 1)
        if rc != pf.PF_EUNSUPP or b"shard" not in msg:
            return fail("a sharded context", rc, msg)
        if eng._window is not None or eng._collect != 0:
            return fail("state after the refusals")
        if check(("after the refusals",), eng.recommend_diverse_interest(u, 10, pool=64), want):
            return 1
        print("sticks ok")
        return 0
    finally:
        eng.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    rc = {"full": check_full, "state": check_state, "profile": check_profile, "group": check_group, "small": check_small,
          "big": check_big, "rerank": check_rerank, "sticks": check_sticks}[mode]()
    if rc == 0:
        print("ok")
    sys.exit(rc)
