"""Child process of test_gpu_club_interest: the engine reads PF_DEBUG once per process, so each scan
path runs in its own.  argv[1] picks the check:
  full      by uid on E for the collect test's queries: no window and the floors of club_corpus.floors_of,
            neighbours = 1, 10, 64, 65 and the whole window, keep_own on and off, topk 10 and every club
  state     under a candidate filter and under a field selection; overflow (cap = total - 1) and cap = total
  profile   E's users given by value: the by-uid list (the clone profile carries the user's exclusions)
  group     G = 5 under mean / min / max, G = 1 (the by-uid list), G = 0
  small     E cut to 2, 512 and 513 users
  big       the seeded 20,000-user synthetic corpus: a floor a few hundred pass, and no window
  sticks    the refusals; a following plain call, the stored totals and scan_collected are unchanged

Expected values never come from the engine's club calls: club_corpus.expect builds them from the oracle's
whole ranking (Ref.ranking, cut by gpu_scan_window_check.cut) and the corpus's club lists.  Ids, counts,
info and float bits must be equal.  Exits non-zero on any mismatch."""
import sys
import tempfile

import numpy as np

import club_corpus as cc
import edge_corpus as ec
import gpu_scan_filter_check as fchk
import gpu_scan_window_check as wchk
import pokec_testlib as tl

pf = tl.product()
W = pf.ScanWindow.make
f32 = np.float32
fail, cut = wchk.fail, wchk.cut
N_CASES = [0]


def check(tag, got, want):
    N_CASES[0] += 1
    if cc.same(got, want):
        return 0
    return fail(tag, "got", list(got[0][:5]), [float(x).hex() for x in got[1][:5]], got[2], "want", list(want[0][:5]),
                [float(x).hex() for x in want[1][:5]], want[2])


def sweep(c, rows, name, call, rank, own, windows, ms=cc.NEIGHBOURS, ks=(10,)):
    """call(k, m, window, keep_own) -> (ids, scores, info) over the windows, neighbour counts and topk values."""
    for w in windows:
        r = cut(rank, w)
        for m in ms:
            for k in ks:
                for keep in (False, True):
                    want = cc.expect(c, rows, r, own, m, k, keep_own=keep)
                    if check((name, "floor", None if w is None else float(w.min_score), "m", m, "k", k, "keep_own", keep),
                             call(k, m, w, keep), want):
                        return 1
    return 0


def windows_of(sc):
    return [None] + [W(min_score=fl) for fl in cc.floors_of(sc)]


def check_full():
    c, eng, orc, ref = wchk.open_e()
    rows = cc.club_rows(c)
    try:
        sizes = set()
        for i in cc.Q_IDX:
            u = ec.uid_of(i)
            ids, sc, _ = ref.ranking(u)
            own = cc.own_clubs(c, rows, [u])
            for w in windows_of(sc):
                sizes.add(len(cut((ids, sc), w)[0]))
            if sweep(c, rows, "uid %d" % u, lambda k, m, w, keep: eng.recommend_clubs_interest(u, k, neighbours=m, window=w, keep_own=keep),
                     (ids, sc), own, windows_of(sc), ks=(10, 1000)):
                return 1
        if not (0 in sizes and 1 in sizes and max(sizes) > 64):
            return fail("guard: window sizes", sorted(sizes))
        # topk = 0 scans nothing; topk = 1
        u = ec.uid_of(441)
        rank = ref.ranking(u)[:2]
        own = cc.own_clubs(c, rows, [u])
        for k in (0, 1):
            if check(("topk", k), eng.recommend_clubs_interest(u, k), cc.expect(c, rows, rank, own, 0, k)):
                return 1
        # a cursor in the window: the neighbours are the ranking after it
        w = W(min_score=0.125, after=(rank[1][100], int(rank[0][100])))
        if check(("cursor",), eng.recommend_clubs_interest(u, 10, neighbours=65, window=w), cc.expect(c, rows, cut(rank, w), own, 65, 10)):
            return 1
        # an unknown uid
        got = eng.recommend_clubs_interest(5, 10)
        if len(got[0]) or got[2] != {"total": 0, "used": 0, "contributions": 0, "clubs": 0}:
            return fail("unknown uid", got)
        print("full:", N_CASES[0], "club lists")
        return 0
    finally:
        eng.close()


def check_state():
    import group_ref as gr
    c, eng, orc, ref = wchk.open_e()
    rows = cc.club_rows(c)
    try:
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            # a candidate filter: reference = filter mask, then window
            filt = pf.CandFilter.make(gender=1)
            mask = fchk.np_pass(c, filt)
            for i in (1, 441):
                u = ec.uid_of(i)
                ids, sc, idx = ref.ranking(u)
                rank = (ids[mask[idx]], sc[mask[idx]])
                if len(rank[0]) < 200:
                    return fail("the filter leaves too few candidates", len(rank[0]))
                own = cc.own_clubs(c, rows, [u])
                if sweep(c, rows, "filter %d" % u,
                         lambda k, m, w, keep: eng.recommend_clubs_interest(u, k, neighbours=m, window=w, keep_own=keep, filter=filt),
                         rank, own, [None, W(min_score=0.125)], ms=(10, 65, 0)):
                    return 1
            # a field selection: reference scores from the pair kernel under the selection
            sel = pf.FieldSelect.make(fixed=0x7F & ~((1 << pf.PF_F_AGE) | (1 << pf.PF_F_CLUBS)),
                                      cols=[t for t in range(ec.N_COLS) if t != ec.COL_L])
            Rs = gr.GroupRef(c, lambda a, b: eng.fas_pairs(a, b, select=sel))
            for i in (1, 441):
                u = ec.uid_of(i)
                rank = Rs.expect([u], c.n_users, "mean", exclude_adj=True)
                own = cc.own_clubs(c, rows, [u])
                if sweep(c, rows, "select %d" % u,
                         lambda k, m, w, keep: eng.recommend_clubs_interest(u, k, neighbours=m, window=w, keep_own=keep, select=sel),
                         rank, own, [None, W(min_score=rank[1][70])], ms=(64, 0)):
                    return 1
            if eng._filter is not None or eng._select is not None:
                return fail("filter= / select= left something in force")
            # overflow: cap = total - 1 reports the exact total and nothing else; cap = total serves
            u = ec.uid_of(441)
            rank = cut(ref.ranking(u)[:2], W(min_score=0.125))
            own = cc.own_clubs(c, rows, [u])
            total = len(rank[0])
            for cap in (total - 1, total, 1):
                if check(("cap", cap), eng.recommend_clubs_interest(u, 10, cap=cap, window=W(min_score=0.125)),
                         cc.expect(c, rows, rank, own, 0, 10, cap=cap)):
                    return 1
        print("state ok", N_CASES[0])
        return 0
    finally:
        eng.close()


def check_profile():
    import query_profile_cases as qc
    c, eng, orc, ref = wchk.open_e()
    rows = cc.club_rows(c)
    try:
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            for i in (441, 1, ec.EMPTY_USER):
                u = ec.uid_of(i)
                p = qc.clone_profile(pf, c, u)  # excludes adj[u] + {u}, by its own exclude list; carries u's clubs
                ids, sc, _ = ref.ranking(u)
                own = cc.own_clubs(c, rows, [u])
                if sweep(c, rows, "profile %d" % u,
                         lambda k, m, w, keep: eng.recommend_clubs_profile(p, k, neighbours=m, window=w, keep_own=keep),
                         (ids, sc), own, [None, W(min_score=0.125), W(min_score=sc[0])], ms=(1, 65, 0)):
                    return 1
                # the same list as by uid, through the engine as well
                if not cc.same(eng.recommend_clubs_profile(p, 10, neighbours=64), eng.recommend_clubs_interest(u, 10, neighbours=64)):
                    return fail("profile and uid disagree", u)
            # own clubs nobody in the corpus holds are simply not there
            u = ec.uid_of(441)
            p = qc.clone_profile(pf, c, u)
            f = p.fields()
            f["clubs"] = list(f["clubs"]) + [123456789]
            p2 = pf.QueryProfile.make(**f)
            # (a different club list is a different profile: only the call's success and the own filter are asked here)
            got = eng.recommend_clubs_profile(p2, 10)
            if len(got[0]) == 0 or set(int(x) for x in got[0]) & {11, 12, 13, 123456789}:
                return fail("a profile with an unknown club", got)
        print("profile ok", N_CASES[0])
        return 0
    finally:
        eng.close()


def check_group():
    import group_ref as gr
    c, eng, orc, ref = wchk.open_e(want_kernel=2)
    rows = cc.club_rows(c)
    try:
        R = gr.GroupRef(c, orc.fas_pairs)
        seeds = gr.uids(gr.SEEDS_MIXED)  # G = 5
        own = cc.own_clubs(c, rows, seeds)
        for agg in gr.AGGS:
            rank = R.expect(seeds, c.n_users, agg, exclude_adj=True)
            if len(rank[1]) < 800:
                return fail("guard: the group's candidates", len(rank[1]))
            if sweep(c, rows, "group %s" % agg,
                     lambda k, m, w, keep: eng.recommend_clubs_group(seeds, k, agg, exclude_adj=True, neighbours=m, window=w, keep_own=keep),
                     rank, own, [None, W(min_score=rank[1][200]), W(min_score=f32(1.0))], ms=(10, 65, 0)):
                return 1
        # G = 1 equals the by-uid list
        for i in (441, 1):
            u = ec.uid_of(i)
            rank = ref.ranking(u)[:2]
            if sweep(c, rows, "G = 1, %d" % u,
                     lambda k, m, w, keep: eng.recommend_clubs_group([u], k, "mean", exclude_adj=True, neighbours=m, window=w, keep_own=keep),
                     rank, cc.own_clubs(c, rows, [u]), [None, W(min_score=0.125)], ms=(64, 0)):
                return 1
        # G = 0
        got = eng.recommend_clubs_group(gr.UNKNOWN_UIDS, 10, window=W(min_score=0.0))
        if len(got[0]) or got[2] != {"total": 0, "used": 0, "contributions": 0, "clubs": 0}:
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
        rows = cc.club_rows(c)
        try:
            for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
                eng.set_scan_kernel(kind)
                for i in (0, 1):
                    u = ec.uid_of(i)
                    if sweep(c, rows, "small %d user %d" % (n, i),
                             lambda k, m, w, keep: eng.recommend_clubs_interest(u, k, neighbours=m, window=w, keep_own=keep),
                             ref.ranking(u)[:2], cc.own_clubs(c, rows, [u]), [None], ms=(1, 0), ks=(3, 100)):
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
    rows = cc.club_rows(c)
    try:
        ref = fchk.Ref(c, orc)
        for u in (8, 1500):
            ids, sc, _ = ref.ranking(u)
            own = cc.own_clubs(c, rows, [u])
            floor = sc[300]
            m = int((sc >= floor).sum())
            if not (64 < m < len(ids)) or len(ids) < n - 1000:
                return fail("guard: the floor passes", m, "of", len(ids))
            for w, nb in ((W(min_score=floor), 0), (None, 0), (None, 5000)):
                want = cc.expect(c, rows, cut((ids, sc), w), own, nb, 25)
                if w is None and nb == 0 and want[2]["contributions"] < 10000:
                    return fail("guard: the whole window's contributions", want[2])
                if check(("big", u, nb), eng.recommend_clubs_interest(u, 25, neighbours=nb, window=w), want):
                    return 1
        print("big ok", N_CASES[0])
        return 0
    finally:
        eng.close()


def check_sticks():
    import ctypes
    c, eng, orc, ref = wchk.open_e()
    rows = cc.club_rows(c)
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

        # before any collecting call the club call leaves "no collecting call has run" as it is
        eng.recommend_clubs_interest(u, 10)
        if code(eng.scan_collected) != pf.PF_EINVAL:
            return fail("a club call left a collected result behind")
        # a window, a collector, stored totals and a collected result in force: all as they were afterwards
        eng.set_scan_window(min_score=0.2, count=True)
        eng.set_scan_collect(700)
        plain = bits(eng.recommend_interest_all(q[:1], 64))
        totals = [int(x) for x in eng.scan_window_totals()]
        coll = eng.scan_collected()
        want = cc.expect(c, rows, ref.ranking(u)[:2], cc.own_clubs(c, rows, [u]), 64, 10)
        for call in (lambda: eng.recommend_clubs_interest(u, 10, neighbours=64),
                     lambda: eng.recommend_clubs_interest(u, 10, neighbours=64, cap=5),            # overflow
                     lambda: eng.recommend_clubs_group(q, 10, window=W(min_score=0.1, count=True)),
                     lambda: eng.recommend_clubs_interest(5, 10)):                                  # unknown uid
            call()
            after = eng.scan_collected()
            if [int(x) for x in eng.scan_window_totals()] != totals or after[2] != coll[2] or not wchk.same(after[:2], coll[:2]):
                return fail("a club call changed the stored totals or the collected result")
            if eng._collect != 700 or eng._window is None or eng._window.fields != (pf.PF_WIN_MIN | pf.PF_WIN_COUNT):
                return fail("a club call changed the binding's state")
        # the context's own window did not leak into the club call, nor the call's into the context
        if check(("under a window in force",), eng.recommend_clubs_interest(u, 10, neighbours=64), want):
            return 1
        if bits(eng.recommend_interest_all(q[:1], 64)) != plain or [int(x) for x in eng.scan_window_totals()] != totals:
            return fail("the plain call after a club call differs")
        after = eng.scan_collected()
        if after[2] != coll[2] or not wchk.same(after[:2], coll[:2]):
            return fail("the collector in force does not collect as before")
        eng.clear_scan_collect()
        eng.clear_scan_window()
        base = bits(eng.recommend_interest_all(q, 64)) + bits(eng.recommend_clubs_collab(q, 10))
        eng.recommend_clubs_interest(u, 10)
        if bits(eng.recommend_interest_all(q, 64)) + bits(eng.recommend_clubs_collab(q, 10)) != base:
            return fail("a result changed after a club call")
        # the refusals
        L, h = eng._L, eng.h
        oc, os_, n = np.zeros(10, np.int32), np.zeros(10, np.float32), np.zeros(1, np.int32)

        def raw(cap=5000, m=0, flags=0, win=None, k=10, out=True, cnt=True, query=True):
            qq = pf.ClubsQuery()
            qq.cap, qq.neighbours, qq.flags = cap, m, flags
            qq.window = None if win is None else ctypes.addressof(win)
            return L.pf_recommend_clubs_interest(h, u, ctypes.byref(qq) if query else None, k, oc.ctypes.data if out else None,
                                                 os_.ctypes.data if out else None, n.ctypes.data if cnt else None, None)
        nan_w = W(min_score=0.5)
        nan_w.min_score = float("nan")
        odd_w = W(min_score=0.5)
        odd_w.fields |= 64
        for name, rc in (("cap 0", raw(cap=0)), ("cap -1", raw(cap=-1)), ("cap 2^31", raw(cap=2**31)), ("m -1", raw(m=-1)),
                         ("flags", raw(flags=2)), ("topk -1", raw(k=-1)), ("null outputs", raw(out=False)),
                         ("null count", raw(cnt=False)), ("null query", raw(query=False)), ("NaN floor", raw(win=nan_w)),
                         ("window bits", raw(win=odd_w))):
            if rc != pf.PF_EINVAL:
                return fail("refusal", name, rc)
        if raw(k=0, out=False) != pf.PF_OK or raw() != pf.PF_OK or n[0] != 10:
            return fail("a good call after the refusals", n[0])
        if code(lambda: eng.recommend_clubs_group(q, 10, agg=7)) != pf.PF_EINVAL or \
                code(lambda: eng.recommend_clubs_group(list(range(1, 1100)), 10)) != pf.PF_EINVAL:
            return fail("the group call's refusals")
        eng.set_shard(0, 2)
        rc = code(lambda: eng.recommend_clubs_interest(u, 10))
        msg = eng._L.pf_last_error(eng.h)
        eng.set_shard(0, 1)
        if rc != pf.PF_EUNSUPP or b"shard" not in msg:
            return fail("a sharded context", rc, msg)
        if eng._window is not None or eng._collect != 0 or code(eng.scan_collected) != pf.PF_OK:
            return fail("state after the refusals")
        if check(("after the refusals",), eng.recommend_clubs_interest(u, 10, neighbours=64), want):
            return 1
        print("sticks ok")
        return 0
    finally:
        eng.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    rc = {"full": check_full, "state": check_state, "profile": check_profile, "group": check_group, "small": check_small,
          "big": check_big, "sticks": check_sticks}[mode]()
    if rc == 0:
        print("ok")
    sys.exit(rc)
