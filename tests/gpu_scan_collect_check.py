"""Child process of test_gpu_scan_collect: the engine reads PF_DEBUG once per process, so each launch
shape runs in its own.  argv[1] picks the check:
  full      the one-query scan (K5, or K1 under PF_DEBUG scan=stream): the guard facts, then the whole
            window collected with no window, under floors (the query's own scores, the tie values and
            their float neighbours, around 2^-3, below it, above everybody), a floor and a cursor, a
            cursor alone, for queries 441, 1, 30, EMPTY_USER and EXCL_CLONES_Q
  caps      cap = total, total + 1, total - 1 and 1 on a floored and a tie case; cap 0 clears
  state     the wide store, a candidate filter, a field selection, three shards merged on the host,
            explain=True
  profile   recommend_profile, E's own users given by value with their exclude lists
  group     recommend_group: G = 5 under mean / min / max with exclude_adj, G = 1, G = 0; run again by the
            parent under PF_DEBUG group_tile=1 (a pass per seed)
  small     E cut to 2, 511, 512, 513 and 1025 users: everyone collected for user 0
  big       the seeded 20,000-user synthetic corpus: three queries under K5 and K1, a floor a few hundred
            pass and no window at all (everybody but the user and its adjacency row: some 19,700 keys from many workgroups, cap exact)
  sticks    the refusals; nothing sticks to the context

The oracle has no collector.  The expected list of a case is the oracle's whole ranking of the query
(Ref.ranking), cut in numpy to the filter and the window (gpu_scan_window_check.cut): ids and float32
bits must be equal, the total exact and the order exact.  Every case also makes the same call with no
collector and asks that the call's own ids, scores and count are the same with one, and under
count=True that scan_window_totals() is the total.  Exits non-zero on any mismatch."""
import os
import sys
import tempfile

import numpy as np

import edge_corpus as ec
import gpu_scan_filter_check as fchk
import gpu_scan_window_check as wchk
import pokec_testlib as tl

pf = tl.product()
W = pf.ScanWindow.make
f32 = np.float32
fail, same, cut, up, down = wchk.fail, wchk.same, wchk.cut, wchk.up, wchk.down
TIES = {441: wchk.TIE_441, 1: wchk.TIE_1, 30: wchk.TIE_30}
N_CASES = [0]


class Subject:
    """One ranked list: call(k, window, collect) -> (ids, scores) makes the engine call, rank is the
    reference's whole ranking (already cut to the filter / selection / shard of the subject)."""

    def __init__(self, eng, name, call, rank):
        self.eng, self.name, self.call = eng, name, call
        self.rank = (np.asarray(rank[0]), np.asarray(rank[1], np.float32))


def by_uid(eng, ref, u, name=None, **kw):
    return Subject(eng, name or "uid %d" % u,
                   lambda k, w, col: eng.recommend_interest_all([u], k, window=w, collect=col, **kw)[0][:2], ref.ranking(u)[:2])


def check_collect(S, w=None, k=10, cap=None, count=False):
    """One case.  cap=None: the window's exact size (at least 1).  Returns 0, or 1 after a message."""
    eng = S.eng
    ids, sc = cut(S.rank, w)
    total = len(ids)
    wc = w
    if count:
        wc = pf.ScanWindow() if w is None else w.copy()
        wc.fields |= pf.PF_WIN_COUNT
    plain = S.call(k, wc, None)
    cap = max(total, 1) if cap is None else cap
    got = S.call(k, wc, cap)
    tag = (S.name, "window", None if w is None else (w.fields, w.min_score, w.after_score, w.after_uid), "k", k, "cap", cap)
    if eng._collect != 0:
        return fail(*tag, "collect= left a collector in force")
    if not same(got, plain) or not same(got, (ids[:k], sc[:k])):
        return fail(*tag, "the call's own list: got", list(got[0][:4]), len(got[0]), "want", list(ids[:4]), min(k, total))
    if count and int(eng.scan_window_totals()[0]) != total:
        return fail(*tag, "scan_window_totals", int(eng.scan_window_totals()[0]), "numpy", total)
    cids, csc, ctot = eng.scan_collected()
    if ctot != total:
        return fail(*tag, "total", ctot, "numpy", total)
    if total > cap:
        if len(cids) != 0 or len(csc) != 0:
            return fail(*tag, "overflow returned", len(cids), "entries")
    elif not same((cids, csc), (ids, sc)):
        bad = next((j for j in range(min(len(cids), total)) if int(cids[j]) != int(ids[j]) or f32(csc[j]).view(np.uint32) != sc[j].view(np.uint32)), -1)
        return fail(*tag, "collected", len(cids), "of", total, "first difference at rank", bad)
    N_CASES[0] += 1
    return 0


def floors_of(S, i):
    sc = S.rank[1]
    fl = [sc[j] for j in (0, 9, 63) if j < len(sc)]
    fl += [f32(0.125), up(0.125), down(0.125), f32(0.1), f32(0.36)]
    if i in TIES:
        fl += [TIES[i], up(TIES[i]), down(TIES[i])]
    return fl


def check_full():
    c, eng, orc, ref = wchk.open_e()
    try:
        if wchk.check_guards(ref):
            return 1
        n = 0
        for i in wchk.Q_IDX:
            S = by_uid(eng, ref, ec.uid_of(i))
            ids, sc = S.rank
            if check_collect(S, None, 10, count=False) or check_collect(S, None, 64, count=True):  # everyone, unpruned
                return 1
            for fl in floors_of(S, i):
                n += 1
                if check_collect(S, W(min_score=fl), (10, 64)[n & 1], count=bool(n & 2)):
                    return 1
            if len(cut(S.rank, W(min_score=0.36))[0]) != 0:
                return fail("guard: somebody scores 0.36 or more", i)
            # a floor and a cursor together; a cursor alone (a member, and nobody: E's uids are 7 or more apart)
            a = (sc[100], int(ids[100]))
            b = (sc[len(ids) // 2], int(ids[len(ids) // 2]) + 3)
            for w in (W(min_score=sc[400], after=a), W(min_score=0.125, after=a), W(after=a), W(after=b),
                      W(after=(sc[-1], int(ids[-1])))):
                n += 1
                if check_collect(S, w, (10, 64)[n & 1], count=bool(n & 2)):
                    return 1
            if i in TIES:  # a cursor inside the tie, a floor at it: the rest of the tie, by uid alone
                tie = np.sort(ids[sc == TIES[i]])
                if check_collect(S, W(min_score=TIES[i], after=(TIES[i], int(tie[len(tie) // 2]))), 64, count=True):
                    return 1
        print("full:", N_CASES[0], "collected windows")
        return 0
    finally:
        eng.close()


def check_caps():
    c, eng, orc, ref = wchk.open_e()
    try:
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            for i, w in ((441, W(min_score=0.125)), (1, W(min_score=wchk.TIE_1, after=(wchk.TIE_1, -2**31)))):
                S = by_uid(eng, ref, ec.uid_of(i))
                total = len(cut(S.rank, w)[0])
                if total < 500:
                    return fail("guard: the cap cases' windows hold", total)
                for cap in (total, total + 1, total - 1, 1):
                    if check_collect(S, w, 10, cap=cap, count=(cap == 1)):
                        return 1
                # after an overflow (cap = total - 1) the next, larger collector returns the right list: the
                # overflowing scan stored nothing the next one could mistake for its own
                if check_collect(S, w, 64, cap=total - 1) or check_collect(S, w, 64, cap=2 * total):
                    return 1
                # ... and a smaller window after a larger one leaves nothing of the larger behind
                if check_collect(S, W(min_score=S.rank[1][9]), 10, cap=2 * total):
                    return 1
            # a collector set on the context (not per call) serves call after call; cap 0 clears
            u = ec.uid_of(441)
            S = by_uid(eng, ref, u)
            eng.set_scan_collect(2000)
            for w in (W(min_score=0.125), None, W(min_score=wchk.TIE_441, count=True)):
                eng.recommend_interest_all([u], 10, window=w)
                ids, sc = cut(S.rank, w)
                cids, csc, ctot = eng.scan_collected()
                if ctot != len(ids) or not same((cids, csc), (ids, sc)):
                    return fail("a collector in force", ctot, len(ids))
            eng.set_scan_collect(0)
            before = eng.scan_collected()
            eng.recommend_interest_all([u], 10, window=W(min_score=0.2))
            after = eng.scan_collected()
            if eng._collect != 0 or after[2] != before[2] or not same(after, before):
                return fail("cap 0 did not clear the collector")
        print("caps ok")
        return 0
    finally:
        eng.close()


def check_state():
    import gpu_group_check as ggc
    import group_ref as gr
    # the wide store, K5 and K1
    c, eng, orc, ref = wchk.open_e(ggc.wide_e())
    try:
        if eng.layout().packed_tokens != 0:
            return fail("store format")
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            for i in (441, 1):
                S = by_uid(eng, ref, ec.uid_of(i), "wide %d" % i)
                if check_collect(S, None, 10) or check_collect(S, W(min_score=TIES[i]), 64, count=True) or \
                        check_collect(S, W(min_score=0.125, after=(S.rank[1][50], int(S.rank[0][50]))), 10):
                    return 1
    finally:
        eng.close()
    c, eng, orc, ref = wchk.open_e()
    try:
        u1, u441 = ec.uid_of(1), ec.uid_of(441)
        # a candidate filter: reference = filter mask and window
        filt = pf.CandFilter.make(gender=1)
        mask = fchk.np_pass(c, filt)
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            for u in (u1, u441):
                ids, sc, idx = ref.ranking(u)
                S = by_uid(eng, ref, u, "filter %d" % u, filter=filt)
                S.rank = (ids[mask[idx]], sc[mask[idx]])
                if len(S.rank[0]) < 200:
                    return fail("the filter leaves too few candidates", len(S.rank[0]))
                if check_collect(S, None, 64, count=True) or check_collect(S, W(min_score=0.125), 10) or \
                        check_collect(S, W(min_score=S.rank[1][70]), 10, count=True):
                    return 1
        eng.set_scan_kernel(pf.PF_SCAN_POSTINGS)
        if eng._filter is not None or eng._window is not None or eng._collect != 0:
            return fail("the filter / window / collector in force before the call was not restored")
        # a field selection: reference scores from fas_pairs(select=)
        sel = pf.FieldSelect.make(fixed=0x7F & ~((1 << pf.PF_F_AGE) | (1 << pf.PF_F_CLUBS)),
                                  cols=[t for t in range(ec.N_COLS) if t != ec.COL_L])
        Rs = gr.GroupRef(c, lambda a, b: eng.fas_pairs(a, b, select=sel))
        for u in (u1, u441):
            S = by_uid(eng, ref, u, "select %d" % u, select=sel)
            S.rank = Rs.expect([u], c.n_users, "mean", exclude_adj=True)
            if check_collect(S, None, 10) or check_collect(S, W(min_score=S.rank[1][70]), 64, count=True):
                return 1
        # three shards: each shard's list is the shard's, merged on the host they are the unsharded list
        for u in (u1, u441):
            rank = ref.ranking(u)[:2]
            for w in (None, W(min_score=0.125), W(min_score=TIES[1 if u == u1 else 441], after=(rank[1][100], int(rank[0][100])))):
                ids, sc = cut(rank, w)
                parts, tot = [], 0
                for sh in range(3):
                    eng.set_shard(sh, 3)
                    own = eng.recommend_interest_all([u], 10, window=w, collect=len(ids) + 1)[0]
                    ci, cs, ct = eng.scan_collected()
                    if ct != len(ci) or not same(own, (ci[:10], cs[:10])):
                        return fail("shard", sh, "its own top-k is not the head of its list")
                    parts.append((ci, cs))
                    tot += ct
                eng.set_shard(0, 1)
                if tot != len(ids) or not same(fchk.merged(parts, len(ids)), (list(ids), sc)):
                    return fail("shards", u, tot, len(ids))
                # (the shards are cut by weight: one of E's three may be empty, which is a case of its own)
                if w is None and sum(1 for p in parts if len(p[0]) > 64) < 2:
                    return fail("guard: fewer than two shards with more than 64 candidates", [len(p[0]) for p in parts])
        # explain=True with a collector: the breakdown of the call's list, the whole window beside it
        rank = ref.ranking(u1)[:2]
        for w in (W(min_score=0.15), None):
            ids, sc = cut(rank, w)
            got = eng.recommend_interest_all([u1], 10, window=w, explain=True, collect=len(ids))[0]
            if len(got) != 3 or not same(got[:2], (ids[:10], sc[:10])) or len(got[2]) != len(got[0]):
                return fail("explain with a collector")
            if not np.array_equal(np.asarray(got[2].score, np.float32).view(np.uint32), np.asarray(got[1], np.float32).view(np.uint32)):
                return fail("explain with a collector: the breakdown's scores")
            ci, cs, ct = eng.scan_collected()
            if ct != len(ids) or not same((ci, cs), (ids, sc)):
                return fail("explain with a collector: the collected list")
        print("state ok")
        return 0
    finally:
        eng.close()


def check_profile():
    import query_profile_cases as qc
    c, eng, orc, ref = wchk.open_e()
    try:
        for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
            eng.set_scan_kernel(kind)
            for i in (441, 1):
                u = ec.uid_of(i)
                p = qc.clone_profile(pf, c, u)  # excludes adj[u] + {u}, by its own exclude list
                S = Subject(eng, "profile %d" % u, lambda k, w, col: eng.recommend_profile(p, k, window=w, collect=col)[0][:2],
                            ref.ranking(u)[:2])
                if check_collect(S, None, 64, count=True) or check_collect(S, W(min_score=0.125), 10) or \
                        check_collect(S, W(min_score=TIES[i]), 10, count=True) or check_collect(S, W(min_score=0.36), 10) or \
                        check_collect(S, W(min_score=0.125), 10, cap=7):
                    return 1
        eng.set_scan_kernel(pf.PF_SCAN_POSTINGS)
        p = qc.clone_profile(pf, c, ec.uid_of(1))
        got = eng.recommend_profile(p, 10, window=W(min_score=0.125), explain=True, collect=2000)[0]
        ids, sc = cut(ref.ranking(ec.uid_of(1))[:2], W(min_score=0.125))
        if len(got) != 3 or not same(got[:2], (ids[:10], sc[:10])) or not same(eng.scan_collected()[:2], (ids, sc)):
            return fail("profile, explain with a collector")
        print("profile ok")
        return 0
    finally:
        eng.close()


def check_group():
    import group_ref as gr
    c, eng, orc, ref = wchk.open_e(want_kernel=2)
    try:
        R = gr.GroupRef(c, orc.fas_pairs)
        seeds = gr.uids(gr.SEEDS_MIXED)  # G = 5
        plan = eng.group_plan(seeds, exclude_adj=True)
        print("plan", plan.n_seeds, "seeds", plan.n_passes, "passes")
        if "group_tile=1" in os.environ.get("PF_DEBUG", "") and plan.n_passes != 5:
            return fail("guard: group_tile=1 did not give a pass per seed", plan.n_passes)
        for agg in gr.AGGS:
            S = Subject(eng, "group %s" % agg,
                        lambda k, w, col: eng.recommend_group(seeds, k, agg, exclude_adj=True, window=w, collect=col),
                        R.expect(seeds, c.n_users, agg, exclude_adj=True))
            sc = S.rank[1]
            if len(sc) < 800:
                return fail("guard: the group's candidates", len(sc))
            for w, k, cnt in ((None, 64, True), (W(min_score=sc[9]), 10, False), (W(min_score=sc[200]), 64, True),
                              (W(min_score=up(sc[200])), 10, False), (W(min_score=sc[700], after=(sc[150], int(S.rank[0][150]))), 10, True),
                              (W(min_score=f32(1.0)), 10, True)):
                if check_collect(S, w, k, count=cnt):
                    return 1
            if check_collect(S, W(min_score=sc[200]), 10, cap=100):
                return 1
        # G = 1 equals the by-uid scan
        for i in (441, 1):
            u = ec.uid_of(i)
            S = Subject(eng, "G = 1, %d" % u, lambda k, w, col: eng.recommend_group([u], k, "mean", exclude_adj=True, window=w, collect=col),
                        ref.ranking(u)[:2])
            if check_collect(S, None, 10) or check_collect(S, W(min_score=TIES[i]), 64, count=True):
                return 1
        # G = 0: nothing, and a total of 0
        got = eng.recommend_group(gr.UNKNOWN_UIDS, 10, window=W(min_score=0.0), collect=10)
        ci, cs, ct = eng.scan_collected()
        if len(got[0]) != 0 or ct != 0 or len(ci) != 0:
            return fail("G = 0 with a collector")
        print("group ok")
        return 0
    finally:
        eng.close()


def check_small():
    for n in (2, 511, 512, 513, 1025):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        c, eng, orc, ref = wchk.open_e(c)
        try:
            for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
                eng.set_scan_kernel(kind)
                # (at n = 2 user 0's only other user is in its adjacency row: an empty ranking; user 1 has one)
                S = by_uid(eng, ref, ec.uid_of(0))
                if n > 2 and len(S.rank[0]) < 500:
                    return fail("small", n, "user 0 has too few candidates", len(S.rank[0]))
                if check_collect(S, None, 3, count=True) or check_collect(by_uid(eng, ref, ec.uid_of(1)), None, 3):
                    return fail("small", n, kind)
        finally:
            eng.close()
    print("small ok")
    return 0


def check_big():
    n = 20000
    sc_ = tl.synth.Corpus(n_users=n, seed=3, edge_cases=1)
    ptr = sc_.desc_ptr()
    c = tl.corpus_from_desc(ptr)
    eng, orc = tl.engine(ptr), tl.Oracle(None, desc_ptr=ptr)
    try:
        ref = fchk.Ref(c, orc)
        for kind, want in ((pf.PF_SCAN_POSTINGS, 2), (pf.PF_SCAN_STREAM, 1)):
            eng.set_scan_kernel(kind)
            if eng.layout().scan_kernel != want:
                return fail("big: scan kernel", eng.layout().scan_kernel)
            for u in (8, 1500, 19999):
                S = by_uid(eng, ref, u)
                ids, sc = S.rank
                floor = sc[300]
                m = int((sc >= floor).sum())
                # (everybody but the user and its adjacency row: a few hundred short of n)
                if not (64 < m < len(ids)) or len(ids) < n - 1000:
                    return fail("guard: the floor passes", m, "of", len(ids))
                if check_collect(S, W(min_score=floor), 10, count=True) or check_collect(S, None, 64):
                    return 1
                if check_collect(S, W(min_score=floor), 64, cap=m - 1):
                    return 1
        print("big ok")
        return 0
    finally:
        eng.close()


def check_sticks():
    c, eng, orc, ref = wchk.open_e()
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
        if code(eng.scan_collected) != pf.PF_EINVAL:
            return fail("scan_collected before any collecting call")
        before = snapshot()
        eng.set_scan_collect(500)
        # FoF interest, collab, clubs, the pair call and scan_bytes never see the collector
        for name, fn, want in (("fof", lambda: bits(eng.recommend_graph_registration(q, 10)), before[1]),
                               ("collab", lambda: bits(eng.recommend_collaborative(q, 10)), before[2]),
                               ("clubs", lambda: bits(eng.recommend_clubs_collab(q, 10)), before[3]),
                               ("pairs", lambda: list(np.asarray(eng.fas_pairs(q, list(reversed(q))), np.float32).view(np.uint32)), before[4]),
                               ("scan_bytes", lambda: list(eng.scan_bytes(q)), before[5])):
            if fn() != want:
                return fail("a call that does not read the collector changed under it", name)
        if code(eng.scan_collected) != pf.PF_EINVAL:
            return fail("a call that does not collect left a result")
        # the refusals, each naming the collector
        import torch
        rows = torch.full((1, 10), -1, dtype=torch.int64, device="cuda")
        for name, fn in (("nq = 2", lambda: eng.recommend_interest_all(q[:2], 10)),
                         ("scan_keys_async", lambda: eng.scan_keys_async(q[:1], 10, rows.data_ptr(), 0)),
                         ("topk = 100", lambda: eng.recommend_interest_all(q[:1], 100))):
            if code(fn) != pf.PF_EUNSUPP or b"collect" not in eng._L.pf_last_error(eng.h):
                return fail("refusal", name, eng._L.pf_last_error(eng.h))
        torch.cuda.synchronize()
        # a negative cap (and one above INT32_MAX) is refused, and the collector in force survives
        for bad in (-1, 2**31):
            if eng._L.pf_set_scan_collect(eng.h, bad) != pf.PF_EINVAL:
                return fail("cap", bad, "accepted")
        w = W(min_score=ref.ranking(q[0])[1][99])
        eng.recommend_interest_all(q[:1], 10, window=w)
        ids, sc = cut(ref.ranking(q[0])[:2], w)
        ci, cs, ct = eng.scan_collected()
        if not (100 <= len(ids) <= 500) or ct != len(ids) or not same((ci, cs), (ids, sc)):
            return fail("the collector in force did not survive a refused cap", ct, len(ids))
        # a collecting call the caller asked no count of leaves the stored totals alone
        eng.clear_scan_collect()
        eng.recommend_interest_all(q[:1], 10, window=W(min_score=0.2, count=True))
        t0 = [int(x) for x in eng.scan_window_totals()]
        eng.recommend_interest_all(q[1:2], 10, window=W(min_score=0.125), collect=2000)
        if [int(x) for x in eng.scan_window_totals()] != t0:
            return fail("an uncounted collecting call changed scan_window_totals")
        # collect= restores the collector in force before it
        eng.set_scan_collect(700)
        eng.recommend_interest_all(q[:1], 10, collect=2000)
        if eng._collect != 700:
            return fail("collect= did not restore the collector in force")
        eng.clear_scan_collect()
        if eng._collect != 0 or eng._window is not None or snapshot() != before:
            return fail("a result changed after the collector was cleared")
        if len(eng.recommend_interest_all(q[:1], 100)[0][0]) != 100:
            return fail("topk 100 without a collector")
        # collect_all: a counted call sizes the buffer, one collecting call fills it
        S = by_uid(eng, ref, q[0])
        for w in (None, W(min_score=0.125), W(min_score=0.36)):
            ids, sc = cut(S.rank, w)
            got = pf.collect_all(eng.collect_call(lambda ww, col: eng.recommend_interest_all(q[:1], 1, window=ww, collect=col)), w)
            if got[2] != len(ids) or not same(got[:2], (ids, sc)) or eng._collect != 0 or eng._window is not None:
                return fail("collect_all", got[2], len(ids))
        # an unknown uid: nothing, and a total of 0
        eng.recommend_interest_all([5], 10, collect=10)
        if eng.scan_collected()[2] != 0 or len(eng.scan_collected()[0]) != 0:
            return fail("an unknown uid with a collector")
        print("sticks ok")
        return 0
    finally:
        eng.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    rc = {"full": check_full, "caps": check_caps, "state": check_state, "profile": check_profile, "group": check_group,
          "small": check_small, "big": check_big, "sticks": check_sticks}[mode]()
    if rc == 0:
        print("ok")
    sys.exit(rc)
