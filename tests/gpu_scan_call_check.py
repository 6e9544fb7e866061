"""Child process of test_gpu_scan_call: what a scan call's options reach when they travel by value
(csrc/pf_scan_call.h) and the synchronous calls share one helper.  On the edge corpus E; argv[1]:
  chunks [stream]  a counted floor over 258 queries, more than one 256-query chunk: by uid (query 256,
                   the first of the second chunk, an unknown uid; the user of query 255 again as 257)
                   and by value (258 clones of those users).  Ids, score bits and all 258 totals.
                   "stream": under PF_SCAN_STREAM (K1); else the automatic choice (K5).
  mixed            one engine, nine calls, each after one of another kind with other options; after
                   them scan_window_totals and scan_collected hold what the last call entitled to
                   store them stored.

Expected values never come from the engine: the oracle's whole ranking (Ref.ranking, GroupRef.expect) cut
by gpu_scan_window_check.cut, and club_corpus.expect over it.  Exits non-zero on any mismatch."""
import sys

import numpy as np

import club_corpus as cc
import edge_corpus as ec
import gpu_scan_window_check as wchk
import group_ref as gr
import pokec_testlib as tl
import query_profile_cases as qc

pf = tl.product()
W = pf.ScanWindow.make
f32 = np.float32
fail, same, cut = wchk.fail, wchk.same, wchk.cut
UNKNOWN = 5          # no profile in E (group_ref.UNKNOWN_UIDS)
CHUNK = 256          # queries per launch of the synchronous calls


def check_chunks(stream):
    c, eng, orc, ref = wchk.open_e()
    try:
        if stream:
            eng.set_scan_kernel(pf.PF_SCAN_STREAM)
        if eng.layout().scan_kernel != (1 if stream else 2):
            return fail("scan kernel", eng.layout().scan_kernel)
        k = 10
        w = W(min_score=0.2, count=True)
        users = [ec.uid_of(i) for i in (441, 1, 30, ec.EMPTY_USER, ec.EXCL_CLONES_Q, 62, 466, 515, 700, 1020, 766)]
        q = [users[i % len(users)] for i in range(CHUNK + 2)]
        q[CHUNK + 1] = q[CHUNK - 1]   # one user on both sides of the chunk boundary
        want = {u: cut(ref.ranking(u)[:2], w) for u in users}
        sizes = sorted(len(v[0]) for v in want.values())
        if not (any(200 <= n <= 900 for n in sizes) and sizes[0] == 0 and len(set(sizes)) >= 4):
            return fail("guard: the floor's window sizes", sizes)
        # by uid: query 256 unknown
        qu = list(q)
        qu[CHUNK] = UNKNOWN
        got = eng.recommend_interest_all(qu, k, window=w)
        tot = [int(x) for x in eng.scan_window_totals()]
        if len(got) != len(qu) or len(tot) != len(qu):
            return fail("by uid: rows", len(got), len(tot))
        for i, u in enumerate(qu):
            ids, sc = want[u] if u != UNKNOWN else (np.zeros(0, np.int32), np.zeros(0, f32))
            if not same(got[i], (ids[:k], sc[:k])) or tot[i] != len(ids):
                return fail("by uid: query", i, "uid", u, "got", list(got[i][0][:4]), tot[i], "want", list(ids[:4]), len(ids))
        # by value: clones of the same users, the unknown one replaced by a clone
        clones = {u: qc.clone_profile(pf, c, u) for u in users}
        got = eng.recommend_profile([clones[u] for u in q], k, window=w)
        tot = [int(x) for x in eng.scan_window_totals()]
        if len(got) != len(q) or len(tot) != len(q):
            return fail("by value: rows", len(got), len(tot))
        for i, u in enumerate(q):
            ids, sc = want[u]
            if not same(got[i][:2], (ids[:k], sc[:k])) or tot[i] != len(ids):
                return fail("by value: query", i, "uid", u, "got", list(got[i][0][:4]), tot[i], "want", list(ids[:4]), len(ids))
        if eng._window is not None:
            return fail("window= left a window in force")
        print("chunks ok", "stream" if stream else "auto", sizes)
        return 0
    finally:
        eng.close()


def check_mixed():
    import torch
    c, eng, orc, ref = wchk.open_e(want_kernel=2)
    rows = cc.club_rows(c)
    try:
        R = gr.GroupRef(c, orc.fas_pairs)
        u441, u1, u30 = ec.uid_of(441), ec.uid_of(1), ec.uid_of(30)
        r441, r1, r30 = ref.ranking(u441)[:2], ref.ranking(u1)[:2], ref.ranking(u30)[:2]
        seeds = gr.uids(gr.SEEDS_MIXED)
        totals, collected = None, None   # what the context should hold

        def stored(tag):
            t = [int(x) for x in eng.scan_window_totals()] if totals is not None else None
            if t != totals:
                return fail(tag, "scan_window_totals", t, "want", totals)
            if collected is not None:
                ci, cs, ct = eng.scan_collected()
                if ct != collected[2] or not same((ci, cs), collected[:2]):
                    return fail(tag, "scan_collected", ct, len(ci), "want", collected[2], len(collected[0]))
            if eng._window is not None or eng._collect != 0 or eng._filter is not None:
                return fail(tag, "an option stayed in force")
            return 0

        def context_plain(tag):
            """The context itself, not the binding's record of it: a plain call of two uids is served (a
            collector left in the context would refuse it) with the unwindowed lists (a window left there
            would cut them), and stores nothing."""
            got = eng.recommend_interest_all([u1, u441], 10)
            if not same(got[0], (r1[0][:10], r1[1][:10])) or not same(got[1], (r441[0][:10], r441[1][:10])):
                return fail(tag, "a plain call of two uids after it")
            return stored(tag + ", then a plain call")

        # 1. by uid, two queries, a counted floor
        w = W(min_score=wchk.TIE_1, count=True)
        got = eng.recommend_interest_all([u1, u441], 10, window=w)
        want = [cut(r1, w), cut(r441, w)]
        if not all(same(g, (x[0][:10], x[1][:10])) for g, x in zip(got, want)):
            return fail("1: by uid under a counted floor")
        totals = [len(x[0]) for x in want]
        if stored("1"):
            return 1
        # 2. collecting by profile, another floor, no count: the totals stay
        w = W(min_score=0.125)
        got = eng.recommend_profile(qc.clone_profile(pf, c, u30), 64, window=w, collect=2000)[0]
        ids, sc = cut(r30, w)
        if not (64 < len(ids) <= 2000) or not same(got[:2], (ids[:64], sc[:64])):
            return fail("2: collecting by profile", len(ids))
        collected = (ids, sc, len(ids))
        if stored("2"):
            return 1
        # 3. clubs by group, a window of its own with PF_WIN_COUNT set: nothing stored
        rank = R.expect(seeds, c.n_users, "max", exclude_adj=True)
        w = W(min_score=rank[1][200], count=True)
        got = eng.recommend_clubs_group(seeds, 10, "max", exclude_adj=True, neighbours=65, window=w)
        if not cc.same(got, cc.expect(c, rows, cut(rank, w), cc.own_clubs(c, rows, seeds), 65, 10)):
            return fail("3: clubs by group", got[2])
        if stored("3") or context_plain("3"):
            return 1
        # 4. scan_keys_async on a stream of the caller's, a plain top-10
        s = torch.cuda.Stream()
        keys = torch.full((1, 10), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.scan_keys_async([u441], 10, keys.data_ptr(), s.cuda_stream)
        s.synchronize()
        if not same(pf.decode_keys(keys.cpu().numpy().view(np.uint64)[0]), (r441[0][:10], r441[1][:10])):
            return fail("4: scan_keys_async")
        if stored("4"):
            return 1
        # 5. collecting by uid, overflowing by one: the exact total and no keys
        w = W(min_score=0.125, after=(r1[1][50], int(r1[0][50])))
        ids, sc = cut(r1, w)
        got = eng.recommend_interest_all([u1], 10, window=w, collect=len(ids) - 1)[0]
        if len(ids) < 500 or not same(got, (ids[:10], sc[:10])):
            return fail("5: an overflowing collect", len(ids))
        collected = (ids[:0], sc[:0], len(ids))
        if stored("5"):
            return 1
        # 6. a collecting call of two uids is refused and stores nothing
        try:
            eng.recommend_interest_all([u1, u441], 10, window=W(min_score=0.3, count=True), collect=100)
            return fail("6: two uids with a collector were served")
        except pf.FasError as e:
            if e.code != pf.PF_EUNSUPP or b"collect" not in eng._L.pf_last_error(eng.h):
                return fail("6: refusal", e.code, eng._L.pf_last_error(eng.h))
        if stored("6"):
            return 1
        # 7. a counted group
        rank = R.expect(seeds, c.n_users, "mean", exclude_adj=True)
        w = W(min_score=rank[1][300], count=True)
        ids, sc = cut(rank, w)
        got = eng.recommend_group(seeds, 64, "mean", exclude_adj=True, window=w)
        if len(ids) < 301 or not same(got, (ids[:64], sc[:64])):
            return fail("7: counted group", len(ids))
        totals = [len(ids)]
        if stored("7"):
            return 1
        # 8. clubs by uid, no window
        got = eng.recommend_clubs_interest(u441, 10, neighbours=64)
        if not cc.same(got, cc.expect(c, rows, r441, cc.own_clubs(c, rows, [u441]), 64, 10)):
            return fail("8: clubs by uid", got[2])
        if stored("8") or context_plain("8"):
            return 1
        # 9. a plain batch of three with an unknown uid
        got = eng.recommend_interest_all([u30, UNKNOWN, u1], 10)
        if not same(got[0], (r30[0][:10], r30[1][:10])) or len(got[1][0]) != 0 or not same(got[2], (r1[0][:10], r1[1][:10])):
            return fail("9: plain batch")
        if stored("9"):
            return 1
        print("mixed ok")
        return 0
    finally:
        eng.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    rc = check_mixed() if mode == "mixed" else check_chunks(len(sys.argv) > 2 and sys.argv[2] == "stream")
    if rc == 0:
        print("ok")
    sys.exit(rc)
