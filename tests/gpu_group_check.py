"""Child process of test_gpu_group (the engine reads PF_DEBUG once per process).  argv[1] picks the
check, every comparison is on ids and score bits against tests/group_ref.py:
  anchor    G = 1 with exclude_adj equals recommend_interest_all([u], k)
  model     G in {2, 3, 5, 16, 17, 64, 65, 200}, noisy seed lists, a permutation, 1024 / 1025 seeds
  state     filter, selection, both; shards merged on the host
  scores    group_scores against the scan and against the model
  small     E cut to 2, 511, 512, 513 and 1025 users
  sticks    nothing sticks to the context; the error codes
  variant   the model on a few sets under whatever PF_DEBUG the parent set; argv[2] = wide | packed,
            argv[3] = the n_global the plan must report: none | all | some
  passes    the G = 5 set: prints {"n_passes", "n_global", "lds", "lists"} as one JSON line
Exits non-zero on any mismatch."""
import json
import sys
import tempfile

import numpy as np

import edge_corpus as ec
import group_ref as gr
import pokec_testlib as tl

pf = tl.product()
KS = (1, 10, 64)


def fail(*a):
    print("mismatch", *a, file=sys.stderr)
    return 1


def open_e(c=None):
    c = tl.golden_corpus("E") if c is None else c
    eng, orc = tl.engine(c), tl.Oracle(c)
    return c, eng, orc, gr.GroupRef(c, orc.fas_pairs)


def check_anchor():
    c, eng, orc, R = open_e()
    try:
        n = 0
        for i in sorted(set(ec.PLANTED_QUERIES) | set(ec.CLONE_QUERIES)):
            u = ec.uid_of(i)
            for k in KS:
                want = eng.recommend_interest_all([u], k)[0]
                for agg in gr.AGGS:
                    got = eng.recommend_group([u], k, agg, exclude_adj=True)
                    if not gr.same(got, want):
                        return fail("anchor", i, k, agg, list(got[0][:4]), list(want[0][:4]))
                    n += 1
        print("anchor:", n, "lists")
        return 0
    finally:
        eng.close()
        orc.close()


def model_lists(eng, R, sets, ks=KS, what="model"):
    n = 0
    for name, s in sets.items():
        for agg in gr.AGGS:
            for k in ks:
                for ea in (False, True):
                    got = eng.recommend_group(s, k, agg, exclude_adj=ea)
                    want = R.expect(s, k, agg, exclude_adj=ea)
                    if not gr.same(got, want):
                        return fail(what, name, agg, k, ea, list(got[0][:4]), list(want[0][:4]), got[1][:2], want[1][:2])
                    n += 1
    return -n


def check_model():
    c, eng, orc, R = open_e()
    try:
        sets = gr.model_sets()
        sets["clones"] = gr.uids(gr.SEEDS_CLONES)
        sets["excl"] = gr.uids(gr.SEEDS_EXCL)
        noisy, kept = gr.seeds_with_noise()
        sets["noisy"] = noisy
        sets["n17 reversed"] = list(reversed(sets["n17"]))
        r = model_lists(eng, R, sets)
        if r > 0:
            return r
        if eng.group_plan(noisy).n_seeds != 3 or not gr.same(eng.recommend_group(noisy, 10), eng.recommend_group(kept, 10)):
            return fail("noisy seed list")
        ex = [int(x) for x in R.expect(sets["n16"], 5)[0]] + [gr.UNKNOWN_UIDS[1]]
        if not gr.same(eng.recommend_group(sets["n16"], 10, exclude=ex), R.expect(sets["n16"], 10, exclude=ex)):
            return fail("exclude list")
        if len(eng.recommend_group(gr.UNKNOWN_UIDS, 10)[0]) != 0 or eng.group_plan(gr.UNKNOWN_UIDS).n_passes != 0:
            return fail("G = 0")
        big = [ec.uid_of(i % ec.N_USERS) for i in range(pf.PF_GROUP_MAX_SEEDS)]
        if eng.group_plan(big).n_seeds != pf.PF_GROUP_MAX_SEEDS:
            return fail("1024 seeds: plan")
        if not gr.same(eng.recommend_group(big, 10), R.expect(big, 10)):
            return fail("1024 seeds")
        try:
            eng.recommend_group(big + [ec.uid_of(1399)], 10)
            return fail("1025 seeds accepted")
        except pf.FasError as e:
            if e.code != pf.PF_EINVAL:
                return fail("1025 seeds: code", e.code)
        print("model:", -r, "lists")
        return 0
    finally:
        eng.close()
        orc.close()


def merged(parts, k):
    ids = np.concatenate([p[0] for p in parts])
    sc = np.concatenate([p[1] for p in parts])
    order = np.lexsort((ids, -sc.astype(np.float64)))[:k]
    return ids[order], sc[order]


def check_state():
    c, eng, orc, R = open_e()
    try:
        filt = pf.CandFilter.make(**gr.FILTER_KW)
        mask = gr.np_pass(c, pf, filt)
        sel = pf.FieldSelect.make(fixed=0x7F & ~((1 << pf.PF_F_AGE) | (1 << pf.PF_F_CLUBS)),
                                  cols=[t for t in range(ec.N_COLS) if t != ec.COL_L])
        Rs = gr.GroupRef(c, lambda a, b: eng.fas_pairs(a, b, select=sel))
        sets = {k: v for k, v in gr.model_sets().items() if k in ("pair", "mixed", "n17", "n65")}
        for name, s in sets.items():
            for agg in gr.AGGS:
                for k in (10, 64):
                    for ea in (False, True):
                        if not gr.same(eng.recommend_group(s, k, agg, exclude_adj=ea, filter=filt),
                                       R.expect(s, k, agg, exclude_adj=ea, mask=mask)):
                            return fail("filter", name, agg, k, ea)
                        if not gr.same(eng.recommend_group(s, k, agg, exclude_adj=ea, select=sel),
                                       Rs.expect(s, k, agg, exclude_adj=ea)):
                            return fail("select", name, agg, k, ea)
                        if not gr.same(eng.recommend_group(s, k, agg, exclude_adj=ea, filter=filt, select=sel),
                                       Rs.expect(s, k, agg, exclude_adj=ea, mask=mask)):
                            return fail("filter + select", name, agg, k, ea)
            if eng._filter is not None or eng._select is not None:
                return fail("the context's filter / selection was not restored")
            # the context's own selection is the scan's, as for PF_MODE_ALL
            eng.set_scan_select(sel)
            if not gr.same(eng.recommend_group(s, 10), Rs.expect(s, 10)):
                return fail("context selection", name)
            eng.clear_scan_select()
        for ns in (2, 3):
            for name, s in sets.items():
                for agg in gr.AGGS:
                    parts = []
                    for sh in range(ns):
                        eng.set_shard(sh, ns)
                        parts.append(eng.recommend_group(s, 64, agg, exclude_adj=True))
                    eng.set_shard(0, 1)
                    if sum(len(p[0]) for p in parts) < 64 * ns:
                        return fail("shard returned a short list", ns, name)
                    if not gr.same(merged(parts, 64), eng.recommend_group(s, 64, agg, exclude_adj=True)):
                        return fail("shards", ns, name, agg)
        print("state ok")
        return 0
    finally:
        eng.close()
        orc.close()


def check_scores():
    c, eng, orc, R = open_e()
    try:
        all_u = np.asarray(c.uid, np.int32)
        sel = pf.FieldSelect.make(fixed=0x7F & ~(1 << pf.PF_F_GENDER), cols=[t for t in range(ec.N_COLS) if t != 7])
        for name, s in {k: v for k, v in gr.model_sets().items() if k in ("trio", "mixed", "n16", "n65")}.items():
            for agg in gr.AGGS:
                full = eng.group_scores(s, all_u, agg)
                if not np.array_equal(gr.bits(full), gr.bits(R.scores(s, agg))):
                    return fail("group_scores vs model", name, agg)
                ids, sc = eng.recommend_group(s, 64, agg, exclude=[int(all_u[3])], exclude_adj=True)
                if not np.array_equal(gr.bits(eng.group_scores(s, ids, agg)), gr.bits(sc)):
                    return fail("group_scores of the returned uids", name, agg)
                ok = R.candidates(s, [int(all_u[3])], True)
                idx = np.nonzero(ok)[0]
                top = idx[np.lexsort((all_u[idx], -full[idx].astype(np.float64)))][:64]
                if list(all_u[top]) != list(ids) or not np.array_equal(gr.bits(full[top]), gr.bits(sc)):
                    return fail("top-64 of group_scores vs the scan", name, agg)
            got = eng.group_scores(s, all_u[::5], "mean", select=sel)
            Rs = gr.GroupRef(c, lambda a, b: eng.fas_pairs(a, b, select=sel))
            if not np.array_equal(gr.bits(got), gr.bits(Rs.scores(s, "mean")[::5])):
                return fail("group_scores under a selection", name)
        x = eng.group_scores(gr.uids(gr.SEEDS_PAIR), [int(all_u[0]), gr.UNKNOWN_UIDS[0], int(all_u[1])])
        if not (np.isnan(x[1]) and not np.isnan(x[0]) and not np.isnan(x[2])):
            return fail("NaN for an unknown b_uid")
        if not np.isnan(eng.group_scores(gr.UNKNOWN_UIDS, all_u[:4])).all():
            return fail("NaN for G = 0")
        print("scores ok")
        return 0
    finally:
        eng.close()
        orc.close()


def check_small():
    for n in (2, 511, 512, 513, 1025):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        c, eng, orc, R = open_e(c)
        try:
            everyone = [ec.uid_of(i) for i in range(n)]
            if n <= pf.PF_GROUP_MAX_SEEDS and len(eng.recommend_group(everyone, 10)[0]) != 0:
                return fail("every user a seed", n)
            sets = {"two": everyone[:2], "mixed": [u for u in gr.uids(gr.SEEDS_MIXED) if u in R.pos],
                    "most": everyone[: max(1, min(n - 3, 200))]}
            for name, s in sets.items():
                for agg in gr.AGGS:
                    for k in (1, 64):
                        for ea in (False, True):
                            got, want = eng.recommend_group(s, k, agg, exclude_adj=ea), R.expect(s, k, agg, exclude_adj=ea)
                            if not gr.same(got, want):
                                return fail("small", n, name, agg, k, ea, list(got[0][:4]), list(want[0][:4]))
            if n == 2 and len(eng.recommend_group(everyone[:1], 64)[0]) > 1:
                return fail("k above the candidates")
            if n == 513:
                got = eng.recommend_group(everyone[:500], 64)
                if not (0 < len(got[0]) < 64) or not gr.same(got, R.expect(everyone[:500], 64)):
                    return fail("k above the candidates", n, len(got[0]))
        finally:
            eng.close()
            orc.close()
    print("small ok")
    return 0


def check_sticks():
    c, eng, orc, R = open_e()
    try:
        q = [ec.uid_of(i) for i in ec.PLANTED_QUERIES[::4] + ec.CLONE_QUERIES[:2]]

        def snapshot():
            out = []
            for kind in (pf.PF_SCAN_POSTINGS, pf.PF_SCAN_STREAM):
                eng.set_scan_kernel(kind)
                out.append([(list(i), list(gr.bits(s))) for i, s in eng.recommend_interest_all(q, 64)])
            eng.set_scan_kernel(pf.PF_SCAN_AUTO)
            out.append(list(eng.scan_bytes(q)))
            out.append([(list(i), list(gr.bits(s))) for i, s in eng.recommend_collaborative(q[:4], 20)])
            out.append(list(gr.bits(eng.fas_pairs(q, list(reversed(q))))))
            return out
        before = snapshot()
        ref = orc.interest(q, 64, tl.PF_MODE_ALL, 0)
        for (i, s), r in zip(before[0], ref):
            if i != list(r[0]) or s != list(gr.bits(r[1])):
                return fail("by-uid lists differ from the oracle before any group call")
        filt = pf.CandFilter.make(**gr.FILTER_KW)
        for name, s in gr.model_sets().items():
            for agg in gr.AGGS:
                eng.recommend_group(s, 64, agg, exclude_adj=True, filter=filt)
                eng.recommend_group(s, 10, agg, exclude=s[:1])
            eng.group_scores(s, q)
            eng.group_plan(s)
        if snapshot() != before:
            return fail("a by-uid result changed after group calls")

        def code(fn):
            try:
                fn()
                return pf.PF_OK
            except pf.FasError as e:
                return e.code
        s = gr.uids(gr.SEEDS_PAIR)
        g = pf.GroupQuery.make(s)
        g.agg = 3
        bad_agg = code(lambda: eng._check(eng._L.pf_group_plan_of(eng.h, g, pf.GroupPlan()), "x"))
        g = pf.GroupQuery.make(s)
        g.flags = 2
        bad_flag = code(lambda: eng._check(eng._L.pf_group_plan_of(eng.h, g, pf.GroupPlan()), "x"))
        g = pf.GroupQuery.make(s)
        g.seed_uid = None
        null_arr = code(lambda: eng._check(eng._L.pf_group_plan_of(eng.h, g, pf.GroupPlan()), "x"))
        topk65 = code(lambda: eng.recommend_group(s, 65))
        many = code(lambda: eng.recommend_group(s, 10, exclude=list(range(3_000_000, 3_000_000 + 30000))))
        all_users = [int(u) for u in c.uid]
        known = code(lambda: eng.recommend_group(s, 10, exclude=all_users))
        if (bad_agg, bad_flag, null_arr) != (pf.PF_EINVAL,) * 3:
            return fail("PF_EINVAL codes", bad_agg, bad_flag, null_arr)
        if topk65 != pf.PF_EUNSUPP:
            return fail("topk 65", topk65)
        if many != pf.PF_OK or known != pf.PF_OK:   # unknown uids are ignored; 1,400 known ones fit
            return fail("exclusion lists", many, known)
        if snapshot() != before:
            return fail("a by-uid result changed after refused calls")
        print("sticks ok")
        return 0
    finally:
        eng.close()
        orc.close()


def wide_e():
    """E with ids at and above 2^30 (test_gpu_edge_domain's _edit_ids_2_30, restated): the wide store."""
    c = tl.golden_corpus("E")
    clubs, friends = c.clubs.copy(), c.friends.copy()
    assert (clubs == ec.ID_TOP).sum() >= 2 and (friends == ec.ID_TOP).sum() >= 2
    clubs[clubs == ec.ID_TOP] = 2**30
    friends[friends == ec.ID_TOP] = 2**31 + 7
    f = dict(uid=c.uid, pub=c.pub, comp=c.comp, gen=c.gen, age=c.age, region=c.region, club_off=c.club_off, clubs=clubs,
             friend_off=c.friend_off, friends=friends, tok_off=c.tok_off, tok_tid=c.tok_tid, tok_tf=c.tok_tf,
             adj_uid=c.adj_uid, adj_off=c.adj_off, adj_nbr=c.adj_nbr)
    return tl.Corpus(n_cols=c.n_cols, norm_present=c.norm_present.copy(), norm_mean=c.norm_mean.copy(),
                     norm_sd=c.norm_sd.copy(), median=c.median, col_names=c.col_names,
                     **{k: np.array(v, copy=True) for k, v in f.items()})


def check_variant(store, want_global):
    c, eng, orc, R = open_e(wide_e() if store == "wide" else None)
    try:
        if eng.layout().packed_tokens != (0 if store == "wide" else 1):
            return fail("store format", store)
        sets = {k: v for k, v in gr.model_sets().items() if k in ("pair", "mixed", "n17", "n65")}
        sets["set users"] = gr.uids(sorted(ec.SET_USERS) + [ec.SET_PARTNER, ec.SET_TOP])
        sets["clones"] = gr.uids(gr.SEEDS_CLONES)
        for name, s in sets.items():
            p = eng.group_plan(s)
            ok = {"none": p.n_global == 0, "all": p.n_global == p.n_seeds, "some": 0 < p.n_global < p.n_seeds,
                  "any": True}[want_global]
            if not ok and name in ("mixed", "n17", "n65"):
                return fail("n_global", name, p.n_global, p.n_seeds, want_global)
        r = model_lists(eng, R, sets, ks=(10, 64), what="variant")
        if r > 0:
            return r
        filt = pf.CandFilter.make(**gr.FILTER_KW)
        mask = gr.np_pass(c, pf, filt)
        s = sets["n17"]
        if not gr.same(eng.recommend_group(s, 64, "min", filter=filt), R.expect(s, 64, "min", mask=mask)):
            return fail("variant under the filter")
        print("variant ok:", -r, "lists")
        return 0
    finally:
        eng.close()
        orc.close()


def check_passes():
    c, eng, orc, R = open_e()
    try:
        s = gr.uids(gr.SEEDS_MIXED)
        p = eng.group_plan(s)
        lds, fixed, budget = eng.group_image_lds(s)
        lists = {}
        for agg in gr.AGGS:
            for k in KS:
                for ea in (False, True):
                    ids, sc = eng.recommend_group(s, k, agg, exclude_adj=ea)
                    want = R.expect(s, k, agg, exclude_adj=ea)
                    if not gr.same((ids, sc), want):
                        return fail("passes vs model", agg, k, ea)
                    lists["%s %d %d" % (agg, k, ea)] = [[int(x) for x in ids], [int(x) for x in gr.bits(sc)]]
        lay = eng.layout()
        print(json.dumps({"n_passes": p.n_passes, "n_global": p.n_global, "n_seeds": p.n_seeds, "stream_bytes": int(p.stream_bytes),
                          "layout_bytes": int(lay.stream_bytes + lay.header_bytes), "lds": [int(x) for x in lds], "fixed": fixed,
                          "budget": budget, "lists": lists}))
        return 0
    finally:
        eng.close()
        orc.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    rc = {"anchor": check_anchor, "model": check_model, "state": check_state, "scores": check_scores, "small": check_small,
          "sticks": check_sticks, "passes": check_passes,
          "variant": lambda: check_variant(*sys.argv[2:4])}[mode]()
    if rc == 0:
        print("ok")
    sys.exit(rc)
