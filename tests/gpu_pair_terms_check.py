"""Child process of test_gpu_pair_terms: the engine reads PF_DEBUG once per process.  argv[1] picks
the check: `pairs` (E's planted pairs), `shapes` (wave and workgroup edges, many queries, unknown
uids, a 2-user corpus), `select` (the breakdown under selections), `gtab` (E plus the user whose
table is probed in global memory), `wide` (E with set ids past the packed store's limit) or
`explain` (recommend_interest_all(explain=True)).

The reference for a term is tests/pair_terms_ref.py: the single-field oracles give each slot's
presence and the float32 bits of its FAS; the whole score must have the base oracle's bits and be
the row's own sequential sum.  Exits non-zero on any mismatch."""
import os
import sys
import tempfile

import numpy as np

import edge_corpus as ec
import field_select_ref as fsr
import gpu_field_select_check as fs_chk
import pair_terms_ref as ptr
import pokec_testlib as tl

pf = tl.product()
S = pf.FieldSelect.make
bits = ptr.bits
ALL_COLS = list(range(ec.N_COLS))


def fail(*a):
    print("mismatch", *a, file=sys.stderr)
    return 1


def without(*cols):
    return [t for t in ALL_COLS if t not in cols]


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def check_rows(name, pt, n_den_cols, sel=None):
    """What every result obeys by itself: the masks within the selection, 0.0 in the slots that are
    not set, and the score the row's own sequential sum."""
    pres = pt.present
    if pt.terms.shape != pres.shape or len(pt.score) != len(pres):
        return fail(name, "shapes", pt.terms.shape, pres.shape)
    off = pt.terms[~pres]
    if len(off) and (u64(off) != 0).any():
        return fail(name, "a slot that is not set does not hold +0.0")
    for i in range(len(pt)):
        want = ptr.score_from_row(pt.terms[i], pres[i], n_den_cols)
        if bits(want)[0] != bits(pt.score[i:i + 1])[0]:
            return fail(name, "score is not the row's sum", i, float(pt.score[i]), float(want))
    if sel is not None:
        T = pt.terms.shape[1] - 7
        if (pt.fixed & ~np.uint32(sel.fixed)).any() or (pt.cols & ~np.uint64(sel.cols & ((1 << T) - 1))).any():
            return fail(name, "a deselected slot is present")
    return 0


def check_terms(name, eng, c, single, a, b):
    """The full check of an unselected call against the references."""
    pt = eng.fas_pairs_terms(a, b)
    W = 7 + c.n_cols
    if pt.terms.shape != (len(a), W):
        return fail(name, "row width", pt.terms.shape)
    ref1 = single.scores(a, b)
    pres = pt.present
    if not np.array_equal(pres, ref1 > 0):
        bad = np.argwhere(pres != (ref1 > 0))[0]
        return fail(name, "present mask vs single-field oracle", int(a[bad[0]]), int(b[bad[0]]), "slot", int(bad[1]))
    if not np.array_equal(pres, ptr.presence(c, a, b)):
        return fail(name, "present mask vs the corpus arrays")
    got1 = ptr.single_score_of_terms(pt.terms)
    neq = pres & (bits(got1).reshape(pres.shape) != bits(ref1).reshape(pres.shape))
    if neq.any():
        bad = np.argwhere(neq)[0]
        return fail(name, "term vs single-field oracle", int(a[bad[0]]), int(b[bad[0]]), "slot", int(bad[1]),
                    float(pt.terms[bad[0], bad[1]]), float(got1[bad[0], bad[1]]), float(ref1[bad[0], bad[1]]))
    plain, base = eng.fas_pairs(a, b), tl.Oracle(c).fas_pairs(a, b)
    if not (np.array_equal(bits(pt.score), bits(plain)) and np.array_equal(bits(pt.score), bits(base))):
        return fail(name, "head score vs fas_pairs / the base oracle")
    print(name, len(a), "pairs, used", int(pt.used.min()), "..", int(pt.used.max()))
    return check_rows(name, pt, c.n_cols)


def check_pairs():
    e = tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        a, b = ptr.uid_arrays(ptr.e_pairs())
        if check_terms("E", eng, e, ptr.SingleRef(e), a, b):
            return 1
        pt = eng.fas_pairs_terms(a, b)
        empty = a == ec.uid_of(ec.EMPTY_USER)
        if not empty.any() or pt.fixed[empty].any() or pt.cols[empty].any() or (bits(pt.score[empty]) != 0).any():
            return fail("the empty user's pairs: used == 0 scores +0.0 with both masks 0")
        if pf.PairTerms.slot_names(ec.COLS)[:8] != list(pf.FIXED_FIELD_NAMES) + ["c00"] or len(pf.PairTerms.slot_names(ec.COLS)) != 55:
            return fail("slot_names")
        return 0
    finally:
        eng.close()


def same_rows(x, i, y, j):
    return (bits(x.score[i:i + 1])[0] == bits(y.score[j:j + 1])[0] and x.fixed[i] == y.fixed[j] and x.cols[i] == y.cols[j] and
            np.array_equal(u64(x.terms[i]), u64(y.terms[j])))


def check_shapes():
    e = tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        single = ptr.SingleRef(e)
        q = ec.uid_of(ec.HIT_Q_SPREAD)
        cand = np.array([ec.uid_of(i) for i in range(513)], np.int32)
        if check_terms("one query x 513", eng, e, single, np.full(513, q, np.int32), cand):
            return 1
        full = eng.fas_pairs_terms(np.full(513, q, np.int32), cand)
        for n in (0, 1, 64, 65, 512):
            pt = eng.fas_pairs_terms(np.full(n, q, np.int32), cand[:n])
            if len(pt) != n or pt.terms.shape != (n, 55) or not all(same_rows(pt, i, full, i) for i in range(n)):
                return fail("n =", n, "vs the rows of n = 513")
        a = np.array([ec.uid_of(i) for i in range(300)], np.int32)
        b = np.array([ec.uid_of((7 * i + 3) % ec.N_USERS) for i in range(300)], np.int32)
        if check_terms("300 queries", eng, e, single, a, b):
            return 1
        known = eng.fas_pairs_terms(a[:4], b[:4])
        ua = np.array([a[0], 5, a[1], a[2], 6, a[3]], np.int32)
        ub = np.array([b[0], b[1], b[1], 7, 8, b[3]], np.int32)
        pt = eng.fas_pairs_terms(ua, ub)
        for i in (1, 3, 4):
            if not np.isnan(pt.score[i]) or pt.fixed[i] or pt.cols[i] or (u64(pt.terms[i]) != 0).any():
                return fail("unknown uid at", i)
        for i, j in ((0, 0), (2, 1), (5, 3)):
            if not same_rows(pt, i, known, j):
                return fail("known pair between unknown ones", i)
        if not np.isnan(eng.fas_pairs(ua, ub)[[1, 3, 4]]).all():
            return fail("fas_pairs on the same unknown uids")
    finally:
        eng.close()
    with tempfile.TemporaryDirectory() as d:
        ec.write_reference_files(d, n_first=2)
        c = tl.read_reference_dir(d)
    eng = tl.engine(c)
    try:
        a, b = ptr.uid_arrays([(0, 1), (1, 0), (0, 0), (1, 1)])
        return check_terms("2 users", eng, c, ptr.SingleRef(c), a, b)
    finally:
        eng.close()


SELECTS = [("age_off", S(fixed=pf.PF_SEL_FIXED_ALL & ~(1 << pf.PF_F_AGE))),
           ("only_col_l", S(fixed=0, cols=[ec.COL_L])),
           ("half_hs_off", S(cols=without(*ec.COLS_HS[::2]))),  # hits on deselected columns between hits on selected ones
           ("nothing", S(fixed=0, cols=0)),
           ("everything", S())]


def check_selected(name, eng, c, a, b, sel, ref):
    """pt under sel against the unselected call, fas_pairs(select=) and the derived oracle."""
    T = c.n_cols
    base, pt = eng.fas_pairs_terms(a, b), eng.fas_pairs_terms(a, b, select=sel)
    cm = np.uint64(sel.cols & ((1 << T) - 1))
    if not (np.array_equal(pt.fixed, base.fixed & np.uint32(sel.fixed)) and np.array_equal(pt.cols, base.cols & cm)):
        return fail(name, "masks != unselected masks AND the selection")
    pres = pt.present
    if (u64(pt.terms)[pres] != u64(base.terms)[pres]).any():
        return fail(name, "a selected slot's term differs from the unselected call's")
    want = ref.fas_pairs(a, b) if ref is not None else None
    got = eng.fas_pairs(a, b, select=sel)
    if not np.array_equal(bits(pt.score), bits(got)) or (want is not None and not np.array_equal(bits(pt.score), bits(want))):
        return fail(name, "score vs fas_pairs(select=) / the derived oracle")
    return check_rows(name, pt, bin(int(cm)).count("1"), sel)


def check_select():
    e = tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        a, b = ptr.uid_arrays(ptr.e_pairs())
        plain = eng.fas_pairs_terms(a, b)
        eng.set_scan_select(S(fixed=0, cols=[3]))  # a scan selection on the context plays no part
        under = eng.fas_pairs_terms(a, b)
        if not all(same_rows(plain, i, under, i) for i in range(len(a))):
            return fail("a scan selection on the context changed the breakdown")
        for sname, s in SELECTS:
            if check_selected(sname, eng, e, a, b, s, fsr.SelRef(e, s)):
                return 1
        if eng._select is None or eng._select.cols != 8:
            return fail("the context's scan selection changed")
        bad = S()
        bad.fixed = 0x80
        head, terms = np.zeros(len(a), "V16"), np.zeros((len(a), 55))
        if eng._L.pf_fas_pairs_terms(eng.h, a.ctypes.data, b.ctypes.data, len(a), bad, head.ctypes.data, terms.ctypes.data) != pf.PF_EINVAL:
            return fail("malformed selection")
        return 0
    finally:
        eng.close()


def check_gtab():
    c = fs_chk.gtab_corpus()
    G = fs_chk.GTAB_UID
    eng = tl.engine(c)
    try:
        cand = [ec.uid_of(i) for i in list(ec.HITS_ONE.values()) + list(ec.RUNS.values()) + list(range(64 - 9))]
        a = np.array([G] * len(cand) + cand + [G], np.int32)
        b = np.array(cand + [G] * len(cand) + [G], np.int32)
        if check_terms("gtab", eng, c, ptr.SingleRef(c), a, b):
            return 1
        s = S(fixed=0x7F & ~(1 << pf.PF_F_FRIENDS), cols=without(ec.COL_L))
        return check_selected("gtab col_l_off_friends_off", eng, c, a, b, s, fsr.SelRef(c, s))
    finally:
        eng.close()


def wide_corpus():
    """E with the ID_TOP club ids at 2^30 and the friend ids at 2^31 + 7: past the packed store's
    id limit, so the store takes the wide format."""
    c = tl.golden_corpus("E")
    clubs, friends = np.array(c.clubs, copy=True), np.array(c.friends, copy=True)
    assert (clubs == ec.ID_TOP).sum() >= 2 and (friends == ec.ID_TOP).sum() >= 2
    clubs[clubs == ec.ID_TOP] = 2**30
    friends[friends == ec.ID_TOP] = 2**31 + 7
    f = dict(uid=c.uid, pub=c.pub, comp=c.comp, gen=c.gen, age=c.age, region=c.region, club_off=c.club_off, clubs=clubs,
             friend_off=c.friend_off, friends=friends, tok_off=c.tok_off, tok_tid=c.tok_tid, tok_tf=c.tok_tf,
             adj_uid=c.adj_uid, adj_off=c.adj_off, adj_nbr=c.adj_nbr)
    f = {k: np.array(v, copy=True) for k, v in f.items()}
    return tl.Corpus(n_cols=c.n_cols, norm_present=c.norm_present.copy(), norm_mean=c.norm_mean.copy(),
                     norm_sd=c.norm_sd.copy(), median=c.median, col_names=c.col_names, **f)


def check_wide():
    c = wide_corpus()
    eng = tl.engine(c)
    try:
        if eng.layout().packed_tokens != 0:
            return fail("the store stayed packed")
        a, b = ptr.uid_arrays(ptr.e_pairs() + [(56, 59), (59, 56), (60, 59), (59, 60)])
        if check_terms("wide", eng, c, ptr.SingleRef(c), a, b):
            return 1
        s = dict(SELECTS)["half_hs_off"]
        return check_selected("wide half_hs_off", eng, c, a, b, s, fsr.SelRef(c, s))
    finally:
        eng.close()


def same_list(x, y):
    return list(x[0]) == list(y[0]) and np.array_equal(bits(x[1]), bits(y[1]))


def check_explain():
    e = tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        qs = [ec.uid_of(i) for i in ec.PLANTED_QUERIES[::4]] + [5]
        filt = pf.CandFilter.make(gender=1, age=(20, 29))
        sel = S(fixed=0x7F & ~(1 << pf.PF_F_GENDER), cols=without(*ec.COLS_HS[::2]))
        first = eng.recommend_interest_all(qs[:3], 10)

        def one(us, k, f, s):
            plain = eng.recommend_interest_all(us, k, filter=f, select=s)
            got = eng.recommend_interest_all(us, k, filter=f, select=s, explain=True)
            if eng._filter is not None or eng._select is not None:
                return fail("explain: the context's filter / selection was not restored")
            for u, p, g in zip(us, plain, got):
                tag = ("explain", u, k, f is not None, s is not None)
                if len(g) != 3 or not same_list(g, p):
                    return fail(*tag, "ids / scores vs explain=False")
                if u == 5:
                    if len(g[0]) or len(g[2]) or g[2].terms.shape != (0, 55):
                        return fail(*tag, "the unknown user's result is not empty")
                    continue
                if len(g[0]) == 0:
                    return fail(*tag, "empty list")
                pt = eng.fas_pairs_terms([u] * len(g[0]), g[0], select=s)
                if len(g[2]) != len(g[0]) or not all(same_rows(g[2], i, pt, i) for i in range(len(pt))):
                    return fail(*tag, "rows / heads vs fas_pairs_terms")
                if not np.array_equal(bits(g[2].score), bits(g[1])):
                    return fail(*tag, "head scores vs the list's")
            return 0

        for f in (None, filt):
            for s in (None, sel):
                for k in (10, 100):
                    for u in qs:
                        if one([u], k, f, s):
                            return 1
                if one((qs[:7] + [5])[:8], 10, f, s):  # a batch of 8 queries in one call
                    return 1
        # a filter and a selection set on the context are the call's, and stay
        eng.set_scan_filter(filt)
        eng.set_scan_select(sel)
        got = eng.recommend_interest_all(qs[:3], 10, explain=True)
        want = eng.recommend_interest_all(qs[:3], 10)
        if not all(same_list(g, w) for g, w in zip(got, want)) or eng._filter is None or eng._select is None:
            return fail("explain under the context's own filter and selection")
        for u, g in zip(qs[:3], got):
            pt = eng.fas_pairs_terms([u] * len(g[0]), g[0], select=sel)
            if not all(same_rows(g[2], i, pt, i) for i in range(len(pt))):
                return fail("explain rows under the context's selection", u)
        eng.clear_scan_filter()
        eng.clear_scan_select()
        if not all(same_list(g, w) for g, w in zip(eng.recommend_interest_all(qs[:3], 10), first)):
            return fail("the plain scan after the explain calls")
        return 0
    finally:
        eng.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "pairs"
    rc = {"pairs": check_pairs, "shapes": check_shapes, "select": check_select, "gtab": check_gtab, "wide": check_wide,
          "explain": check_explain}[mode]()
    if rc:
        return 1
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
