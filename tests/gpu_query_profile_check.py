"""Child process of test_gpu_query_profile (the engine reads PF_DEBUG once per process).  argv[1]
picks the check:
  clone_profiles / clone_explicit   a QueryProfile copied from a stored user X, excluding adj[X] + {X},
                                    gives the by-uid scan's ids and score bits (idf from the profiles /
                                    the golden explicit map), under both scan kernels, a filter, a
                                    selection and explain=True
  absent                            Y and Z, whom E does not hold, against the oracle opened on
                                    C+ = E + {Y, Z}; the breakdown; one batch = its single calls; shards
  state                             nothing sticks to the context; the error codes
  heavy                             one call of ordinary profiles and one too large for the postings scan
                                    (a clone of the hub corpus's uid 4242) equals the by-uid call
Cases and corpora: tests/query_profile_cases.py.  Exits non-zero on any mismatch."""
import ctypes
import sys

import numpy as np

import edge_corpus as ec
import pair_terms_ref as ptr
import pokec_testlib as tl
import query_profile_cases as qc

pf = tl.product()
S = pf.FieldSelect.make
bits = ptr.bits
KERNELS = [("postings", pf.PF_SCAN_POSTINGS), ("stream", pf.PF_SCAN_STREAM)]


def fail(*a):
    print("mismatch", *a, file=sys.stderr)
    return 1


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_list(x, y):
    return list(x[0]) == list(y[0]) and np.array_equal(bits(x[1]), bits(y[1]))


def same_terms(x, y):
    return (np.array_equal(bits(x.score), bits(y.score)) and np.array_equal(x.fixed, y.fixed) and
            np.array_equal(x.cols, y.cols) and np.array_equal(u64(x.terms), u64(y.terms)))


def check_clone(explicit):
    e = qc.e_explicit() if explicit else tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        uids = qc.clone_query_uids()
        profs = {u: qc.clone_profile(pf, e, u) for u in uids}
        filt = pf.CandFilter.make(gender=1, age=(20, 29))
        sel = S(fixed=0x7F & ~((1 << pf.PF_F_AGE) | (1 << pf.PF_F_CLUBS)), cols=[t for t in range(ec.N_COLS) if t != ec.COL_L])
        n = 0
        for kname, kind in KERNELS:
            eng.set_scan_kernel(kind)
            for u in uids:
                for k in (1, 10, 64):
                    want = eng.recommend_interest_all([u], k)[0]
                    got = eng.recommend_profile(profs[u], k)[0]
                    if not same_list(got, want):
                        return fail("clone", kname, u, k, list(got[0][:5]), list(want[0][:5]))
                    n += 1
                for f, s in ((filt, None), (None, sel), (filt, sel)):
                    want = eng.recommend_interest_all([u], 10, filter=f, select=s)[0]
                    got = eng.recommend_profile(profs[u], 10, filter=f, select=s)[0]
                    if not same_list(got, want):
                        return fail("clone", kname, u, "filter" if f else "", "select" if s else "")
                for s in (None, sel):
                    want = eng.recommend_interest_all([u], 10, select=s, explain=True)[0]
                    got = eng.recommend_profile(profs[u], 10, select=s, explain=True)[0]
                    if len(got) != 3 or not same_list(got, want) or not same_terms(got[2], want[2]):
                        return fail("clone explain", kname, u, s is not None)
                if eng._filter is not None or eng._select is not None:
                    return fail("the context's filter / selection was not restored")
        # the pair calls of a clone: bit-equal to the stored user's
        b = e.uid[::7].astype(np.int32)
        for u in uids[::6]:
            a = np.full(len(b), u, np.int32)
            for s in (None, sel):
                if not np.array_equal(bits(eng.fas_profile_pairs(profs[u], b, select=s)), bits(eng.fas_pairs(a, b, select=s))):
                    return fail("clone pairs", u, s is not None)
                if not same_terms(eng.fas_profile_pairs_terms(profs[u], b, select=s), eng.fas_pairs_terms(a, b, select=s)):
                    return fail("clone pair terms", u, s is not None)
        print("clones:", len(uids), "users,", n, "plain scans per kernel pair")
        return 0
    finally:
        eng.close()


def oracle_list(orc, uid, k, drop):
    ids, sc = orc.interest([uid], k + len(drop), pf.PF_MODE_ALL, 0)[0]
    keep = ~np.isin(ids, list(drop))
    return ids[keep][:k], sc[keep][:k]


def merged(parts, k):
    ids = np.concatenate([p[0] for p in parts])
    sc = np.concatenate([p[1] for p in parts])
    order = sorted(range(len(ids)), key=lambda i: (-float(sc[i]), int(ids[i])))[:k]
    return ids[order], sc[order]


def check_absent():
    e = qc.e_explicit()
    eng = tl.engine(e)
    try:
        all_uids = e.uid.astype(np.int32)
        for variant in qc.Y_AGES:
            orc = tl.Oracle(qc.c_plus(variant))
            Y = qc.profile_of_record(pf, qc.y_record(variant), exclude=qc.ADJ_Y)
            Z = qc.profile_of_record(pf, qc.z_record())
            for kname, kind in KERNELS:
                eng.set_scan_kernel(kind)
                for k in (1, 10, 64):
                    got = eng.recommend_profile(Y, k)[0]
                    want = oracle_list(orc, qc.UID_Y, k, (qc.UID_Y, qc.UID_Z))
                    if not same_list(got, want):
                        return fail("Y vs oracle", variant, kname, k, list(got[0][:5]), list(want[0][:5]),
                                    got[1][:3], want[1][:3])
                    got = eng.recommend_profile(Z, k)[0]
                    want = oracle_list(orc, qc.UID_Z, k, (qc.UID_Y, qc.UID_Z))
                    if not same_list(got, want) or (bits(got[1]) != 0).any() or list(got[0]) != sorted(all_uids)[:k]:
                        return fail("Z vs oracle", variant, kname, k)
            for name, P, u in (("Y", Y, qc.UID_Y), ("Z", Z, qc.UID_Z)):
                got = eng.fas_profile_pairs(P, all_uids)
                want = orc.fas_pairs(np.full(len(all_uids), u, np.int32), all_uids)
                if not np.array_equal(bits(got), bits(want)):
                    bad = int(np.nonzero(bits(got) != bits(want))[0][0])
                    return fail(name, "pairs vs oracle", variant, int(all_uids[bad]), float(got[bad]), float(want[bad]))
            orc.close()
            # terms: the head is fas_profile_pairs, the score the row's own sum, a deselected slot absent
            plain = eng.fas_profile_pairs(Y, all_uids)
            pt = eng.fas_profile_pairs_terms(Y, all_uids)
            if not np.array_equal(bits(pt.score), bits(plain)):
                return fail("terms head vs fas_profile_pairs", variant)
            pres = pt.present
            for i in range(0, len(pt), 3):
                if bits(ptr.score_from_row(pt.terms[i], pres[i], ec.N_COLS))[0] != bits(pt.score[i:i + 1])[0]:
                    return fail("score is not the row's sum", variant, int(all_uids[i]))
            if not pres[:, pf.PF_F_GENDER].any() or not pres[:, 7 + qc.COL_NOVEL].any():
                return fail("Y's unknown gender / novel column never present: the s = 0 term is missing")
            sel = S(fixed=0x7F & ~(1 << pf.PF_F_GENDER), cols=[t for t in range(ec.N_COLS) if t != qc.COL_MIXED])
            ps = eng.fas_profile_pairs_terms(Y, all_uids, select=sel)
            if not np.array_equal(bits(ps.score), bits(eng.fas_profile_pairs(Y, all_uids, select=sel))):
                return fail("selected terms head vs fas_profile_pairs(select=)")
            sp = ps.present
            if sp[:, pf.PF_F_GENDER].any() or sp[:, 7 + qc.COL_MIXED].any():
                return fail("a deselected slot is present")
            if (u64(ps.terms[:, pf.PF_F_GENDER]) != 0).any() or (u64(ps.terms[:, 7 + qc.COL_MIXED]) != 0).any():
                return fail("a deselected slot does not hold 0.0")
            if (u64(ps.terms)[sp] != u64(pt.terms)[sp]).any():
                return fail("a selected slot's term differs from the unselected call's")
            for i in range(0, len(ps), 3):
                if bits(ptr.score_from_row(ps.terms[i], sp[i], ec.N_COLS - 1))[0] != bits(ps.score[i:i + 1])[0]:
                    return fail("selected score is not the row's sum", int(all_uids[i]))
        # batch = singles, under both kernels
        Y = qc.profile_of_record(pf, qc.y_record(), exclude=qc.ADJ_Y)
        Z = qc.profile_of_record(pf, qc.z_record())
        X1 = qc.clone_profile(pf, e, ec.uid_of(ec.Q_LONG[200]))
        X2 = qc.clone_profile(pf, e, ec.uid_of(ec.CLONE_QUERIES[2]))
        batch = [Y, X1, Z, X2]
        for kname, kind in KERNELS:
            eng.set_scan_kernel(kind)
            for k in (10, 64):
                got = eng.recommend_profile(batch, k)
                one = [eng.recommend_profile(p, k)[0] for p in batch]
                if len(got) != 4 or not all(same_list(g, w) for g, w in zip(got, one)):
                    return fail("batch vs singles", kname, k)
                gt = eng.recommend_profile(batch, k, explain=True)
                ot = [eng.recommend_profile(p, k, explain=True)[0] for p in batch]
                if not all(same_list(g, w) and same_terms(g[2], w[2]) for g, w in zip(gt, ot)):
                    return fail("batch vs singles, explain", kname, k)
            # shards: the two halves merged on the host are the unsharded result
            for p, name in ((Y, "Y"), (X2, "clone"), (Z, "Z")):
                for k in (10, 64):
                    whole = eng.recommend_profile(p, k)[0]
                    parts = []
                    for sh in (0, 1):
                        eng.set_shard(sh, 2)
                        parts.append(eng.recommend_profile(p, k)[0])
                    eng.set_shard(0, 1)
                    if not same_list(merged(parts, k), whole):
                        return fail("shards", kname, name, k)
        return 0
    finally:
        eng.close()


def raw_profile(**kw):
    """A pf_query_profile with its arrays given as they are (no QueryProfile.make checks)."""
    p = pf.QueryProfile()
    p.public_flag = p.gender = -1
    p.region[0] = p.region[1] = p.region[2] = -1
    keep = []
    for name, cnt, dt in (("club_ids", "n_clubs", np.uint32), ("friend_ids", "n_friends", np.uint32),
                          ("exclude_uid", "n_exclude", np.int32)):
        a = np.asarray(kw.get(name, []), dt)
        keep.append(a)
        setattr(p, name, a.ctypes.data if len(a) else None)
        setattr(p, cnt, len(a))
    off = np.asarray(kw.get("tok_off", [0] * (ec.N_COLS + 1)), np.int64)
    tid, tf = np.asarray(kw.get("tok_tid", [0]), np.int32), np.asarray(kw.get("tok_tf", [0]), np.int32)
    keep += [off, tid, tf]
    p.tok_off, p.tok_tid, p.tok_tf = off.ctypes.data, tid.ctypes.data, tf.ctypes.data
    p.flags = kw.get("flags", 0)
    p._keep = keep
    return p


def check_state():
    e = tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        L = eng._L
        gq = [ec.uid_of(i) for i in (ec.Q_LONG[200], ec.CLONE_QUERIES[0], ec.EXCL_RUN_Q)]
        before = eng.recommend_interest_all(gq, 10)
        pairs_before = eng.fas_pairs(np.full(64, gq[0], np.int32), e.uid[:64])
        bytes_before = eng.scan_bytes(gq)
        gold = {k[1]: v for k, v in tl.golden_lists("E", "all.txt").items()}  # the reference's own top-50
        for u, (ids, sc) in zip(gq, before):
            if [(int(i), int(b)) for i, b in zip(ids, bits(sc))] != gold[u][:10]:
                return fail("the by-uid query is not the golden list", u)
        Y = qc.profile_of_record(pf, qc.y_record(), exclude=qc.ADJ_Y)
        Z = qc.profile_of_record(pf, qc.z_record())
        X = qc.clone_profile(pf, e, gq[0])
        for _ in range(3):
            eng.recommend_profile([Y, X, Z], 10)
            eng.recommend_profile(X, 64, explain=True)
            eng.recommend_profile(Y, 10, filter=pf.CandFilter.make(gender=1), select=S(fixed=0x3F))
            eng.fas_profile_pairs(Y, e.uid[:100])
            eng.fas_profile_pairs_terms(X, e.uid[:100])
        after = eng.recommend_interest_all(gq, 10)
        if not all(same_list(a, b) for a, b in zip(before, after)):
            return fail("a by-uid query changed after the ad-hoc calls")
        if not np.array_equal(bits(pairs_before), bits(eng.fas_pairs(np.full(64, gq[0], np.int32), e.uid[:64]))):
            return fail("by-uid pairs changed after the ad-hoc calls")
        if list(bytes_before) != list(eng.scan_bytes(gq)):
            return fail("scan_bytes changed after the ad-hoc calls")
        for u, one in zip(gq, before):  # one query from its resident image, as before
            if not same_list(eng.recommend_interest_all([u], 10)[0], one):
                return fail("the resident one-query launch changed", u)

        # ---- errors
        k = 10
        ou, os_, oc = np.full(2 * 65, -7, np.int32), np.full(2 * 65, -7, np.float32), np.full(2, -7, np.int32)

        def call(p, n=1, topk=k):
            arr = (pf.QueryProfile * 1)()
            if p is not None:
                ctypes.memmove(ctypes.byref(arr[0]), ctypes.byref(p), ctypes.sizeof(pf.QueryProfile))
            return L.pf_recommend_interest_profile(eng.h, ctypes.byref(arr) if p is not None else None, n, topk,
                                                   ou.ctypes.data, os_.ctypes.data, oc.ctypes.data)

        T = ec.N_COLS
        off1 = [0] * 3 + [2] * (T - 2)  # column 2 holds two tokens
        cases = [("negative tid", raw_profile(tok_off=off1, tok_tid=[4, -1], tok_tf=[1, 1]), pf.PF_EINVAL),
                 ("repeated tid", raw_profile(tok_off=off1, tok_tid=[4, 4], tok_tf=[1, 1]), pf.PF_EINVAL),
                 ("non-monotone tok_off", raw_profile(tok_off=[0, 2, 1] + [2] * (T - 2), tok_tid=[4, 5], tok_tf=[1, 1]), pf.PF_EINVAL),
                 ("flags", raw_profile(flags=1), pf.PF_EINVAL),
                 ("club x 256", raw_profile(club_ids=[9] * 256), pf.PF_EUNSUPP),
                 ("tf 256", raw_profile(tok_off=off1, tok_tid=[4, 5], tok_tf=[1, 256]), pf.PF_EUNSUPP)]
        for name, p, want in cases:
            rc = call(p)
            if rc != want or not L.pf_last_error(eng.h):
                return fail("error case", name, rc, want)
            if (ou != -7).any() or (os_ != -7).any():
                return fail("error case wrote results", name)
        if call(None, n=1) != pf.PF_EINVAL:
            return fail("NULL profile with nq > 0")
        if call(raw_profile(), topk=65) != pf.PF_EUNSUPP:
            return fail("topk = 65")
        oc[:] = -7
        if call(raw_profile(), n=0) != pf.PF_OK or call(None, n=0) != pf.PF_OK or (oc != -7).any() or (ou != -7).any():
            return fail("nq = 0 is PF_OK with no writes")
        if call(raw_profile(club_ids=[9] * 255)) != pf.PF_OK:
            return fail("a club repeated 255 times is within the limit")
        for code, p in ((pf.PF_EINVAL, raw_profile(flags=1)), (pf.PF_EUNSUPP, raw_profile(club_ids=[9] * 256))):
            for fn in (lambda: eng.fas_profile_pairs(p, e.uid[:4]), lambda: eng.fas_profile_pairs_terms(p, e.uid[:4]),
                       lambda: eng.recommend_profile(p, 10, explain=True)):
                try:
                    fn()
                    return fail("no exception for a refused profile")
                except pf.FasError as ex:
                    if ex.code != code:
                        return fail("exception code", ex.code, code)
        # unknown uids in exclude are ignored; a known one is never returned
        base = eng.recommend_profile(qc.profile_of_record(pf, qc.y_record()), 10)[0]
        unk = eng.recommend_profile(qc.profile_of_record(pf, qc.y_record(), exclude=[5, 123456789, -3]), 10)[0]
        if not same_list(base, unk):
            return fail("unknown uids in exclude changed the result")
        drop = [int(base[0][0]), int(base[0][3])]
        ex = eng.recommend_profile(qc.profile_of_record(pf, qc.y_record(), exclude=drop + [5]), 10)[0]
        if set(drop) & set(int(x) for x in ex[0]) or list(ex[0][:8]) != [int(x) for x in base[0] if int(x) not in drop]:
            return fail("an excluded uid was returned, or the rest moved")
        # an unknown b_uid scores NaN
        sc = eng.fas_profile_pairs(Y, [int(e.uid[0]), 5, int(e.uid[1])])
        if not np.isnan(sc[1]) or np.isnan(sc[0]) or np.isnan(sc[2]):
            return fail("unknown b_uid")
        if not all(same_list(a, b) for a, b in zip(before, eng.recommend_interest_all(gq, 10))):
            return fail("a by-uid query changed after the refused calls")
        return 0
    finally:
        eng.close()


def check_heavy():
    """The hub corpus of test_gpu_parity.py: 20,000 users, uid 4242 naming 22,000 friend ids (about 20k
    set lists, beyond one workgroup's 160 KB).  One recommend_profile call of clones of
    [4242, 3, 15000, 4242, 777] under the auto kernel sends the heavy ones to K1 and the others to K5;
    ids and float32 bits are the by-uid call's (pinned to the oracle by test_heavy_query_routes_to_stream_scan)."""
    base = tl.synth.Corpus(n_users=20000, seed=77, edge_cases=1)
    c = tl.with_rows(tl.corpus_from_desc(base.desc_ptr()), user=4242, friends=np.arange(1, 22001, dtype=np.uint32))
    eng = tl.engine(c)
    try:
        q = [4242, 3, 15000, 4242, 777]
        if eng.layout().scan_kernel != pf.PF_SCAN_POSTINGS:
            return fail("the auto kernel is not the postings scan")
        want = eng.recommend_interest_all(q, 10)
        got = eng.recommend_profile([qc.clone_profile(pf, c, u) for u in q], 10)
        for u, g, w in zip(q, got, want):
            if len(w[0]) != 10 or not same_list(g, w):
                return fail("heavy batch", u, list(g[0]), list(w[0]))
        return 0
    finally:
        eng.close()


def main():
    mode = sys.argv[1]
    rc = {"clone_profiles": lambda: check_clone(False), "clone_explicit": lambda: check_clone(True),
          "absent": check_absent, "state": check_state, "heavy": check_heavy}[mode]()
    if rc:
        return 1
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
