"""Child process of test_gpu_field_select: the engine reads PF_DEBUG once per process, so each launch
shape runs in its own.  argv[1] picks the path: `one` (one query per call: K5's one-query
instantiation, or K1 under PF_DEBUG scan=stream), `batch` (8 queries in one call), `topk100` (the
job pipeline's all-candidates jobs), `async` (one-query scan_keys_async calls on a caller's stream,
a different selection before each and no synchronisation between them), `pairs`
(pf_fas_pairs_select) or `gtab` (E plus one user whose K1 / K1' table is probed in global memory).

The oracle knows no selection: the expected bits are the oracle's on the derived corpus of
tests/field_select_ref.py (only the selected columns, every deselected fixed field blanked), its
whole ranking of the query cut in numpy by the filter mask where one is set.  Ids and float32 bits
must be equal.  Exits non-zero on any mismatch."""
import json
import os
import sys
import tempfile

import numpy as np

import edge_corpus as ec
import field_select_ref as fsr
import gpu_scan_filter_check as fchk
import pokec_testlib as tl

pf = tl.product()
S = pf.FieldSelect.make
same, np_pass, merged = fchk.same, fchk.np_pass, fchk.merged
ALL_COLS = list(range(ec.N_COLS))


def without(*cols):
    return [t for t in ALL_COLS if t not in cols]


# the selections on E
E_SELECTS = [(n + "_off", S(fixed=pf.PF_SEL_FIXED_ALL & ~(1 << k))) for k, n in enumerate(pf.FIXED_FIELD_NAMES)] + [
    ("fixed_off", S(fixed=0)),                                        # text only, every column
    ("only_col_l", S(fixed=0, cols=[ec.COL_L])),                      # the 64..200-token column, where rounds split
    ("col_l_off", S(cols=without(ec.COL_L))),
    ("col_hc_off", S(cols=without(ec.COL_HC))),                       # hits on a deselected column in the K1 / K1' hit lists
    ("half_hs_off", S(cols=without(*ec.COLS_HS[::2]))),               # ... between hits on selected ones
    ("hs_and_hc_only", S(fixed=0, cols=ec.COLS_HS[1::2] + [ec.COL_HC])),
] + [("z_" + m, S(cols=[t])) for m, t in ec.SPLIT_Z_MODES.items()] + [  # the three normaliser modes
    ("prefix5", S(cols=range(5))),
    ("dense_cols_off", S(cols=without(*ec.D_TOKENS))),                # the clones keep one text column: a top-k of ties
    ("everything", S()),                                              # the bits of no selection
    ("everything_t", S(fixed=0x7F, cols=(1 << ec.N_COLS) - 1)),
    ("nothing", S(fixed=0, cols=0)),                                  # no field used: every score 0.0, order by uid
    ("friends_only", S(fixed=[pf.PF_F_FRIENDS], cols=0)),
]
SMALL = ("gender_off", "only_col_l", "half_hs_off", "prefix5", "nothing", "dense_cols_off")


def fail(*a):
    print("mismatch", *a, file=sys.stderr)
    return 1


def e_queries():
    idx = (sorted(ec.Q_LONG.values()) + [ec.Q_TWO_LONG, ec.HIT_Q_ONE, ec.HIT_Q_SPREAD, ec.EMPTY_USER, ec.TF0_USER,
                                           ec.SET_PARTNER, ec.EXCL_RUN_Q, ec.EXCL_CLONES_Q, 44, 47, 515, 1020] +
           ec.CLONE_QUERIES[::3] + list(range(0, ec.N_USERS, 331)))
    return [ec.uid_of(i) for i in sorted(set(idx))]


def run_one(name, c, q, ks, selects, mode, want_kernel, filt=None):
    eng = tl.engine(c)
    try:
        if want_kernel and eng.layout().scan_kernel != want_kernel:
            return fail(f"{name}: scan kernel {eng.layout().scan_kernel}, wanted {want_kernel}")
        mask = np_pass(c, filt) if filt is not None else None
        base = {u: eng.recommend_interest_all([u], ks[-1])[0] for u in q[::4]}  # before any selection
        for sname, s in selects:
            ref = fsr.SelRef(c, s)
            for k in ks:
                if mode == "batch":  # 8 queries in one call: the batch instantiation
                    for b in range(0, len(q), 8):
                        qs = (q[b:b + 8] + q[:8])[:8]
                        got = eng.recommend_interest_all(qs, k, filter=filt, select=s)
                        for u, g in zip(qs, got):
                            if not same(g, ref.expect(u, k, mask)):
                                return fail(name, sname, "batch", u, k)
                else:
                    for u in q:
                        g = eng.recommend_interest_all([u], k, filter=filt, select=s)[0]
                        w = ref.expect(u, k, mask)
                        if not same(g, w):
                            return fail(name, sname, mode, u, k, list(zip(g[0], g[1]))[:4], list(zip(w[0], w[1]))[:4])
            if eng._select is not None or eng._filter is not None:
                return fail(name, "the previous (no) selection was not restored")
            if sname == "nothing":  # no field used by anybody: 0.0 everywhere, ascending uid
                g = eng.recommend_interest_all([q[0]], ks[-1], select=s)[0]
                if len(g[0]) == 0 and c.n_users > 2:
                    return fail(name, "nothing: empty list")
                if any(float(x) != 0.0 for x in g[1]) or list(g[0]) != sorted(g[0]):
                    return fail(name, "nothing: scores / order", list(g[0])[:5], list(g[1])[:5])
            if sname.startswith("everything"):  # the same bits as cleared, and as before any selection
                for u, b in base.items():
                    eng.set_scan_select(s)
                    if eng._select is None:
                        return fail(name, "binding state")
                    g = eng.recommend_interest_all([u], ks[-1])[0]
                    eng.clear_scan_select()
                    if not same(g, b) or not same(eng.recommend_interest_all([u], ks[-1])[0], b):
                        return fail(name, sname, "vs no selection", u)
        return 0
    finally:
        eng.close()


def check_rest(e):
    """The recommenders and calls that never see the selection, the malformed selections on a live
    context, both shards merged, and a selection with a filter / against the query's exclusion row."""
    eng, orc = tl.engine(e), tl.Oracle(e)
    try:
        q5 = [ec.uid_of(i) for i in (1, 62, 466, 515, 1020)]
        pairs = ec.planted_pairs()[:200]
        a = np.array([ec.uid_of(x) for x, _ in pairs], np.int32)
        b = np.array([ec.uid_of(y) for _, y in pairs], np.int32)
        rest = lambda: (eng.recommend_graph_registration(q5, 10), eng.recommend_collaborative(q5, 10),
                        eng.recommend_clubs_collab(q5, 10))
        before, pb = rest(), eng.fas_pairs(a, b)
        sel = S(fixed=["gender"], cols=[ec.COL_L, 7])
        eng.set_scan_select(sel)
        under, pu = rest(), eng.fas_pairs(a, b)
        for what, x, y in zip(("fof interest", "collab", "clubs"), before, under):
            if not all(same(g, r) for g, r in zip(x, y)):
                return fail(what, "changed under a selection")
        if not np.array_equal(pb.view(np.uint32), pu.view(np.uint32)):
            return fail("plain fas_pairs changed under a selection")
        if list(eng.fof_candidates(q5[0], 50)) != list(orc.fof(q5[0], 50, tl.PF_FOF_GRAPH)):
            return fail("fof_candidates under a selection")
        # malformed: refused, and the selection in force stays
        ref = fsr.SelRef(e, sel)
        for fixed, flags in ((0x80, 0), (0x1FF, 0), (0x7F, 1), (1, 0x80000000)):
            bad = S()
            bad.fixed, bad.flags = fixed, flags
            rc = eng._L.pf_set_scan_select(eng.h, bad)
            if rc != pf.PF_EINVAL or not same(eng.recommend_interest_all([q5[3]], 10)[0], ref.expect(q5[3], 10)):
                return fail("malformed selection", fixed, flags, rc)
            out = np.zeros(len(a), np.float32)
            if eng._L.pf_fas_pairs_select(eng.h, a.ctypes.data, b.ctypes.data, len(a), bad, out.ctypes.data) != pf.PF_EINVAL:
                return fail("malformed pairs selection", fixed, flags)
        # both shards, merged
        for u in q5:
            parts = []
            for r_ in range(2):
                eng.set_shard(r_, 2)
                parts.append(eng.recommend_interest_all([u], 10)[0])
            eng.set_shard(0, 1)
            if not same(merged(parts, 10), ref.expect(u, 10)):
                return fail("shards", u)
        eng.clear_scan_select()
        for u in q5:
            if not same(eng.recommend_interest_all([u], 10)[0], orc.interest([u], 10, tl.PF_MODE_ALL, 0)[0]):
                return fail("unselected list after clearing", u)
        # a selection with a filter, and against EXCL_CLONES_Q's exclusion row (525 of the clones)
        F = pf.CandFilter.make
        for filt in (F(gender=1, age=(20, 29), keep_missing=True), F(region=(3, 9, 27))):
            m = np_pass(e, filt)
            for sname in ("age_off", "only_col_l", "dense_cols_off"):
                s = dict(E_SELECTS)[sname]
                r2 = fsr.SelRef(e, s)
                for u in q5:
                    for k in (10, 64, 100):
                        if not same(eng.recommend_interest_all([u], k, filter=filt, select=s)[0], r2.expect(u, k, m)):
                            return fail("filter + selection", sname, u, k)
        u = ec.uid_of(ec.EXCL_CLONES_Q)
        row = {int(x) for i, au in enumerate(e.adj_uid) if int(au) == u for x in e.adj_nbr[e.adj_off[i]:e.adj_off[i + 1]]} | {u}
        g = eng.recommend_interest_all([u], 64, select=dict(E_SELECTS)["dense_cols_off"])[0]
        if len(g[0]) != 64 or any(int(x) in row for x in g[0]):
            return fail("EXCL_CLONES_Q's row under a selection")
        return 0
    finally:
        eng.close()


def check_e(mode, want_kernel):
    e = tl.golden_corpus("E")
    q = e_queries()
    if mode == "topk100":
        return run_one("E", e, q[::3] + [ec.uid_of(ec.EXCL_CLONES_Q)], (100,), E_SELECTS, mode, 0)
    if run_one("E", e, q, (10, 64), E_SELECTS, mode, want_kernel):
        return 1
    if mode == "one" and check_rest(e):
        return 1
    small = [x for x in E_SELECTS if x[0] in SMALL]
    for n in (2, 511, 512, 513, 1025):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        qs = [ec.uid_of(i) for i in sorted({0, 1, min(5, n - 1), min(ec.HIT_Q_SPREAD, n - 1), n // 2, n - 1})]
        if run_one(f"n{n}", c, qs, (10, 64), small, mode, want_kernel):
            return 1
    return 0


def check_stats():
    """The pruning counters under selections: every candidate of every one-query scan is seen."""
    e = tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        eng.k5_prune_stats(reset=True)
        scans = 0
        for sname in ("only_col_l", "fixed_off", "half_hs_off", "nothing"):
            for u in e_queries()[::3]:
                eng.recommend_interest_all([u], 10, select=dict(E_SELECTS)[sname])
                scans += 1
        print("stats " + json.dumps({**eng.k5_prune_stats(), "scans": scans, "n_users": e.n_users}))
        return 0
    finally:
        eng.close()


def check_async():
    """Six one-query scan_keys_async calls on a caller's stream, a different selection set before each
    and no synchronisation between them: every row obeys its own, so the selection travels by value."""
    import torch
    e = tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        q = e_queries()
        names = ("gender_off", "only_col_l", "everything", "half_hs_off", "nothing", "fixed_off")
        ss = [(nm, dict(E_SELECTS)[nm]) for nm in names]
        refs = [fsr.SelRef(e, s) for _, s in ss]
        st = torch.cuda.Stream()
        for k in (10, 64):
            for b in range(0, len(q) - 5, 6):
                us = q[b:b + 6]
                rows = torch.full((6, k), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                for i, (u, (_, s)) in enumerate(zip(us, ss)):
                    eng.set_scan_select(s)
                    eng.scan_keys_async([u], k, rows[i].data_ptr(), st.cuda_stream)
                eng.clear_scan_select()
                st.synchronize()
                keys = rows.cpu().numpy().view(np.uint64)
                for i, (u, (sname, _)) in enumerate(zip(us, ss)):
                    if not same(pf.decode_keys(keys[i]), refs[i].expect(u, k)):
                        return fail("async", sname, u, k)
        return 0
    finally:
        eng.close()


def pair_arrays(pairs):
    return (np.array([ec.uid_of(x) for x, _ in pairs], np.int32), np.array([ec.uid_of(y) for _, y in pairs], np.int32))


def check_pairs():
    e = tl.golden_corpus("E")
    eng = tl.engine(e)
    try:
        a, b = pair_arrays(ec.planted_pairs() + [(x, y) for x, y, _ in ec.HIT_PAIRS] + [(y, x) for x, y, _ in ec.HIT_PAIRS])
        plain = eng.fas_pairs(a, b)
        eng.set_scan_select(S(fixed=0, cols=[3]))  # the scan selection plays no part in either pair call
        for sname, s in E_SELECTS:
            got = eng.fas_pairs(a, b, select=s)
            want = fsr.SelRef(e, s).fas_pairs(a, b)
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
                return fail("pairs", sname, len(bad), int(a[bad[0]]), int(b[bad[0]]), got[bad[0]], want[bad[0]])
            if sname.startswith("everything") and not np.array_equal(got.view(np.uint32), plain.view(np.uint32)):
                return fail("pairs", sname, "vs plain fas_pairs")
        if not np.array_equal(eng.fas_pairs(a, b).view(np.uint32), plain.view(np.uint32)):
            return fail("plain fas_pairs under a scan selection")
        unknown = eng.fas_pairs(np.array([a[0], 5], np.int32), np.array([7, b[0]], np.int32), select=S(fixed=0))
        if not np.isnan(unknown).all():
            return fail("unknown uids under a selection")
        return 0
    finally:
        eng.close()


GTAB_UID = 1_500_000_000


def gtab_corpus():
    """E plus one user with 9,000 distinct friend ids and tokens in two columns: its K1 / K1' table
    is past the LDS staging limit, so its image is probed in global memory (the GTAB instantiations)."""
    with tempfile.TemporaryDirectory() as d:
        ec.write_reference_files(d)
        p = ec._base(7)
        p["friends"] = [ec.uid_of(j % ec.N_USERS) if j < 200 else 3_000_000 + j for j in range(9000)]
        p["clubs"] = [11, 12, 5]
        p["toks"][ec.COL_HC] = {tok: 1 + k % 4 for k, tok in enumerate(ec.HC_TOKENS)}
        p["toks"][ec.COL_L] = {tok: 1 + k % 3 for k, tok in enumerate(ec.L_TOKENS[:40])}
        with open(os.path.join(d, "data", "users_encoded.csv"), "a") as f:
            f.write(ec._line(GTAB_UID, p) + "\n")
        return tl.read_reference_dir(d)


def check_gtab(want_kernel):
    c = gtab_corpus()
    assert c.n_users == ec.N_USERS + 1
    sels = [("col_hc_off", S(cols=without(ec.COL_HC))), ("col_l_off_friends_off", S(fixed=0x7F & ~(1 << pf.PF_F_FRIENDS), cols=without(ec.COL_L))),
            ("only_col_hc", S(fixed=0, cols=[ec.COL_HC])), ("everything", S())]
    q = [GTAB_UID, ec.uid_of(ec.HIT_Q_ONE), ec.uid_of(ec.Q_LONG[64])]
    if run_one("gtab", c, q, (10, 64, 100), sels, "one", 0):
        return 1
    eng = tl.engine(c)
    try:
        cand = [ec.uid_of(i) for i in list(ec.HITS_ONE.values()) + list(ec.RUNS.values()) + list(range(64 - 9))]
        a = np.array([GTAB_UID] * len(cand) + cand, np.int32)
        b = np.array(cand + [GTAB_UID] * len(cand), np.int32)
        for sname, s in sels:
            got, want = eng.fas_pairs(a, b, select=s), fsr.SelRef(c, s).fas_pairs(a, b)
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                return fail("gtab pairs", sname)
        return 0
    finally:
        eng.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "one"
    stream = "scan=stream" in os.environ.get("PF_DEBUG", "")
    if mode == "async":
        rc = check_async()
    elif mode == "pairs":
        rc = check_pairs()
    elif mode == "gtab":
        rc = check_gtab(1 if stream else 0)
    elif mode == "stats":
        rc = check_stats()
    else:
        rc = check_e(mode, 1 if stream else (0 if mode == "topk100" else 2))
    if rc:
        return 1
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
