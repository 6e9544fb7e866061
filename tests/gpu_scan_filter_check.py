"""Child process of test_gpu_scan_filter: the engine reads PF_DEBUG once per process, so each launch
shape runs in its own.  argv[1] picks the path: `one` (one query per call: K5's one-query
instantiation, or K1 under PF_DEBUG scan=stream), `batch` (8 queries in one call), `topk100` (the
job pipeline's all-candidates jobs) or `async` (one-query scan_keys_async calls on a caller's
stream, a different filter before each and no synchronisation between them).

The oracle has no filter.  The expected list of (query, filter, k) is the oracle's whole ranking of
the query (Oracle.interest([u], n_users, PF_MODE_ALL, 0): every candidate but adj[u] and u itself,
in order), cut in numpy to the candidates whose corpus values pass the filter, then to its first k;
ids and float32 bits must be equal.  Exits non-zero on any mismatch."""
import json
import os
import sys
import tempfile

import numpy as np

import edge_corpus as ec
import pokec_testlib as tl

pf = tl.product()
F = pf.CandFilter.make

# the filters on E, with the number of users the issue states for each (None: not stated)
E_FILTERS = [
    ("gender1", F(gender=1), 363),
    ("gender1_keep", F(gender=1, keep_missing=True), 433),
    ("age20_29", F(age=(20, 29)), 134),
    ("age129_32767", F(age=(129, 32767)), 624),          # past the sigmoid tables
    ("completion80", F(completion=(80, None)), 781),
    ("region2_4", F(region=(2, 4)), 70),
    ("region2_4_9", F(region=(2, 4, 9)), 19),            # fewer than k = 64
    ("combo", F(gender=1, age=(20, 29), region=(2,)), 15),
    ("gender77", F(gender=77), 1),
    ("gender5", F(gender=5), 0),                         # a value nobody has
    ("region3_9_27", F(region=(3, 9, 27)), 602),         # the 601 byte-identical clones and one more: a top-k of ties
    ("public2_keep", F(public_flag=2, keep_missing=True), None),
    ("everybody", F(completion=(-5, None), keep_missing=True), 1400),
]


def np_pass(c, f):
    """The filter on the corpus arrays, in the domain the corpus was given in."""
    keep = bool(f.flags & pf.PF_FILT_KEEP_MISSING)
    reg = np.asarray(c.region).reshape(-1, 3)
    ok = np.ones(len(c.uid), bool)
    if f.fields & pf.PF_FILT_GENDER:
        ok &= np.where(c.gen < 0, keep, c.gen == f.gender)
    if f.fields & pf.PF_FILT_PUBLIC:
        ok &= np.where(c.pub < 0, keep, c.pub == f.public_flag)
    if f.fields & pf.PF_FILT_AGE:
        ok &= np.where(c.age <= 0, keep, (c.age >= f.age_min) & (c.age <= f.age_max))
    if f.fields & pf.PF_FILT_COMPLETION:
        ok &= np.where(c.comp <= 0, keep, (c.comp >= f.completion_min) & (c.comp <= f.completion_max))
    if f.fields & pf.PF_FILT_REGION:
        for i in range(3):
            if f.region[i] >= 0:
                ok &= np.where(reg[:, i] < 0, keep, reg[:, i] == f.region[i])
    return ok


def same(g, r):
    return list(g[0]) == list(r[0]) and np.array_equal(np.asarray(g[1], np.float32).view(np.uint32),
                                                       np.asarray(r[1], np.float32).view(np.uint32))


class Ref:
    """The oracle's whole ranking per query, computed once and cut per filter."""

    def __init__(self, c, orc):
        self.c, self.orc, self.full, self.pos = c, orc, {}, c.index()

    def ranking(self, u):
        if u not in self.full:
            ids, sc = self.orc.interest([u], self.c.n_users, tl.PF_MODE_ALL, 0)[0]
            self.full[u] = (np.asarray(ids), np.asarray(sc, np.float32), np.array([self.pos[int(x)] for x in ids], np.int64))
        return self.full[u]

    def expect(self, u, mask, k):
        ids, sc, idx = self.ranking(u)
        m = mask[idx] if len(idx) else np.zeros(0, bool)
        return ids[m][:k], sc[m][:k]


def fail(*a):
    print("mismatch", *a, file=sys.stderr)
    return 1


def e_queries():
    idx = sorted(set(ec.PLANTED_QUERIES) | set(ec.CLONE_QUERIES) | {ec.EMPTY_USER, ec.EXCL_CLONES_Q} |
                 set(range(0, ec.N_USERS, 97)))
    return [ec.uid_of(i) for i in idx]


def check_counts_and_rest(name, c, eng, orc, filters, q5):
    """scan_filter_count, the other recommenders under a filter, and the cleared filter."""
    for fname, f, stated in filters:
        eng.set_scan_filter(f)
        want = int(np_pass(c, f).sum())
        if stated is not None and want != stated:
            return fail(name, fname, "numpy count", want, "stated", stated)
        if eng.scan_filter_count() != want:
            return fail(name, fname, "scan_filter_count", eng.scan_filter_count(), "numpy", want)
    eng.clear_scan_filter()
    base = (eng.recommend_graph_registration(q5, 10), eng.recommend_collaborative(q5, 10), eng.recommend_clubs_collab(q5, 10))
    eng.set_scan_filter(gender=1, age=(20, 29))
    under = (eng.recommend_graph_registration(q5, 10), eng.recommend_collaborative(q5, 10), eng.recommend_clubs_collab(q5, 10))
    for what, a, b in zip(("fof interest", "collab", "clubs"), base, under):
        if not all(same(x, y) for x, y in zip(a, b)):
            return fail(name, what, "changed under a filter")
    eng.clear_scan_filter()
    if eng.scan_filter_count() != c.n_users:
        return fail(name, "count without a filter")
    # a malformed filter is refused (PF_EINVAL) and leaves the one in force alone
    eng.set_scan_filter(gender=77)
    bad = [F(gender=1), F(gender=1), F(age=(30, 20)), F(completion=(81, 80)), F(region=(-1, -1, -1))]
    bad[0].fields |= 32
    bad[1].flags |= 2
    for f in bad:
        rc = eng._L.pf_set_scan_filter(eng.h, f)
        if rc != pf.PF_EINVAL or eng.scan_filter_count() != 1:
            return fail(name, "malformed filter", rc, eng.scan_filter_count())
    eng.clear_scan_filter()
    for u in q5:
        if not same(eng.recommend_interest_all([u], 10)[0], orc.interest([u], 10, tl.PF_MODE_ALL, 0)[0]):
            return fail(name, "unfiltered list after clearing", u)
    return 0


def run_one(name, c, q, ks, filters, mode, want_kernel):
    eng, orc = tl.engine(c), tl.Oracle(c)
    try:
        if want_kernel and eng.layout().scan_kernel != want_kernel:
            print(f"{name}: scan kernel {eng.layout().scan_kernel}, wanted {want_kernel}", file=sys.stderr)
            return 1
        ref = Ref(c, orc)
        nonempty = 0
        for fname, f, _ in filters:
            mask = np_pass(c, f)
            for k in ks:
                if mode == "batch":  # 8 queries in one call: the batch instantiation
                    for b in range(0, len(q), 8):
                        qs = (q[b:b + 8] + q[:8])[:8]
                        got = eng.recommend_interest_all(qs, k, filter=f)
                        for u, g in zip(qs, got):
                            if not same(g, ref.expect(u, mask, k)):
                                return fail(name, fname, "batch", u, k)
                            nonempty += len(g[0]) > 0
                else:
                    for u in q:
                        g = eng.recommend_interest_all([u], k, filter=f)[0]
                        if not same(g, ref.expect(u, mask, k)):
                            return fail(name, fname, mode, u, k, list(g[0])[:5], list(ref.expect(u, mask, k)[0])[:5])
                        nonempty += len(g[0]) > 0
            if eng._filter is not None:
                return fail(name, "the previous (no) filter was not restored")
            if fname == "gender5":
                eng.set_scan_filter(f)
                if eng.scan_filter_count() != 0:
                    return fail(name, "gender5 count")
                eng.clear_scan_filter()
            if fname == "everybody":  # equals the unfiltered bits
                for u in q[::5]:
                    if not same(eng.recommend_interest_all([u], ks[-1], filter=f)[0], eng.recommend_interest_all([u], ks[-1])[0]):
                        return fail(name, "everybody vs unfiltered", u)
        if c.n_users > 2 and nonempty == 0:
            return fail(name, "every list is empty")
        if mode == "one" and c.n_users == ec.N_USERS:
            q5 = [ec.uid_of(i) for i in (1, 62, 466, 515, 1020)]
            if check_counts_and_rest(name, c, eng, orc, filters, q5):
                return 1
        return 0
    finally:
        eng.close()


def check_e(mode, want_kernel):
    e = tl.golden_corpus("E")
    filters = list(E_FILTERS)
    q = e_queries()
    if mode == "topk100":
        return run_one("E", e, q[::4] + [ec.uid_of(ec.EXCL_CLONES_Q)], (100,), filters, mode, 0)
    ks = (10, 64) if mode == "batch" else (1, 10, 64)
    if run_one("E", e, q, ks, filters, mode, want_kernel):
        return 1
    # Filters against the query's own exclusions (adj[q] + {q}), which apply on top.  EXCL_CLONES_Q's
    # row names 525 of the 602 users region (3, 9, 27) passes: what is left are the others, none of
    # the row.  gender == 77 passes one user: asked by that user, the filter passes only users of the
    # query's exclusion row, and the list is empty.
    eng = tl.engine(e)
    try:
        u = ec.uid_of(ec.EXCL_CLONES_Q)
        row = {int(x) for i, a in enumerate(e.adj_uid) if int(a) == u for x in e.adj_nbr[e.adj_off[i]:e.adj_off[i + 1]]} | {u}
        f = next(x[1] for x in E_FILTERS if x[0] == "region3_9_27")
        m = np_pass(e, f)
        left = int(sum(1 for x, ok in zip(e.uid, m) if ok and int(x) not in row))
        if not all(m[e.index()[ec.uid_of(i)]] for i in ec.CLONES) or not 64 < left < 100:
            return fail("region (3, 9, 27) should pass every clone and leave 64 < n < 100 outside the row", left)
        g = eng.recommend_interest_all([u], 64, filter=f)[0]
        if len(g[0]) != 64 or any(int(x) in row for x in g[0]):
            return fail("EXCL_CLONES_Q under region (3, 9, 27)", list(g[0]))
        f77 = next(x[1] for x in E_FILTERS if x[0] == "gender77")
        only = [int(x) for x, ok in zip(e.uid, np_pass(e, f77)) if ok]
        g = eng.recommend_interest_all(only, 64, filter=f77)[0]
        if len(only) != 1 or len(g[0]) != 0:
            return fail("a filter passing only the query itself left", list(g[0]))
    finally:
        eng.close()
    small = [x for x in E_FILTERS if x[0] in ("gender1", "combo", "region3_9_27", "gender5")]
    for n in (2, 511, 512, 513, 1025):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        qs = [ec.uid_of(i) for i in range(0, n, max(1, n // 12))] + [ec.uid_of(n - 1)]
        if run_one(f"n{n}", c, qs, (10, 64), [(a, b, None) for a, b, _ in small], mode, want_kernel):
            return 1
    return 0


def merged(parts, k):
    rows = sorted(((-float(s), int(u), np.float32(s)) for g in parts for u, s in zip(g[0], g[1])), key=lambda x: x[:2])[:k]
    return [r[1] for r in rows], np.asarray([r[2] for r in rows], np.float32)


def check_synth(mode, want_kernel):
    n = 20000
    sc = tl.synth.Corpus(n_users=n, seed=3, edge_cases=1)
    ptr = sc.desc_ptr()
    c = tl.corpus_from_desc(ptr)
    eng, orc = tl.engine(ptr), tl.Oracle(None, desc_ptr=ptr)
    try:
        if want_kernel and eng.layout().scan_kernel != want_kernel:
            print(f"synth: scan kernel {eng.layout().scan_kernel}, wanted {want_kernel}", file=sys.stderr)
            return 1
        ref = Ref(c, orc)
        reg = np.asarray(c.region).reshape(-1, 3)
        g0 = int(np.bincount(c.gen[c.gen >= 0]).argmax())
        r0 = int(np.bincount(reg[reg[:, 0] >= 0, 0]).argmax())
        filters = [("gender", F(gender=g0)), ("age20_29", F(age=(20, 29))), ("region", F(region=(r0,))),
                   ("combo", F(gender=g0, age=(20, 29), region=(r0,), keep_missing=True))]
        q = [1, 8, 77, 1500, 2999, 10000, 19999, 20000]
        eng.k5_prune_stats(reset=True)
        scans = 0
        for fname, f in filters:
            mask = np_pass(c, f)
            if not 0 < mask.sum() < n:
                return fail("synth", fname, "passes", int(mask.sum()))
            for k in (10, 64):
                for u in q:
                    want = ref.expect(u, mask, k)
                    g = eng.recommend_interest_all([u], k, filter=f)[0]
                    scans += 1
                    if not same(g, want):
                        return fail("synth", fname, u, k)
                    if k == 10:  # both shards, merged as the prune check merges them
                        parts, cnt = [], 0
                        eng.set_scan_filter(f)
                        for r_ in range(2):
                            eng.set_shard(r_, 2)
                            parts.append(eng.recommend_interest_all([u], k)[0])
                            if u == q[0]:
                                cnt += eng.scan_filter_count()
                        eng.set_shard(0, 1)
                        if u == q[0] and (cnt != int(mask.sum()) or eng.scan_filter_count() != cnt):
                            return fail("synth", fname, "shard counts", cnt, int(mask.sum()))
                        eng.clear_scan_filter()
                        scans += 1  # the two shards together are one pass over the candidates
                        if not same(merged(parts, k), want):
                            return fail("synth shards", fname, u, k)
        print("stats " + json.dumps({**eng.k5_prune_stats(), "scans": scans, "n_users": n}))
        return 0
    finally:
        eng.close()


def check_async():
    """Six one-query scan_keys_async calls on a caller's stream, a different filter set before each
    and no synchronisation between them: every row obeys its own filter, so the filter travels by
    value with the launch."""
    import torch
    e = tl.golden_corpus("E")
    eng, orc = tl.engine(e), tl.Oracle(e)
    try:
        ref = Ref(e, orc)
        q = e_queries()
        names = ("gender1", "age20_29", "region2_4", "gender5", "completion80", "region3_9_27")
        fs = [next(x for x in E_FILTERS if x[0] == nm) for nm in names]
        s = torch.cuda.Stream()
        for k in (10, 64):
            for b in range(0, len(q) - 5, 6):
                us = q[b:b + 6]
                rows = torch.full((6, k), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                for i, (u, (_, f, _)) in enumerate(zip(us, fs)):
                    eng.set_scan_filter(f)
                    eng.scan_keys_async([u], k, rows[i].data_ptr(), s.cuda_stream)
                eng.clear_scan_filter()
                s.synchronize()
                keys = rows.cpu().numpy().view(np.uint64)
                for i, (u, (fname, f, _)) in enumerate(zip(us, fs)):
                    if not same(pf.decode_keys(keys[i]), ref.expect(u, np_pass(e, f), k)):
                        return fail("async", fname, u, k)
        return 0
    finally:
        eng.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "one"
    if mode == "async":
        rc = check_async()
    else:
        want = 1 if "scan=stream" in os.environ.get("PF_DEBUG", "") else (0 if mode == "topk100" else 2)
        rc = check_e(mode, want)
        if rc == 0 and mode == "one":
            rc = check_synth(mode, want)
    if rc:
        return 1
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
