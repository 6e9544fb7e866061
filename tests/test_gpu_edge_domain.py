"""GPU parity on the edge corpus "E" (tests/edge_corpus.py; its planted cases are asserted by
tests/test_edge_corpus_cpu.py): columns split over K5 rounds, runs at kItemRunMax, hit lists at
kHitCap / kHitSlots, ages and completions past the sigmoid tables, tf and set multiplicities of
255, hundreds of tied scores over block and shard edges, sparse unordered uids, tiny corpora.

Every comparison is bit-exact, ids and float32 bits: against goldens of the real reference
(tests/golden/E) and against the oracle, which tests/test_oracle_golden.py pins to the reference
on this corpus."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import edge_corpus as ec
import pokec_testlib as tl

pytestmark = pytest.mark.gpu
SCAN_KERNELS = {"stream": 1, "postings": 2}


@pytest.fixture(scope="module")
def edge():
    c = tl.golden_corpus("E")
    return c, tl.engine(c), tl.Oracle(c)


@pytest.fixture(scope="module")
def oracle_top64(edge):
    """The oracle's all-candidates top-64 of every user of E (computed once, read only)."""
    c, eng, orc = edge
    q = [ec.uid_of(i) for i in range(ec.N_USERS)]
    return dict(zip(q, orc.interest(q, 64, tl.PF_MODE_ALL, 0)))


def _same(got, ref, ctx):
    assert list(got[0]) == list(ref[0]), ctx
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(ref[1], np.float32).view(np.uint32)), ctx


def _check_lists(got, items, ctx):
    assert list(got[0]) == [x for x, _ in items], ctx
    assert list(got[1].view(np.uint32)) == [h for _, h in items], ctx


def test_layout_is_the_fast_one(edge):
    """E stays inside the packed store and the postings scan: tf and multiplicities <= 255, ids
    < 2^30, ages and completions within 16 bits."""
    c, eng, orc = edge
    assert eng.layout().packed_tokens == 1 and eng.layout().scan_kernel == 2
    assert eng.num_users == ec.N_USERS


def test_idf_matches_reference(edge):
    c, eng, orc = edge
    N, rows = tl.golden_idf("E")
    got = np.array([np.float32(eng.idf(t, k)).view(np.uint32) for t, k, _ in rows], np.uint32)
    assert np.array_equal(got, np.array([h for _, _, h in rows], np.uint32))


def test_fas_pairs_match_reference(edge):
    """K1' on every golden pair: 20,000 random ones and the planted ones in both orders (hit
    lists of 19, 20, 21, 24, 25 and 200 shared tokens, in one column and spread over columns;
    runs; values past the tables; sets with multiplicity 255; the empty user)."""
    c, eng, orc = edge
    a, b, s = tl.golden_pairs("E")
    have = set(zip(a.tolist(), b.tolist()))
    for q, cand, k in ec.HIT_PAIRS:
        assert (ec.uid_of(q), ec.uid_of(cand)) in have and (ec.uid_of(cand), ec.uid_of(q)) in have, k
    got = eng.fas_pairs(a, b).view(np.uint32)
    bad = np.nonzero(got != s)[0]
    assert len(bad) == 0, (len(bad), [(int(a[i]), int(b[i])) for i in bad[:8]])


@pytest.mark.parametrize("kernel", list(SCAN_KERNELS))
def test_all_candidates_match_reference(edge, oracle_top64, kernel):
    """The golden queries (every 23rd user and the planted ones) at top-1, 10, 50 against the
    reference's top-50, and at top-64 against the oracle."""
    c, eng, orc = edge
    eng.set_scan_kernel(SCAN_KERNELS[kernel])
    try:
        assert eng.layout().scan_kernel == SCAN_KERNELS[kernel]
        g = tl.golden_lists("E", "all.txt")
        keys = list(g.keys())
        uids = [k[1] for k in keys]
        for k in (1, 10, 50):
            for key, res in zip(keys, eng.recommend_interest_all(uids, k)):
                _check_lists(res, g[key][:k], (k,) + key)
        for key, res in zip(keys, eng.recommend_interest_all(uids, 64)):
            _check_lists((res[0][:50], res[1][:50]), g[key], (64,) + key)
            if key[1] in oracle_top64:
                _same(res, oracle_top64[key[1]], (64,) + key)
            else:
                assert len(res[0]) == 0, key          # unknown users
    finally:
        eng.set_scan_kernel(0)


def test_every_user_on_both_kernels(edge, oracle_top64):
    """Every user of E as a query at top-64: K5 against K1 and both against the oracle, so every
    candidate of the dense block and every clone is also a query."""
    c, eng, orc = edge
    q = list(oracle_top64)
    try:
        eng.set_scan_kernel(2)
        post = eng.recommend_interest_all(q, 64)
        eng.set_scan_kernel(1)
        stream = eng.recommend_interest_all(q, 64)
    finally:
        eng.set_scan_kernel(0)
    for u, p, s in zip(q, post, stream):
        _same(p, s, ("K5 vs K1", u))
        _same(p, oracle_top64[u], ("K5 vs oracle", u))


def test_recommenders_match_reference(edge):
    """Interest (FoF), collaborative and clubs through the device job pipeline against recs.txt,
    each (recommender, top-k, limit) group in one call."""
    c, eng, orc = edge
    groups = {}
    for key, items in tl.golden_lists("E", "recs.txt").items():
        groups.setdefault((key[0], key[2], key[3]), []).append((key[1], items))
    assert len(groups) == 22
    for (tag, k, lim), rows in groups.items():
        uids = [u for u, _ in rows]
        kk = min(k, 100000)
        if tag in ("graph", "interest"):
            got = eng.recommend_interest(uids, kk, tl.PF_MODE_FOF, lim)
        elif tag == "collab":
            got = eng.recommend_collaborative(uids, kk, lim)
        else:
            got = eng.recommend_clubs_collab(uids, kk, lim)
        for (u, items), res in zip(rows, got):
            _check_lists(res, items, (tag, u, k, lim))


def test_explicit_idf_matches_reference():
    """PF_IDF_EXPLICIT on E: the long column COL_L takes the raw-count cosine, a split column of
    the dense block as well; pairs, all-candidates on both kernels and the recommenders."""
    c = tl.explicit_idf_corpus("E")
    eng = tl.engine(c)
    present, entries = tl.golden_explicit_idf("E")
    assert ec.COL_L not in present
    for t in range(c.n_cols):
        assert np.isnan(eng.idf(t, 1)) == (t not in present), t
    a, b, s = tl.golden_pairs_file("E", "idf_explicit_pairs.txt")
    assert int(np.count_nonzero(eng.fas_pairs(a, b).view(np.uint32) != s)) == 0
    g = tl.golden_lists("E", "idf_explicit_all.txt")
    keys = list(g.keys())
    for kern in (1, 2):
        eng.set_scan_kernel(kern)
        for key, res in zip(keys, eng.recommend_interest_all([k[1] for k in keys], 50)):
            _check_lists(res, g[key], (kern,) + key)
    eng.set_scan_kernel(0)
    groups = {}
    for key, items in tl.golden_lists("E", "idf_explicit_recs.txt").items():
        groups.setdefault((key[0], key[2], key[3]), []).append((key[1], items))
    for (tag, k, lim), rows in groups.items():
        uids = [u for u, _ in rows]
        fn = {"collab": eng.recommend_collaborative, "clubs": eng.recommend_clubs_collab}.get(tag)
        got = fn(uids, k, lim) if fn else eng.recommend_interest(uids, k, tl.PF_MODE_FOF, lim)
        for (u, items), res in zip(rows, got):
            _check_lists(res, items, (tag, u, k, lim))
    eng.close()


def _expected_clone_top(c, qi, k=64):
    """The first k clone uids that query idx qi does not exclude."""
    u = ec.uid_of(qi)
    j = np.nonzero(c.adj_uid == u)[0]
    excl = set(c.adj_nbr[c.adj_off[j[0]]:c.adj_off[j[0] + 1]].tolist()) if len(j) else set()
    return [x for x in (ec.uid_of(i) for i in ec.CLONES) if x != u and x not in excl][:k]


CLONE_Q = ec.CLONE_QUERIES + [ec.EXCL_CLONES_Q]


@pytest.mark.parametrize("kernel", list(SCAN_KERNELS))
def test_ties_are_broken_by_uid(edge, oracle_top64, kernel):
    """A clone's top-64 is 64 other clones with one score: strictly ascending uids, over the 512
    and 1024 block edges, also for the clone that excludes seven eighths of them; the user without
    any field ties every candidate at 0.0."""
    c, eng, orc = edge
    q = [ec.uid_of(i) for i in CLONE_Q] + [ec.uid_of(ec.EMPTY_USER)]
    eng.set_scan_kernel(SCAN_KERNELS[kernel])
    try:
        got = eng.recommend_interest_all(q, 64)
    finally:
        eng.set_scan_kernel(0)
    for qi, u, (ids, sc) in zip(CLONE_Q, q, got):
        bits = sc.view(np.uint32)
        assert len(ids) == 64 and np.all(bits == bits[0]), u
        assert np.all(np.diff(ids.astype(np.int64)) > 0), u
        assert list(ids) == _expected_clone_top(c, qi), u
        _same((ids, sc), oracle_top64[u], u)
    ids, sc = got[-1]
    assert not sc.view(np.uint32).any() and np.all(np.diff(ids.astype(np.int64)) > 0)
    _same((ids, sc), oracle_top64[q[-1]], "empty user")
    kept = _expected_clone_top(c, ec.EXCL_CLONES_Q)
    assert kept[0] < ec.uid_of(ec.BLOCK) and kept[-1] > ec.uid_of(ec.BLOCK)   # its 64 cross a block edge


def test_ties_over_shard_edges(edge, oracle_top64):
    """The clone queries under pf_set_shard with 2, 3 and 5 shards (E has 3 K5 blocks, so some
    shards are empty), merged as the multi-GPU step does, equal the single-GPU result; every shard
    edge lies inside the clone range."""
    import torch
    pf = tl.product()
    c, eng, orc = edge
    q = np.array([ec.uid_of(i) for i in CLONE_Q] + [ec.uid_of(ec.EMPTY_USER), ec.uid_of(515)], np.int32)
    k = 64
    eng2 = tl.engine(c)
    s = torch.cuda.Stream()
    try:
        for world, kern in ((2, 2), (3, 2), (5, 2), (2, 1), (3, 1), (5, 1)):
            eng2.set_scan_kernel(kern)
            parts = torch.empty((world, len(q), k), dtype=torch.int64, device="cuda")
            edges, at = [], 0
            for r in range(world):
                eng2.set_shard(r, world)
                at += eng2.layout().shard_cands
                edges.append(at)
                eng2.scan_keys_async(q, k, parts[r].data_ptr(), s.cuda_stream)
            assert edges[-1] == ec.N_USERS
            if kern == 2:  # contiguous idx ranges: the cuts fall between clones
                cuts = sorted(set(e for e in edges[:-1] if 0 < e < ec.N_USERS))
                assert cuts, world
                for e in cuts:
                    assert ec.CLONE_RANGE[0] < e < ec.CLONE_RANGE[1] and (e - 1) in ec.CLONES and e in ec.CLONES, (world, e)
            out = torch.empty((len(q), k), dtype=torch.int64, device="cuda")
            eng2.merge_keys_async(parts.data_ptr(), world, len(q), k, out.data_ptr(), s.cuda_stream)
            s.synchronize()
            keys = out.cpu().numpy().view(np.uint64)
            for i, u in enumerate(q):
                _same(pf.decode_keys(keys[i]), oracle_top64[int(u)], (world, kern, int(u)))
    finally:
        eng2.set_shard(0, 1)
        eng2.set_scan_kernel(0)
        eng2.close()


@pytest.mark.parametrize("n", [2, 511, 512, 513, 1025])
def test_corpus_sizes(n):
    """The first n users of E as a corpus: one short block, one block less one, exactly one, one
    plus one, two plus one; top-64 and top-1, so fewer than k come back where n - 1 - |excluded|
    < k.  Every user is a query, on both kernels, against the oracle."""
    with tempfile.TemporaryDirectory() as d:
        ec.write_reference_files(d, n_first=n)
        c = tl.read_reference_dir(d)
    assert c.n_users == n
    eng, orc = tl.engine(c), tl.Oracle(c)
    q = [ec.uid_of(i) for i in range(n)][:: (1 if n <= 513 else 3)] + [ec.uid_of(n - 1), 5]
    try:
        for k in (64, 1):
            ref = orc.interest(q, k, tl.PF_MODE_ALL, 0)
            if n - 1 < k:
                assert max(len(r[0]) for r in ref) <= n - 1
            for kern in (2, 1):
                eng.set_scan_kernel(kern)
                for u, g, r in zip(q, eng.recommend_interest_all(q, k), ref):
                    _same(g, r, (n, k, kern, u))
        eng.set_scan_kernel(0)
        qs = q[:: max(1, len(q) // 40)]
        for g, r in zip(eng.recommend_collaborative(qs, 64, 1000), orc.collab(qs, 64, 1000)):
            _same(g, r, (n, "collab"))
    finally:
        eng.close()
        orc.close()


def _copy(c, **over):
    """A deep copy of numpy Corpus c with some arrays replaced."""
    f = dict(uid=c.uid, pub=c.pub, comp=c.comp, gen=c.gen, age=c.age, region=c.region, club_off=c.club_off,
             clubs=c.clubs, friend_off=c.friend_off, friends=c.friends, tok_off=c.tok_off, tok_tid=c.tok_tid,
             tok_tf=c.tok_tf, adj_uid=c.adj_uid, adj_off=c.adj_off, adj_nbr=c.adj_nbr)
    f = {k: np.array(over.get(k, v), copy=True) for k, v in f.items()}
    return tl.Corpus(n_cols=c.n_cols, norm_present=c.norm_present.copy(), norm_mean=c.norm_mean.copy(),
                     norm_sd=c.norm_sd.copy(), median=c.median, col_names=c.col_names, **f)


def _edit_club_256(c):
    i = int(np.nonzero(c.uid == ec.uid_of(56))[0][0])      # SET_USERS[56]: CLUB_Y 255 times
    assert ec.SET_USERS[56] == ("clubs", ec.CLUB_Y, 255)
    at = int(c.club_off[i]) + 1
    assert c.clubs[at] == ec.CLUB_Y
    off = c.club_off.copy()
    off[i + 1:] += 1
    return _copy(c, clubs=np.insert(c.clubs, at, ec.CLUB_Y), club_off=off)


def _edit_age_40000(c):
    age = c.age.copy()
    age[int(np.nonzero(c.uid == ec.uid_of(600))[0][0])] = 40000
    return _copy(c, age=age)


def _edit_ids_2_30(c):
    clubs, friends = c.clubs.copy(), c.friends.copy()
    assert (clubs == ec.ID_TOP).sum() >= 2 and (friends == ec.ID_TOP).sum() >= 2
    clubs[clubs == ec.ID_TOP] = 2**30
    friends[friends == ec.ID_TOP] = 2**31 + 7
    return _copy(c, clubs=clubs, friends=friends)


@pytest.mark.parametrize("edit,packed,kernel", [(_edit_club_256, 1, 1), (_edit_age_40000, 1, 1), (_edit_ids_2_30, 0, 2)],
                         ids=["club-256-times", "age-40000", "ids-at-2^30"])
def test_fallback_contexts(edit, packed, kernel):
    """E with one value past an encoding limit: the store keeps (or widens) its format and the
    scan falls back to K1 (or stays on K5) as documented, and results stay bit-exact.  Forcing K5
    where the postings store was refused is an error, not a wrong answer."""
    pf = tl.product()
    c = edit(tl.golden_corpus("E"))
    eng, orc = tl.engine(c), tl.Oracle(c)
    try:
        lay = eng.layout()
        assert (lay.packed_tokens, lay.scan_kernel) == (packed, kernel)
        if kernel == 1:
            with pytest.raises(pf.FasError, match="postings store unavailable"):
                eng.set_scan_kernel(2)
        pairs = ec.planted_pairs() + [(56, 59), (59, 56), (600, 441), (441, 600), (60, 59), (59, 60)]
        a = np.array([ec.uid_of(x) for x, _ in pairs], np.int32)
        b = np.array([ec.uid_of(y) for _, y in pairs], np.int32)
        assert np.array_equal(eng.fas_pairs(a, b).view(np.uint32), orc.fas_pairs(a, b).view(np.uint32))
        q = [ec.uid_of(i) for i in ec.PLANTED_QUERIES + [56, 59, 60, 600]]
        ref = orc.interest(q, 64, tl.PF_MODE_ALL, 0)
        for kern in ((1,) if kernel == 1 else (2, 1)):
            eng.set_scan_kernel(kern)
            for u, g, r in zip(q, eng.recommend_interest_all(q, 64), ref):
                _same(g, r, (kern, u))
        eng.set_scan_kernel(0)
        qs = q[::6]
        for g, r in zip(eng.recommend_clubs_collab(qs, 20, 1000), orc.clubs(qs, 20, 1000)):
            _same(g, r, "clubs")
    finally:
        eng.close()
        orc.close()


@pytest.mark.parametrize("debug", ["scan=postings,k5_block=64", "scan=postings,k5_block=333", "scan=postings,k5_wgs=16",
                                   "resident_images=0", "scan=stream,tile_steps=1,stage_limit=0"])
def test_forced_variants_on_edge_corpus(debug):
    """E under forced kernel variants, each in a fresh process (PF_DEBUG is read once): K5 blocks
    of 64 and 333 candidates (other split points, other block edges through the clones and the
    dense range), few workgroups claiming blocks, per-call query images, K1 with records split over
    lanes and its tables in global memory."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "gpu_edge_check.py")],
                       env={**os.environ, "PF_DEBUG": debug}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
