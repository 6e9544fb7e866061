"""Guards of the planted waves (tests/pair_wave_corpus.py), on the CPU: every planted class's item
count, hit count and overflow status is recomputed from the corpus arrays and compared with the
kernels' limits, every composition the GPU tests issue is classified by the host model of
pair_epilogue's split and the categories it claims are asserted, the terms of a planted pair are
shown to differ from one another (so a lane that read a neighbour's term would score differently),
and the oracle alone scores every planted pair finite and in (0, 1).  The GPU tests
(tests/test_gpu_pair_waves.py) rely on these: each guard fails if its class or composition is
edited away."""
import numpy as np
import pytest

import pair_terms_ref as ptr
import pair_wave_corpus as pw
import pokec_testlib as tl

# the kernels' limits, as their sources state them
HIT_CAP = 20        # csrc/pf_types.h:19-22 PF_HIT_CAP / kHitCap
HIT_SLOTS = 24      # csrc/pf_types.h:28 kHitSlots = kHitCap + 4
QUEUE = 384         # csrc/pf_kernels.hip:517 kQueue = kHitSlots * 64 / 4
PAIR_THREADS = 512  # csrc/pf_kernels.h kPairThreads
BYTE_MAX = 255      # csrc/pf_store.cpp:270-276: tf <= 255 and ids < 2^30 keep the packed format
ID_LIMIT = 2**30    # csrc/pf_types.h:50 kIdLimit
MAX_TILE_WORDS = 192  # csrc/pf_types.h:30 kMaxTileSteps = 48 steps of 4 words


@pytest.fixture(scope="module")
def C():
    return pw.corpus()[0]


def instances(name):
    return range(min(pw.CLASSES[name][0], 8))


def test_constants_match_the_builder():
    assert (pw.HIT_CAP, pw.HIT_SLOTS, pw.QUEUE, pw.PAIR_THREADS) == (HIT_CAP, HIT_SLOTS, QUEUE, PAIR_THREADS)
    assert pw.T >= HIT_CAP + 2, "a dense lane can reach 19 hit columns + clubs + friends"
    assert pw.MAX_DENSE_ITEMS == HIT_CAP - 1 + 2 == 21


def test_corpus_is_packed_and_its_twin_is_wide(C):
    W = pw.corpus(wide=True)[0]
    assert C.n_users == W.n_users and 200 <= C.n_users <= 500
    assert int(C.tok_tf.max()) <= BYTE_MAX and int(C.tok_tf.min()) >= 1
    assert int(C.clubs.max()) < ID_LIMIT and int(C.friends.max()) < ID_LIMIT
    assert int(W.tok_tf.max()) == 300 and np.count_nonzero(W.tok_tf != C.tok_tf) == 1
    assert len(C.adj_uid) == 0, "an all-candidates call ranks everyone but the query"
    assert np.array_equal(C.uid, pw.UID0 + np.arange(C.n_users)), "consecutive uids: idx = position"


def test_queries(C):
    _, _, qt = pw.record(C, pw.uid_of("Q"))
    assert all(pw.q_tid(t) in qt[t] for t in range(pw.T))
    assert [len(qt[t]) for t in range(pw.T) if t != pw.COL_LONG] == [1] * (pw.T - 1) and len(qt[pw.COL_LONG]) == 1 + pw.N_LONG
    c1, f1, t1 = pw.record(C, pw.uid_of("Q1"))
    assert len(t1[pw.COL_Q1]) >= HIT_CAP + 5 and c1 and f1
    gc, gf, gt = pw.record(C, pw.uid_of("QG"))
    qc_, qf, _ = pw.record(C, pw.uid_of("Q"))
    assert (gc, gf) == (qc_, qf) and all(set(qt[t]) <= set(gt[t]) for t in range(pw.T)), "QG holds all of Q"
    # QG's table is probed in global memory: keys + values above the staging limit (csrc/pf_scan_host.cpp kStageLimit,
    # image_ref's lds_bytes; csrc/pf_jobs_plan.cpp:760-761), the table sized as csrc/pf_store.cpp:455-459 lg_for (load <= 0.4)
    n = len(gc) + len(gf) + sum(len(m) for m in gt)
    lg = 4
    while (1 << lg) * 2 < n * 5:
        lg += 1
    kv = ((1 << lg) + 16) * 8 + 16 * sum(len(m) for m in gt)
    assert kv > pw.STAGE_LIMIT and 16 * sum(len(m) for m in gt) < pw.STAGE_LIMIT < (1 << lg) * 8
    # and Q's is staged in LDS
    nq = len(qc_) + len(qf) + sum(len(m) for m in qt)
    assert nq * 5 <= (1 << 8) * 2 and ((1 << 8) + 16) * 8 + 16 * nq < pw.STAGE_LIMIT
    # every other class against QG makes the items it makes against Q
    for name in pw.EXPECT:
        assert pw.lane_of_pair(C, pw.uid_of("QG"), pw.uid_of(name))[:3] == pw.lane_of_pair(C, pw.uid_of("Q"), pw.uid_of(name))[:3]


def test_every_class_has_its_items_hits_and_overflow(C):
    assert sorted(n for n in pw.EXPECT if n[0] == "I" and n[1:].isdigit()) == sorted("I%d" % n for n in range(22))
    q = pw.uid_of("Q")
    for name, (items, hits, over) in pw.EXPECT.items():
        for k in instances(name):
            got = pw.lane_of_pair(C, q, pw.uid_of(name, k))
            assert got[:3] == (items, hits, over), (name, k, got)
            assert over == (hits >= HIT_CAP) and (over or items <= pw.MAX_DENSE_ITEMS)
    for n in range(2, 22):  # n - 2 hit columns, a club and a friend item
        cl, fr, tk = pw.record(C, pw.uid_of("I%d" % n))
        assert len(pw.lane_of_pair(C, q, pw.uid_of("I%d" % n))[3]) == n - 2
        assert set(cl) & set(pw.Q_CLUBS) and set(fr) & set(pw.Q_FRIENDS)
    assert pw.EXPECT["I21"][1] == HIT_CAP - 1, "the longest list that is still dense"
    assert pw.EXPECT["OV20"][1] == HIT_CAP and pw.EXPECT["OV21"][1] == HIT_CAP + 1
    for name, (items, hits, over) in pw.EXPECT_Q1.items():
        got = pw.lane_of_pair(C, pw.uid_of("Q1"), pw.uid_of(name))
        assert got[:3] == (items, hits, over) and got[3] == [pw.COL_Q1], (name, got)


def test_variants_without_an_intersection_or_a_field(C):
    rec = lambda name: pw.record(C, pw.uid_of(name))
    shares = lambda ids, q: bool(set(ids) & set(q))
    cl, fr, _ = rec("club_other")
    assert cl and not shares(cl, pw.Q_CLUBS) and shares(fr, pw.Q_FRIENDS)     # the sig0 clubs term, no clubs item
    cl, fr, _ = rec("friend_other")
    assert fr and not shares(fr, pw.Q_FRIENDS) and shares(cl, pw.Q_CLUBS)
    for n in (0, 1):
        cl, fr, _ = rec("I%d" % n)
        assert cl and fr and not shares(cl, pw.Q_CLUBS) and not shares(fr, pw.Q_FRIENDS)
    cl, fr, _ = rec("no_clubs")
    assert not cl and shares(fr, pw.Q_FRIENDS)
    cl, fr, _ = rec("no_friends")
    assert not fr and shares(cl, pw.Q_CLUBS)
    cl, fr, tk = rec("no_sets")
    assert not cl and not fr and any(tk)
    cl, fr, tk = rec("header_only")
    assert not cl and not fr and not any(tk)
    # common columns without a hit between the hit columns: their s = 0 terms sit between the items' terms
    for n in (6, 10, 12, 21):
        _, _, tk = rec("I%d" % n)
        hit = pw.item_cols(n)
        plain = [t for t in range(pw.T) if tk[t] and t not in hit]
        assert plain and any(hit[0] < t < hit[-1] for t in plain), n


def test_headers_cycle_over_the_table_ends_and_missing_fields(C):
    for name in ("I6", "I12", "I21"):
        i0 = pw.uid_of(name) - pw.UID0
        k = slice(i0, i0 + min(pw.CLASSES[name][0], 64))
        if name != "I6":
            assert {0, 1, 128, 129} <= set(C.comp[k].tolist()) and {0, 1, 128, 129} <= set(C.age[k].tolist()), name
            assert -1 in C.gen[k] and -1 in C.pub[k] and 0 in C.gen[k] and 1 in C.gen[k]
            reg = C.region.reshape(-1, 3)[k]
            assert (reg == -1).all(axis=1).any() and (reg >= 0).all(axis=1).any()
    i0 = pw.uid_of("I6") - pw.UID0
    assert len({(int(C.comp[i]), int(C.age[i]), int(C.gen[i])) for i in range(i0, i0 + 4)}) == 4


def test_the_long_overflow_records_cross_a_trip_edge(C):
    """The wave's re-walk reads 64 words a trip from word nset (csrc/pf_kernels.hip:638): MT starts at a
    multiple of 64, UA at a word that is no multiple of 4, both take more than one trip, and the run of
    COL_LONG's hits lies across a trip edge."""
    for name, aligned in (("MT", True), ("UA", False)):
        for k in instances(name):
            cl, fr, tk = pw.record(C, pw.uid_of(name, k))
            nset, ntok = len(cl) + len(fr), sum(len(m) for m in tk)
            assert (nset % 64 == 0 and nset > 0) if aligned else (nset % 4 != 0 and nset % 64 != 0), (name, nset)
            assert ntok > 64 and nset + ntok <= MAX_TILE_WORDS
            assert pw.lane_of_pair(C, pw.uid_of("Q"), pw.uid_of(name, k))[1] > 64, "more than 64 shared tokens"
            first = nset + sum(len(tk[t]) for t in range(pw.COL_LONG))
            words = [first + j for j, tid in enumerate(tk[pw.COL_LONG]) if tid in pw.record(C, pw.uid_of("Q"))[2][pw.COL_LONG]]
            trips = {(w - nset) // 64 for w in words}
            assert len(trips) >= 2, (name, trips)
    for name in ("OV20", "OV21"):
        cl, fr, _ = pw.record(C, pw.uid_of(name))
        assert (len(cl) + len(fr)) % 4 == 0


def test_runs_are_adjacent_in_store_order(C):
    """The store orders slots by record length, longest first, ties by idx (csrc/pf_store.cpp:300-318;
    idx = rank of the uid).  The 127 users of I(12) and of I(21) have consecutive uids and one record
    length each, so each class fills 127 consecutive slots: at least one whole wave of the job
    pipeline's slot-ordered blocks is that class, wherever the blocks are cut."""
    n = C.n_users
    ln = np.diff(C.club_off) + np.diff(C.friend_off) + np.diff(C.tok_off[::pw.T])
    slots = sorted(range(n), key=lambda i: (-int(ln[i]), i))
    for name in ("I12", "I21"):
        assert pw.CLASSES[name][0] >= 127
        i0 = pw.uid_of(name) - pw.UID0
        idx = range(i0, i0 + pw.CLASSES[name][0])
        assert len({int(ln[i]) for i in idx}) == 1
        at = [slots.index(i) for i in idx]
        assert at == list(range(at[0], at[0] + len(at))), name


def test_job_route_has_whole_waves_of_the_runs(C):
    """The all-candidates job's lanes are the profiles in idx order, the query's own lane inactive in
    place (pair_wave_corpus.job_route_pairs): against Q and against QG one wave is 64 x I(12), both
    rounds exactly full, another 64 x I(21), the per-lane fallback; Q1's waves are light."""
    for q in ("Q", "QG"):
        cat = pw.categories(C, pw.job_route_pairs(C, pw.uid_of(q)))
        assert ("two_rounds", 384, 384, 0, 0) in cat and ("per_lane", 378, 966, 0, 0) in cat, (q, cat)
        assert cat[0][4] == 1 and sum(c[4] for c in cat) == 1 + (-C.n_users) % 64, "the query's own lane"
        assert any(c[3] for c in cat)
    assert {c[0] for c in pw.categories(C, pw.job_route_pairs(C, pw.uid_of("Q1")))} == {"one_round"}


REQUIRED = {  # composition -> (kind, total0, total1) of its (first) wave
    "full_384": ("one_round", 384, 0), "385_lane63": ("two_rounds", 378, 7), "385_lane0": ("two_rounds", 379, 6),
    "385_lane31": ("two_rounds", 379, 6), "two_640": ("two_rounds", 380, 260), "two_full_768": ("two_rounds", 384, 384),
    "zero_at_split": ("two_rounds", 384, 217), "zero_after_split": ("two_rounds", 384, 217),
    "zero_after_odd_split": ("two_rounds", 372, 292), "fallback_385_second": ("per_lane", 384, 385),
    "fallback_385_first": ("per_lane", 373, 396), "fallback_all21": ("per_lane", 378, 966),
    "fallback_partial": ("per_lane", 378, 462),
}


def test_compositions_fall_where_they_claim(C):
    for name, (q, lanes, kinds) in pw.COMPOSITIONS.items():
        cat = pw.categories(C, pw.lanes_uids(lanes, q))
        assert [k[0] for k in cat] == kinds, (name, cat)
        if name in REQUIRED:
            assert cat[0][:3] == REQUIRED[name], (name, cat[0])
    assert set(REQUIRED) <= set(pw.COMPOSITIONS)
    cat = lambda name: pw.categories(C, pw.lanes_uids(pw.COMPOSITIONS[name][1], pw.COMPOSITIONS[name][0]))
    lanes = lambda name: pw.COMPOSITIONS[name][1]
    # the I0 lanes at the split: x = 384 exactly (round 0, its first item index is the queue's end); the lane
    # after the first round-1 lane.  (The first round-1 lane itself always has items: its own push x past 384.)
    assert lanes("zero_at_split")[32] == "I0" and lanes("zero_at_split")[:32] == ["I12"] * 32
    assert lanes("zero_after_split")[33] == "I0" and lanes("zero_after_split")[32] == "I7"
    assert lanes("zero_after_odd_split")[32] == "I0" and lanes("zero_after_odd_split")[31] == "I13"
    # the fallback wave with overflowed lanes, zero-item lanes and lanes without a club / friend field
    mix = lanes("fallback_mix")
    assert {"OV20", "MT", "UA", "I0", "no_clubs", "no_friends", "header_only"} <= set(mix) and cat("fallback_mix")[0][3] == 4
    assert cat("fallback_partial")[0][4] == 24 and lanes("fallback_partial") == ["I21"] * 40
    # overflowed lanes in dense waves
    assert lanes("ov_lane0")[0] in pw.EXPECT and pw.EXPECT[lanes("ov_lane0")[0]][2] and cat("ov_lane0")[0][3] == 1
    assert pw.EXPECT[lanes("ov_lane63")[63]][2] and cat("ov_lane63")[0][3] == 1
    assert cat("ov_three")[0][3] == 3 and cat("ov_all64")[0][3] == 64
    assert {"OV20", "OV21", "MT", "UA"} == set(lanes("ov_all64"))
    for name, lane, rnd in (("ov_round0_of_two", 5, 0), ("ov_round1_of_two", 50, 1)):
        ls = lanes(name)
        assert pw.EXPECT[ls[lane]][2] and cat(name)[0][0] == "two_rounds"
        x = sum(pw.EXPECT[c][0] for c in ls[:lane + 1])
        assert (x > QUEUE) == bool(rnd), (name, x)
    assert lanes("ov_multi_trip").count("MT") == 2 and lanes("ov_unaligned").count("UA") == 2
    q1 = pw.categories(C, pw.lanes_uids(lanes("ov_q1_column"), "Q1"))
    assert pw.COMPOSITIONS["ov_q1_column"][0] == "Q1" and q1[0][3] == 2
    # position in the block
    for name, heavy in (("block_two_rounds_037", "two_rounds"), ("block_fallback_037", "per_lane")):
        k = [c[0] for c in cat(name)]
        assert len(k) == 8 and [w for w in range(8) if k[w] == heavy] == [0, 3, 7] and k.count("one_round") == 5
    assert any(c[3] for c in cat("block_two_rounds_037")) and any(c[3] for c in cat("block_fallback_037"))
    for name, n in (("group_513", 513), ("group_1025", 1025)):
        assert len(lanes(name)) == n and n % PAIR_THREADS == 1 and cat(name)[-1][4] == 63
        assert {"two_rounds", "per_lane"} <= {c[0] for c in cat(name)}
    # two groups interleaved in the input arrays
    pairs = pw.interleaved()
    assert [a for a, _ in pairs[:4]] == [pw.uid_of("Q"), pw.uid_of("Q1")] * 2
    assert [c[0] for c in pw.categories(C, pairs)] == ["two_rounds", "one_round"]
    # field selections move a composition to another kind
    for name, (comp, fixed, cols, k0, k1) in pw.SELECTED.items():
        q, ls, _ = pw.COMPOSITIONS[comp]
        assert [c[0] for c in pw.categories(C, pw.lanes_uids(ls, q))] == [k0], name
        assert [c[0] for c in pw.categories(C, pw.lanes_uids(ls, q), fixed, cols)] == [k1], name
    assert pw.SELECTED["select_two_to_one"][3:] == ("two_rounds", "one_round")
    assert pw.SELECTED["select_per_lane_to_dense"][3] == "per_lane" and pw.SELECTED["select_per_lane_to_dense"][4] != "per_lane"
    assert cat(pw.HEAVY_TWO)[0][:3] == ("two_rounds", 384, 384) and cat(pw.HEAVY_FALLBACK)[0][0] == "per_lane"
    assert len(pw.OVERFLOW_COMPOSITIONS) >= 8


def test_model_edges():
    """The model on hand-made waves: the strict > of both tests, flags that remove a lane's items."""
    assert pw.classify([6] * 64) == ("one_round", 384, 0)
    assert pw.classify([6] * 63 + [7]) == ("two_rounds", 378, 7)
    assert pw.classify([12] * 64) == ("two_rounds", 384, 384)
    assert pw.classify([12] * 63 + [13]) == ("per_lane", 384, 385)
    assert pw.classify([21] * 64, overflow=[True] * 64) == ("one_round", 0, 0)
    assert pw.classify([21] * 64, inactive=[False] * 18 + [True] * 46) == ("one_round", 378, 0)
    assert pw.classify([21] * 64, inactive=[False] * 37 + [True] * 27) == ("per_lane", 378, 399)
    assert pw.waves_of([(1, k) for k in range(513)] + [(2, 0)])[-2:] == [(1, [512]), (2, [0])]
    assert [q for q, _ in pw.waves_of([(1, 0), (2, 0), (1, 1)])] == [1, 2]


def _terms(single, a, b):
    """float64[n, 7 + T]: the pairs' terms as a float of each single-field score resolves them
    (tests/pair_terms_ref.py: score = 2 t F / (t + F), so t = s F / (2 F - s))."""
    s = single.scores(a, b).astype(np.float64)
    F = np.where(np.arange(s.shape[1]) < tl.NUM_FIXED, 1.0 / 7.0, 1.0 / 8.0)[None, :]
    return s * F / (2.0 * F - s)


def test_terms_of_a_pair_differ_from_one_another(C):
    """What makes a wrong kk, rbase or total0 visible: a lane that picked the neighbouring item of the
    queue would add another term.  For every planted class, in item order (clubs, friends, the hit
    columns ascending; csrc/pf_kernels.hip:562-578), replacing an item's term by the next item's
    changes the float32 score; and the items of the next lane's user of the class sum to another value."""
    single = ptr.SingleRef(C)
    orc = tl.Oracle(C)
    q = pw.uid_of("Q")
    names = [n for n in pw.EXPECT]
    b = np.array([pw.uid_of(n, k) for n in names for k in instances(n)], np.int32)
    who = [(n, k) for n in names for k in instances(n)]
    a = np.full(len(b), q, np.int32)
    terms, present, want = _terms(single, a, b), ptr.presence(C, a, b), orc.fas_pairs(a, b)
    K = tl.NUM_FIXED
    for j, (name, k) in enumerate(who):
        base = ptr.score_from_row(terms[j], present[j], pw.T)
        assert abs(float(base) - float(want[j])) <= 4e-7, (name, k, base, want[j])   # the terms are the pair's
        _, _, _, hit = pw.lane_of_pair(C, q, int(b[j]))
        cl, fr, _ = pw.record(C, int(b[j]))
        order = ([5] if set(cl) & set(pw.Q_CLUBS) else []) + ([6] if set(fr) & set(pw.Q_FRIENDS) else []) + [K + t for t in hit]
        assert all(present[j][s] for s in order), (name, k)
        for s0, s1 in zip(order, order[1:]):
            row = terms[j].copy()
            row[s0] = row[s1]
            assert abs(terms[j][s0] - terms[j][s1]) > 1e-4, (name, k, s0, s1)
            assert ptr.bits(ptr.score_from_row(row, present[j], pw.T)) != ptr.bits(base), (name, k, s0, s1)
        if k + 1 in instances(name) and name[0] == "I":   # the next lane's user of a class that fills waves
            assert not order or abs(sum(terms[j][s] - terms[j + 1][s] for s in order)) > 1e-5, (name, k)
    orc.close()


def test_oracle_scores_every_planted_pair_in_0_1(C):
    orc = tl.Oracle(C)
    for q in ("Q", "Q1", "QG"):
        b = np.array([u for u in C.uid if u != pw.uid_of(q)], np.int32)
        s = orc.fas_pairs(np.full(len(b), pw.uid_of(q), np.int32), b)
        assert np.isfinite(s).all() and (s > 0).all() and (s < 1).all(), (q, float(s.min()), float(s.max()))
    orc.close()
    W = pw.corpus(wide=True)[0]
    orw = tl.Oracle(W)
    b = np.array([u for u in W.uid if u != pw.uid_of("Q")], np.int32)
    s = orw.fas_pairs(np.full(len(b), pw.uid_of("Q"), np.int32), b)
    assert np.isfinite(s).all() and (s > 0).all() and (s < 1).all()
    orw.close()
