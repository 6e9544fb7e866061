"""Guards of the edge corpus "E" (tests/edge_corpus.py), on the CPU: every planted case is
asserted on the corpus as parsed back from the reference's files, against the kernels' own
limits, so a later edit of the builder cannot silently drop a case.  The GPU tests on E
(tests/test_gpu_edge_domain.py) rely on these."""
import gzip
import os
import tempfile

import numpy as np
import pytest

import edge_corpus as ec
import pokec_testlib as tl

# the kernels' limits, as their sources state them
ROUND_TOKS = 64     # pf_types.h:219 kRoundToks; pf_kernels.hip, K5: "ROUNDS of <= 64 query tokens"
ROUND_CAP = 1536    # pf_types.h:220 kRoundCap = PF_K5_RCAP (6, :217) * kPostThreads (4 waves * 64, :209-210)
ITEM_RUN_MAX = 31   # pf_kernels.hip kItemRunMax
HIT_CAP = 20        # pf_types.h:20-22 PF_HIT_CAP / kHitCap
HIT_SLOTS = 24      # pf_types.h:28 kHitSlots = kHitCap + 4
VAL_TAB = 128       # pf_types.h:16 kValTab
BYTE_MAX = 255      # pf_store.cpp:700 (tf) and :768 (set multiplicity): the packed entry's low byte
BLOCK = 512         # pf_types.h:211 kBlockCands = 2 * kPostThreads
VAL_16 = 32767      # pf_store.cpp:693: completion / age within 16 bits keeps K5 on
ID_LIMIT = 2**30    # club / friend ids at or above it take the wide store


class View:
    """The parsed corpus addressed by idx (rank of the uid), as the engine orders candidates."""

    def __init__(self, c):
        self.c = c
        self.pos = np.argsort(c.uid, kind="stable")       # idx -> row of the parsed corpus
        self.T = c.n_cols
        self._toks = {}

    def uid(self, i):
        return int(self.c.uid[self.pos[i]])

    def toks(self, i, t):
        if (i, t) not in self._toks:
            r = int(self.pos[i]) * self.T + t
            lo, hi = self.c.tok_off[r], self.c.tok_off[r + 1]
            self._toks[(i, t)] = dict(zip(self.c.tok_tid[lo:hi].tolist(), self.c.tok_tf[lo:hi].tolist()))
        return self._toks[(i, t)]

    def clubs(self, i):
        p = self.pos[i]
        return self.c.clubs[self.c.club_off[p]:self.c.club_off[p + 1]].tolist()

    def friends(self, i):
        p = self.pos[i]
        return self.c.friends[self.c.friend_off[p]:self.c.friend_off[p + 1]].tolist()

    def fixed(self, i):
        p = self.pos[i]
        c = self.c
        return (int(c.pub[p]), int(c.comp[p]), int(c.gen[p]), int(c.age[p])) + tuple(c.region[3 * p:3 * p + 3].tolist())

    def row(self, i):
        return (self.fixed(i), self.clubs(i), self.friends(i), [self.toks(i, t) for t in range(self.T)])

    def shared(self, a, b, t):
        """tokens both hold with a positive count (what a postings list or a hit list can see)"""
        A, B = self.toks(a, t), self.toks(b, t)
        return sum(1 for k, v in A.items() if v > 0 and B.get(k, 0) > 0)

    def adj(self, i):
        j = np.nonzero(self.c.adj_uid == self.uid(i))[0]
        if len(j) == 0:
            return None
        return self.c.adj_nbr[self.c.adj_off[j[0]]:self.c.adj_off[j[0] + 1]].tolist()

    def block_entries(self, q, t, block):
        """entries (tf > 0) in idx range `block` of the lists of query q's tokens in column t"""
        want = [k for k, v in self.toks(q, t).items() if v > 0]
        return {k: sum(1 for i in range(*block) if self.toks(i, t).get(k, 0) > 0) for k in want}


@pytest.fixture(scope="module")
def E():
    return View(tl.golden_corpus("E"))


def test_constants_match_the_builder():
    assert ec.BLOCK == BLOCK and ec.DENSE == (BLOCK, 2 * BLOCK) and ec.ID_TOP == ID_LIMIT - 1
    assert ec.N_USERS > 2 * BLOCK + 64


def test_uids_sparse_unordered_large_and_one_repeated_line(E):
    c = E.c
    assert c.n_users == ec.N_USERS
    assert [E.uid(i) for i in range(ec.N_USERS)] == [ec.uid_of(i) for i in range(ec.N_USERS)]
    u = c.uid.astype(np.int64)
    assert np.all(np.diff(np.sort(u)) >= 2), "sparse: no two consecutive uids"
    assert np.count_nonzero(np.diff(u) < 0) > ec.N_USERS // 4, "file order is not ascending"
    assert int(u.max()) == ec.UID_MAX == 2_000_000_000 < 2**31 - 1000
    with tempfile.TemporaryDirectory() as d:
        ec.write_reference_files(d)
        with open(os.path.join(d, "data", "users_encoded.csv")) as f:
            first = [ln.split(",", 1)[0] for ln in f]
    dup = str(ec.uid_of(ec.DUP_LINE_USER))
    assert first.count(dup) == 2 and len(first) == ec.N_USERS + 2
    # the later line's fields win: the earlier one names a club 256 times and an age of 40000
    fx, clubs, _, _ = E.row(ec.DUP_LINE_USER)
    assert clubs == [5, 6] and fx[3] != 40000
    assert E.toks(ec.DUP_LINE_USER, ec.COL_HC) == {ec.HC_TOKENS[0]: 4, ec.HC_TOKENS[3]: 1}


def test_token_count_splits(E):
    assert sorted(ec.Q_LONG) == [ROUND_TOKS, ROUND_TOKS + 1, 2 * ROUND_TOKS, 2 * ROUND_TOKS + 1, 200]
    for n, q in ec.Q_LONG.items():
        tk = E.toks(q, ec.COL_L)
        assert len(tk) == n and min(tk.values()) > 0, n
    a, b = E.toks(ec.Q_TWO_LONG, ec.COL_L), E.toks(ec.Q_TWO_LONG, ec.COL_L2)
    assert ec.COL_L2 == ec.COL_L + 1 and len(a) > ROUND_TOKS and len(b) > ROUND_TOKS
    assert E.shared(ec.Q_TWO_LONG, ec.P_TWO_LONG, ec.COL_L) == 50
    assert E.shared(ec.Q_TWO_LONG, ec.P_TWO_LONG, ec.COL_L2) == 70


def test_entry_count_splits(E):
    blocks = [(0, BLOCK), ec.DENSE, (2 * BLOCK, ec.N_USERS)]
    tfs = set()
    for i in range(*ec.DENSE):                            # every candidate of the block holds the same tokens
        for t, want in ec.D_TOKENS.items():
            tk = E.toks(i, t)
            assert sorted(tk) == want, (i, t)
            tfs.update(tk.values())
    assert tfs == set(range(BYTE_MAX + 1)), "tf cycles over 0..255"
    for q in (515, ec.Q_LONG[200], ec.EXCL_RUN_Q, 441):   # dense, block-0, block-0, clone queries
        ent = {t: E.block_entries(q, t, ec.DENSE) for t in ec.D_TOKENS}
        one = ent[ec.COL_D1]
        assert list(one.values()) == [BLOCK], "a single token's list fills the block"
        for t in (ec.COL_D4, ec.COL_D5):
            assert 4 <= len(ent[t]) < ROUND_TOKS and sum(ent[t].values()) > ROUND_CAP, (q, t)
        big = ent[ec.COL_D200]
        assert len(big) > ROUND_TOKS and sum(big.values()) > ROUND_CAP
        for t in (ec.COL_D1, ec.COL_D4, ec.COL_D5):      # sparse in the other blocks: whole columns there
            for blk in (blocks[0], blocks[2]):
                assert sum(E.block_entries(q, t, blk).values()) <= ROUND_CAP // 2, (q, t, blk)
    K = tl.NUM_FIXED
    c = E.c
    assert set(ec.SPLIT_Z_MODES.values()) <= set(ec.D_TOKENS)
    assert not c.norm_present[K + ec.SPLIT_Z_MODES["absent"]]
    assert c.norm_present[K + ec.SPLIT_Z_MODES["present"]] and c.norm_sd[K + ec.SPLIT_Z_MODES["present"]] > 0
    assert c.norm_present[K + ec.SPLIT_Z_MODES["sd0"]] and c.norm_sd[K + ec.SPLIT_Z_MODES["sd0"]] == 0


def test_runs(E):
    assert sorted(ec.RUNS) == [ITEM_RUN_MAX, ITEM_RUN_MAX + 1, ITEM_RUN_MAX + 2, ROUND_TOKS]
    assert len(E.toks(ec.RUN_Q, ec.COL_L)) <= ROUND_TOKS, "the query's column is one round"
    for blk in ((0, BLOCK), ec.DENSE, (2 * BLOCK, ec.N_USERS)):
        assert sum(E.block_entries(ec.RUN_Q, ec.COL_L, blk).values()) <= ROUND_CAP
    for n, cand in ec.RUNS.items():
        assert E.shared(ec.RUN_Q, cand, ec.COL_L) == n


def test_hit_lists(E):
    counts = sorted(k for _, _, k in ec.HIT_PAIRS)
    assert counts == sorted(2 * [HIT_CAP - 1, HIT_CAP, HIT_CAP + 1, HIT_SLOTS, HIT_SLOTS + 1] + [200])
    for q, cand, k in ec.HIT_PAIRS:
        per_col = [E.shared(q, cand, t) for t in range(E.T)]
        assert sum(per_col) == k, (q, cand)
        if q == ec.HIT_Q_SPREAD:
            assert max(per_col) == 1 and sum(1 for x in per_col if x) == k, "spread over k columns"
        else:
            assert sum(1 for x in per_col if x) == 1


def test_values(E):
    assert VAL_TAB in ec.VALS and VAL_TAB - 1 in ec.VALS and VAL_TAB + 1 in ec.VALS and VAL_16 in ec.VALS and 1 in ec.VALS
    ages, comps = set(), set()
    for i, (age, comp) in ec.VAL_USERS.items():
        fx = E.fixed(i)
        assert (fx[3], fx[1]) == (age, comp)
        ages.add(age)
        comps.add(comp)
    assert ages == comps == set(ec.VALS)
    assert max(int(E.c.age.max()), int(E.c.comp.max())) == VAL_16
    assert E.fixed(ec.COMP_ZERO)[1] == 0 and E.fixed(ec.COMP_MINUS1)[1] == -1
    for i, (pub, gen) in ec.FLAG_USERS.items():
        assert (E.fixed(i)[0], E.fixed(i)[2]) == (pub, gen) and pub > 1 and gen > 1
    regs = {i: E.fixed(i)[4:] for i in ec.REGION_USERS}
    assert regs == ec.REGION_USERS
    assert any(r[0] == r[1] == r[2] > 2**30 for r in regs.values()) and any(-1 in r and max(r) >= 0 for r in regs.values())
    # dense-block candidates carry ages / completions past the table as well, and every clone's age
    assert sum(1 for i in range(*ec.DENSE) if E.fixed(i)[3] > VAL_TAB) > BLOCK // 2
    fx, clubs, friends, toks = E.row(ec.EMPTY_USER)
    assert fx == (-1, -1, -1, 0, -1, -1, -1) and not clubs and not friends and not any(toks)
    assert E.c.median == 0
    _, _, _, toks = E.row(ec.TF0_USER)
    assert [t for t in range(E.T) if toks[t]] == [ec.COL_TF0] and list(toks[ec.COL_TF0].values()) == [0]
    assert sum(1 for i in range(ec.N_USERS) if E.toks(i, ec.COL_TF0)) > 10, "others use that column"
    assert ec.EMPTY_USER in ec.PLANTED_QUERIES and ec.TF0_USER in ec.PLANTED_QUERIES


def test_sets(E):
    reps = sorted(r for _, _, r in ec.SET_USERS.values())
    assert reps == [2, 2, BYTE_MAX, BYTE_MAX]
    for i, (field, x, rep) in ec.SET_USERS.items():
        ids = E.clubs(i) if field == "clubs" else E.friends(i)
        assert ids.count(x) == rep and len(set(ids)) == 3
        partner = E.clubs(ec.SET_PARTNER) if field == "clubs" else E.friends(ec.SET_PARTNER)
        assert x in partner
    assert int(E.c.clubs.max()) == int(E.c.friends.max()) == ID_LIMIT - 1
    assert ec.ID_TOP in E.clubs(ec.SET_TOP) and ec.ID_TOP in E.clubs(ec.SET_PARTNER)
    assert ec.ID_TOP in E.friends(ec.SET_TOP) and E.friends(ec.SET_PARTNER).count(ec.ID_TOP) == 2
    # no profile repeats an id more than 255 times (K5 stays on)
    for i in range(ec.N_USERS):
        for ids in (E.clubs(i), E.friends(i)):
            assert not ids or max(ids.count(x) for x in set(ids)) <= BYTE_MAX


def test_clones_and_ties(E):
    assert len(ec.CLONES) >= 600
    first = E.row(ec.CLONES[0])
    assert first[1] and first[2] and any(first[3])
    for i in ec.CLONES:
        assert E.row(i) == first, i
    below, inside, above = [sum(1 for i in ec.CLONES if lo <= i < hi)
                            for lo, hi in ((0, BLOCK), ec.DENSE, (2 * BLOCK, ec.N_USERS))]
    assert below >= 32 and inside >= 256 and above >= 64
    assert BLOCK - 1 in ec.CLONES and BLOCK + 1 in ec.CLONES and 2 * BLOCK - 1 in ec.CLONES and 2 * BLOCK + 2 in ec.CLONES
    assert any(b - a > 1 for a, b in zip(ec.CLONES, ec.CLONES[1:])), "idx (and uids) not contiguous"
    for i in range(*ec.CLONE_RANGE):
        if i not in ec.CLONES:
            assert E.row(i) != first
    orc = tl.Oracle(E.c)
    q = [ec.uid_of(i) for i in ec.CLONE_QUERIES + [ec.EXCL_CLONES_Q]]
    clone_uids = [ec.uid_of(i) for i in ec.CLONES]
    for u, (ids, sc) in zip(q, orc.interest(q, 200, tl.PF_MODE_ALL, 0)):
        bits = sc.view(np.uint32)
        nbest = int(np.count_nonzero(bits == bits[0]))
        assert nbest >= 64, (u, nbest)                   # the top-64 is decided by uid alone
        excl = set(E.adj(ec.CLONES[clone_uids.index(u)]) or []) | {u}
        assert list(ids[:64]) == [x for x in clone_uids if x not in excl][:64], u
    # the user without any field scores 0.0 against everyone: 1,399 tied candidates
    (ids, sc), = orc.interest([ec.uid_of(ec.EMPTY_USER)], 64, tl.PF_MODE_ALL, 0)
    assert not sc.view(np.uint32).any() and list(ids) == [ec.uid_of(i) for i in range(65) if i != ec.EMPTY_USER][:64]
    orc.close()


def test_adjacency_exclusions(E):
    lo, hi = ec.EXCL_RUN
    assert lo < BLOCK < hi and E.adj(ec.EXCL_RUN_Q) == [ec.uid_of(j) for j in range(lo, hi)]
    row = set(E.adj(ec.EXCL_CLONES_Q))
    clone_uids = {ec.uid_of(i) for i in ec.CLONES}
    assert ec.EXCL_CLONES_Q in ec.CLONES and row <= clone_uids and len(row) > len(clone_uids) * 3 // 4
    kept = [i for i in ec.EXCL_CLONES_KEPT if i != ec.EXCL_CLONES_Q]
    assert len(kept) >= 64 and min(kept) < BLOCK and max(kept) >= 2 * BLOCK
    assert all(ec.uid_of(i) not in row for i in kept)
    assert E.adj(ec.EMPTY_USER) is None
    assert any(x not in set(E.c.uid.tolist()) for r in range(ec.N_USERS) for x in (E.adj(r) or [])[-2:]), "unknown uids"


def test_goldens_hold_the_planted_cases():
    for fn in ("all.txt", "idf_explicit_all.txt"):
        have = {k[1] for k in tl.golden_lists("E", fn)}
        assert {ec.uid_of(i) for i in ec.PLANTED_QUERIES} <= have, fn
    have = {k[1] for k in tl.golden_lists("E", "recs.txt")}
    assert {ec.uid_of(i) for i in ec.PLANTED_QUERIES} <= have
    for fn in ("pairs.txt", "idf_explicit_pairs.txt"):
        a, b, _ = tl.golden_pairs_file("E", fn)
        got = set(zip(a.tolist(), b.tolist()))
        for x, y in ec.planted_pairs():
            assert (ec.uid_of(x), ec.uid_of(y)) in got, (fn, x, y)
        for q, cand, _ in ec.HIT_PAIRS:
            assert (ec.uid_of(cand), ec.uid_of(q)) in got
    present, entries = tl.golden_explicit_idf("E")
    assert ec.COL_L not in present, "the raw-count cosine column is a long one"
    assert ec.SPLIT_Z_MODES["absent"] not in present and ec.COL_D200 in present


def test_golden_files_within_the_largest_committed_before():
    size = lambda name: {fn: os.path.getsize(os.path.join(tl.GOLDEN, name, fn)) for fn in os.listdir(os.path.join(tl.GOLDEN, name))}
    largest = max(max(size("A").values()), max(size("B").values()))
    assert max(size("E").values()) <= largest
    with gzip.open(os.path.join(tl.GOLDEN, "E", "profiles.txt.gz"), "rt") as f:
        assert sum(1 for _ in f) == ec.N_USERS + 2


@pytest.mark.parametrize("n", [2, 511, 512, 513, 1025])
def test_slices_parse(n):
    """The first n users of E (by idx) as a corpus of their own, for the size tests."""
    with tempfile.TemporaryDirectory() as d:
        ec.write_reference_files(d, n_first=n)
        c = tl.read_reference_dir(d)
    assert sorted(c.uid.tolist()) == [ec.uid_of(i) for i in range(n)]
    assert set(c.adj_uid.tolist()) <= set(c.uid.tolist())
