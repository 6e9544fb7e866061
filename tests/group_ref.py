"""Host model of the group query (include/pokec_fas.h "Group query") and the seed sets the group
tests share.

The per-pair floats come from outside: `pairs(a_uids, b_uids) -> float32[]` is the oracle's
fas_pairs (profile_similarity of the reference), or under a field selection the engine's
fas_pairs(select=), which the field-selection tests pin.  The model adds what the group query adds:
seed resolution (unknown uids dropped, the first occurrence of a repeated uid kept), the aggregate
in seed order (the sequential double sum divided by G, or the float minimum / maximum), the
exclusion rules (seeds, exclude, and under exclude_adj every seed's adjacency row), a host filter
mask, and the ranking (score descending, uid ascending)."""
import numpy as np

import edge_corpus as ec

AGGS = ("mean", "min", "max")


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def aggregate(S, agg):
    """S: float32 [G, n], row g = s_g of every user; the aggregate of each column."""
    G = S.shape[0]
    if agg == "mean":
        acc = np.zeros(S.shape[1], np.float64)
        for g in range(G):
            acc = acc + S[g].astype(np.float64)
        return (acc / np.float64(G)).astype(np.float32)
    m = S[0].copy()
    for g in range(1, G):
        x = S[g]
        m = np.where(x < m, x, m) if agg == "min" else np.where(x > m, x, m)
    return m.astype(np.float32)


def np_pass(c, pf, f):
    """A CandFilter on the corpus arrays (the candidate filter's definition, include/pokec_fas.h)."""
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


class GroupRef:
    """The model over corpus c.  Rows of per-seed scores are computed once per seed and shared."""

    def __init__(self, c, pairs):
        self.c, self.pairs, self.pos, self.rows = c, pairs, c.index(), {}
        self.uids = np.asarray(c.uid, np.int32)
        self.adj = {int(u): [int(x) for x in c.adj_nbr[c.adj_off[j]:c.adj_off[j + 1]]] for j, u in enumerate(c.adj_uid)}

    def kept(self, seeds):
        out = []
        for u in seeds:
            u = int(u)
            if u in self.pos and u not in out:
                out.append(u)
        return out

    def row(self, u):
        if u not in self.rows:
            self.rows[u] = np.asarray(self.pairs(np.full(len(self.uids), u, np.int32), self.uids), np.float32)
        return self.rows[u]

    def scores(self, seeds, agg):
        """The aggregate of every user of the corpus (None when no seed is kept)."""
        k = self.kept(seeds)
        return aggregate(np.stack([self.row(u) for u in k]), agg) if k else None

    def candidates(self, seeds, exclude=(), exclude_adj=False, mask=None):
        k = self.kept(seeds)
        drop = set(k) | {int(x) for x in exclude}
        if exclude_adj:
            for u in k:
                drop |= set(self.adj.get(u, ()))
        ok = ~np.isin(self.uids, sorted(drop))
        return ok if mask is None else ok & mask

    def expect(self, seeds, k, agg="mean", exclude=(), exclude_adj=False, mask=None, shard=None):
        """(ids, scores) of the top-k.  shard: a bool mask of the shard's users."""
        sc = self.scores(seeds, agg)
        if sc is None:
            return np.zeros(0, np.int32), np.zeros(0, np.float32)
        ok = self.candidates(seeds, exclude, exclude_adj, mask)
        if shard is not None:
            ok = ok & shard
        idx = np.nonzero(ok)[0]
        order = idx[np.lexsort((self.uids[idx], -sc[idx].astype(np.float64)))][:k]
        return self.uids[order], sc[order]


def same(got, want):
    return list(got[0]) == list(want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


# ---------------------------------------------------------------- seed sets on corpus E (idx)
U = ec.uid_of
UNKNOWN_UIDS = (5, 123456789)                      # no profile in E
SEEDS_CLONES = [441, 766, 1191]                    # every other clone ties: ranks k and k + 1 are equal
SEEDS_MIXED = [ec.EMPTY_USER, 441, ec.Q_LONG[200], ec.HIT_Q_ONE, 600]   # G = 5, the pass tests' set
SEEDS_EXCL = [ec.EXCL_CLONES_Q, ec.EXCL_RUN_Q]      # adjacency rows that name most clones / idx 500..530
SEEDS_PAIR = [ec.HIT_Q_SPREAD, ec.Q_TWO_LONG]       # G = 2
SEEDS_TRIO = [ec.Q_LONG[64], 515, ec.SET_PARTNER]   # G = 3


def seeds_n(G):
    """G distinct idx: the planted users first (EMPTY_USER, a clone, the long-column and hit-list
    users), then a stride over the corpus."""
    out = [ec.EMPTY_USER, 441] + sorted(ec.Q_LONG.values()) + [ec.HIT_Q_ONE, ec.HIT_Q_SPREAD, ec.Q_TWO_LONG]
    i = 0
    while len(out) < G:
        x = (i * 37 + 11) % ec.N_USERS
        if x not in out:
            out.append(x)
        i += 1
    return out[:G]


def uids(idx):
    return [U(i) for i in idx]


def seeds_with_noise():
    """A caller's list with duplicates and unknown uids: three seeds remain, in this order."""
    a, b, c = U(ec.Q_LONG[128]), U(ec.HIT_Q_SPREAD), U(700)
    return [a, UNKNOWN_UIDS[0], b, a, UNKNOWN_UIDS[1], c, b], [a, b, c]


NAMED_SETS = {"clones": SEEDS_CLONES, "mixed": SEEDS_MIXED, "excl": SEEDS_EXCL, "pair": SEEDS_PAIR, "trio": SEEDS_TRIO}
MODEL_G = (2, 3, 5, 16, 17, 64, 65, 200)


def model_sets():
    """{name: seed uids} of the model test: G in MODEL_G."""
    out = {"pair": uids(SEEDS_PAIR), "trio": uids(SEEDS_TRIO), "mixed": uids(SEEDS_MIXED)}
    for G in MODEL_G[3:]:
        out["n%d" % G] = uids(seeds_n(G))
    return out


# the filter of the group tests: keeps >= 64 candidates for every seed set (test_group_cpu asserts it)
FILTER_KW = dict(gender=1, age=(14, 60))
