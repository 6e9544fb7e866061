"""Reference for the FAS score breakdown (pf_fas_pairs_terms).

The oracle returns whole scores only.  A term is pinned through single-field corpora: the derived
corpus of tests/field_select_ref.py that keeps exactly one slot (fixed = 1 << k, cols = 0, or
fixed = 0, cols = 1 << t).  On it the reference's score of a pair is 0.0 where the field is absent
on either side, and otherwise (float)((2 * term * F) / (term + F)) with used = 1, so S = term and
F = 1 / 7 for a fixed field (no column left) or 1 / 8 for a column.  So
  - the slot is present exactly where the single-field oracle's score is > 0, and
  - the engine's double term, pushed through that expression in float64 (the same operations in the
    same order) and cast to float32, must have the single-field oracle's bits.
This pins a term to what a float of its FAS resolves, not to its last double bits; the whole-score
check (the score recomputed from the row equals the base oracle's bits) closes part of that gap.
"""
import numpy as np

import edge_corpus as ec
import field_select_ref as fsr
import pokec_testlib as tl

NUM_FIXED = 7


class Sel:
    """What field_select_ref needs of a selection."""

    def __init__(self, fixed, cols):
        self.fixed, self.cols = fixed, cols


def single_field_sel(slot):
    return Sel(1 << slot, 0) if slot < NUM_FIXED else Sel(0, 1 << (slot - NUM_FIXED))


def e_pairs():
    """(a idx, b idx): the planted pairs (both orders: the hit-list pairs on both sides of kHitCap,
    the empty user, the tf = 0 user, a == b, values past the sigmoid tables, set multiplicities 2 and
    255, the dense columns of the three normaliser modes) and the hit pairs in both orders again."""
    return ec.planted_pairs() + [(x, y) for x, y, _ in ec.HIT_PAIRS] + [(y, x) for x, y, _ in ec.HIT_PAIRS]


def uid_arrays(pairs):
    return (np.array([ec.uid_of(x) for x, _ in pairs], np.int32), np.array([ec.uid_of(y) for _, y in pairs], np.int32))


def presence(c, a_uid, b_uid):
    """bool[n, 7 + T] from the corpus arrays: the reference adds a slot's term when the field is
    filled in on both sides (recommender_similarity.cpp:38-114)."""
    pos, T = c.index(), c.n_cols
    ia = np.array([pos[int(u)] for u in a_uid], np.int64)
    ib = np.array([pos[int(u)] for u in b_uid], np.int64)
    reg = np.asarray(c.region).reshape(-1, 3)
    nclub = np.diff(np.asarray(c.club_off, np.int64))
    nfriend = np.diff(np.asarray(c.friend_off, np.int64))
    ntok = np.diff(np.asarray(c.tok_off, np.int64).reshape(-1)).reshape(-1, T)
    has = np.stack([np.asarray(c.pub) >= 0, np.asarray(c.gen) >= 0, np.asarray(c.comp) > 0, np.asarray(c.age) > 0,
                    (reg >= 0).any(axis=1), nclub > 0, nfriend > 0], axis=1)
    has = np.concatenate([has, ntok > 0], axis=1)
    return has[ia] & has[ib]


class SingleRef:
    """The 7 + T single-field oracles of corpus c, built once (the derived corpora are the cost)."""

    def __init__(self, c):
        self.c = c
        self.refs = [fsr.SelRef(c, single_field_sel(s)) for s in range(NUM_FIXED + c.n_cols)]

    def scores(self, a_uid, b_uid):
        """f32[n, 7 + T]: column s = the pairs' scores on the corpus that keeps slot s alone."""
        out = np.zeros((len(a_uid), len(self.refs)), np.float32)
        for s, r in enumerate(self.refs):
            out[:, s] = r.fas_pairs(a_uid, b_uid)
        return out


def single_score_of_terms(terms):
    """f32[n, 7 + T]: each term as the score of its single-field corpus, fas_score's operations in
    float64: used = 1, S = term, F = 1 / 7 (a fixed field) or 1 / 8 (a column)."""
    terms = np.asarray(terms, np.float64)
    F = np.where(np.arange(terms.shape[1]) < NUM_FIXED, 1.0 / 7.0, 1.0 / 8.0)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2.0 * terms * F) / (terms + F)).astype(np.float32)


def score_from_row(row, present, n_den_cols):
    """The reference's score from one row: a sequential float64 sum over the present slots in
    ascending order, S = sum / used, F = used / (7 + T'), (float)(2SF / (S + F))."""
    used, total = 0, 0.0
    for s in range(len(row)):
        if present[s]:
            total = total + float(row[s])
            used += 1
    if used == 0:
        return np.float32(0.0)
    S = total / float(used)
    F = float(used) / float(NUM_FIXED + n_den_cols)
    if S <= 0.0 and F <= 0.0:
        return np.float32(0.0)
    return np.float32((2.0 * S * F) / (S + F))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
