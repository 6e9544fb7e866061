"""Reference for the field selection of the all-candidates scans (pf_set_scan_select).

The oracle knows no selection.  The expected bits of FAS(A, B | selection) are the oracle's on a
derived corpus: the same users and adjacency, only the selected columns' token rows and their
normaliser slots (idf mode unchanged; with explicit idf maps, the same subset of maps), and each
deselected fixed field blanked for every user (public / gender -1, completion / age 0, all region
parts -1, no clubs, no friends).  A term needs the field on both sides, so blanking it for
everybody equals treating it as missing on the query's side, and 7 + (selected columns) is the
derived corpus' own denominator.
"""
import numpy as np

import pokec_testlib as tl

PUBLIC, GENDER, COMPLETION, AGE, REGION, CLUBS, FRIENDS = range(7)
FIXED_ALL = 0x7F


def selected_cols(cols_mask, n_cols):
    return [t for t in range(n_cols) if (int(cols_mask) >> t) & 1]


def derived_corpus(c, sel):
    """tl.Corpus c under selection sel (anything with .fixed and .cols, e.g. pokec_fas.FieldSelect)."""
    fixed, T = int(sel.fixed), c.n_cols
    keep = selected_cols(sel.cols, T)
    n = c.n_users
    on = lambda k: bool((fixed >> k) & 1)
    pub = c.pub if on(PUBLIC) else np.full(n, -1, np.int32)
    gen = c.gen if on(GENDER) else np.full(n, -1, np.int32)
    comp = c.comp if on(COMPLETION) else np.zeros(n, np.int32)
    age = c.age if on(AGE) else np.zeros(n, np.int32)
    region = c.region if on(REGION) else np.full(3 * n, -1, np.int32)
    zero_off = np.zeros(n + 1, np.int64)
    club_off, clubs = (c.club_off, c.clubs) if on(CLUBS) else (zero_off, np.zeros(0, np.uint32))
    friend_off, friends = (c.friend_off, c.friends) if on(FRIENDS) else (zero_off, np.zeros(0, np.uint32))
    # token rows (u, t) of the selected columns, in ascending column index
    Tk = len(keep)
    off = np.asarray(c.tok_off, np.int64).reshape(-1)
    lo = off[:-1].reshape(n, T)[:, keep].reshape(-1) if Tk else np.zeros(0, np.int64)
    hi = off[1:].reshape(n, T)[:, keep].reshape(-1) if Tk else np.zeros(0, np.int64)
    lens = hi - lo
    tok_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if len(lens) and lens.sum():
        idx = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi) if b > a])
    else:
        idx = np.zeros(0, np.int64)
    slots = list(range(tl.NUM_FIXED)) + [tl.NUM_FIXED + t for t in keep]
    d = tl.Corpus(c.uid, pub, comp, gen, age, region, club_off, clubs, friend_off, friends, tok_off,
                  c.tok_tid[idx], c.tok_tf[idx], c.adj_uid, c.adj_off, c.adj_nbr, Tk, c.norm_present[slots],
                  c.norm_mean[slots], c.norm_sd[slots], c.median,
                  [c.col_names[t] for t in keep] if c.col_names else None)
    if c.desc.idf_mode == tl.PF_IDF_EXPLICIT:
        present = {j for j, t in enumerate(keep) if c.col_has_idf[t]}
        entries = {j: [(int(c.idf_tid[x]), np.float32(c.idf_val[x])) for x in range(int(c.idf_off[t]), int(c.idf_off[t + 1]))]
                   for j, t in enumerate(keep) if c.col_has_idf[t]}
        d.set_explicit_idf(present, entries)
    return d


class SelRef:
    """The derived oracle's whole ranking per query, computed once and cut per filter mask (as
    gpu_scan_filter_check.Ref cuts the base oracle's)."""

    def __init__(self, c, sel):
        self.c = c
        self.d = derived_corpus(c, sel)
        self.orc = tl.Oracle(self.d)
        self.full, self.pos = {}, c.index()

    def ranking(self, u):
        if u not in self.full:
            ids, sc = self.orc.interest([u], self.c.n_users, tl.PF_MODE_ALL, 0)[0]
            self.full[u] = (np.asarray(ids), np.asarray(sc, np.float32), np.array([self.pos[int(x)] for x in ids], np.int64))
        return self.full[u]

    def expect(self, u, k, mask=None):
        ids, sc, idx = self.ranking(u)
        if mask is not None:
            m = mask[idx] if len(idx) else np.zeros(0, bool)
            ids, sc = ids[m], sc[m]
        return ids[:k], sc[:k]

    def fas_pairs(self, a, b):
        return self.orc.fas_pairs(a, b)
