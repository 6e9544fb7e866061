"""The group query's host model (tests/group_ref.py) on corpus E with the oracle alone, so that the
GPU tests, which compare the engine with this model, cannot pass vacuously: the planted seed sets
tell the three aggregates apart, tie at the cut of a top-k among E's byte-identical clones, react to
exclude_adj and keep enough candidates under the tests' filter.  Also the ctypes structs against
include/pokec_fas.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import edge_corpus as ec
import group_ref as gr
import pokec_testlib as tl

pf = tl.product()
IDX = {ec.uid_of(i): i for i in range(ec.N_USERS)}   # uid -> idx (the rank of the uid)


@pytest.fixture(scope="module")
def model():
    c = tl.golden_corpus("E")
    orc = tl.Oracle(c)
    yield gr.GroupRef(c, orc.fas_pairs)
    orc.close()


def all_sets():
    s = dict(gr.model_sets())
    s.update({k: gr.uids(v) for k, v in gr.NAMED_SETS.items()})
    return s


def test_aggregate_definition():
    """The sequential double sum, not a float sum and not a pairwise one; min / max of floats; G = 1."""
    S = np.array([[0.1, 1e-8, 0.5], [0.2, 1.0, 0.25], [0.7, -1.0, 0.125]], np.float32)
    for j in range(3):
        acc = 0.0
        for g in range(3):
            acc += float(S[g, j])
        assert gr.bits(gr.aggregate(S, "mean"))[j] == gr.bits(np.float32(acc / 3.0))
    assert list(gr.aggregate(S, "min")) == [S[:, j].min() for j in range(3)]
    assert list(gr.aggregate(S, "max")) == [S[:, j].max() for j in range(3)]
    for a in gr.AGGS:
        assert np.array_equal(gr.bits(gr.aggregate(S[1:2], a)), gr.bits(S[1]))


def test_seed_resolution(model):
    noisy, kept = gr.seeds_with_noise()
    assert model.kept(noisy) == kept and len(kept) == 3
    assert model.kept(gr.UNKNOWN_UIDS) == [] and model.scores(gr.UNKNOWN_UIDS, "mean") is None
    assert len(model.expect(gr.UNKNOWN_UIDS, 10)[0]) == 0
    for G in gr.MODEL_G[3:]:
        assert len(set(gr.seeds_n(G))) == G


def test_aggregates_differ(model):
    """MEAN, MIN and MAX rank differently: pairwise different top-10 lists."""
    n = 0
    for name, s in all_sets().items():
        if name in ("clones", "mixed", "excl"):   # all-clone seeds tie under every aggregate; see the tie test
            continue
        L = {a: list(model.expect(s, 10, a)[0]) for a in gr.AGGS}
        assert L["mean"] != L["min"] and L["mean"] != L["max"] and L["min"] != L["max"], name
        n += 1
    assert n >= 7


def test_ties_at_the_cut_among_clones(model):
    """Seeds that are clones: every other clone scores the same, so ranks k and k + 1 tie at k = 10 and
    64 and uid order decides; the tied run crosses idx 512 and more than one 64-candidate tile."""
    s = gr.uids(gr.SEEDS_CLONES)
    for agg in gr.AGGS:
        ids, sc = model.expect(s, 130, agg)
        pos = [IDX[int(u)] for u in ids]
        assert all(ec.is_clone(p) for p in pos) and pos == sorted(pos)
        assert len(set(gr.bits(sc))) == 1
        assert pos[9] < 512 < pos[63]   # the top-64 itself crosses idx 512; ranks 10 | 11 and 64 | 65 tie
        assert pos[-1] - pos[0] > 2 * 64
    ids, _ = model.expect(s, 64, "mean")
    assert not set(int(u) for u in ids) & set(s)


def test_exclude_adj_and_exclude_change_lists(model):
    changed = 0
    for name, s in all_sets().items():
        a = model.expect(s, 10, "mean")
        b = model.expect(s, 10, "mean", exclude_adj=True)
        changed += list(a[0]) != list(b[0])
        x = model.expect(s, 10, "mean", exclude=[int(a[0][0]), gr.UNKNOWN_UIDS[0]])
        assert int(a[0][0]) not in x[0] and list(x[0][:9]) == list(a[0][1:])
    assert changed >= 1
    # the clone seed whose adjacency row names most clones: only the kept clones remain on top
    s = gr.uids(gr.SEEDS_EXCL)
    ids, _ = model.expect(s, 64, "max", exclude_adj=True)
    named = set(model.adj[ec.uid_of(ec.EXCL_CLONES_Q)]) | set(model.adj[ec.uid_of(ec.EXCL_RUN_Q)])
    assert not named & set(int(u) for u in ids)


def test_filter_keeps_enough_candidates(model):
    mask = gr.np_pass(model.c, pf, pf.CandFilter.make(**gr.FILTER_KW))
    for name, s in all_sets().items():
        for ea in (False, True):
            assert int(model.candidates(s, exclude_adj=ea, mask=mask).sum()) >= 64, name


def test_struct_sizes_match_the_header():
    """GroupQuery / GroupPlan against the C structs of include/pokec_fas.h (LP64 layout)."""
    with open(os.path.join(tl.ROOT, "include", "pokec_fas.h")) as f:
        h = f.read()
    m = re.search(r"typedef struct pf_group_query \{(.*?)\} pf_group_query;", h, re.S)
    assert m and [x for x in re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1)))] == \
        [n for n, _ in pf.GroupQuery._fields_]
    assert ctypes.sizeof(pf.GroupQuery) == 40 and pf.GroupQuery.exclude_uid.offset == 24
    m = re.search(r"typedef struct pf_group_plan \{(.*?)\} pf_group_plan;", h, re.S)
    assert m and ctypes.sizeof(pf.GroupPlan) == 24 and pf.GroupPlan.stream_bytes.offset == 16
    for name in ("PF_GROUP_MEAN", "PF_GROUP_MIN", "PF_GROUP_MAX", "PF_GROUP_EXCLUDE_ADJ", "PF_GROUP_MAX_SEEDS",
                 "PF_GROUP_MAX_EXCLUDE"):
        v = re.search(r"#define %s\s+(\d+)" % name, h)
        assert v and int(v.group(1)) == getattr(pf, name), name
    assert re.search(r"#define PF_ABI_VERSION\s+2\b", h)


def test_group_line():
    """app.group_line: the CLI's GROUP line of a POST /api/group body, and the bodies it refuses."""
    import sys
    sys.path.insert(0, os.path.join(tl.ROOT, "recommendation-system-pokec_amd"))
    import app as appmod
    assert appmod.group_line({"seeds": [3, 1, 2]}) == "GROUP 20 mean 3 1 2"
    assert appmod.group_line({"seeds": [7], "topk": 5, "agg": "min", "exclude": [9, 8], "exclude_adj": True}) == \
        "GROUP 5 min 7 noadj exclude=9,8"
    assert appmod.group_line({"seeds": (4, 5), "agg": "max", "exclude": [], "exclude_adj": False}) == "GROUP 20 max 4 5"
    for bad in ([1], {}, {"seeds": []}, {"seeds": [1, "2"]}, {"seeds": [True]}, {"seeds": [-1]}, {"seeds": [1], "agg": "median"},
                {"seeds": [1], "topk": "5"}, {"seeds": [1], "topk": -1}, {"seeds": [1], "exclude": [1.5]},
                {"seeds": [1], "exclude_adj": 1}, {"seeds": [1], "weights": [1]}):
        with pytest.raises(ValueError):
            appmod.group_line(bad)
