"""Device checks of the query-image builder K6 (qimage_kernel, pf_jobs.hip).

test_qimage_vs_host_references runs tools/probe/qimage (built by __graft_entry__.build() through
tools/Makefile; it links the product's own build/pf_jobs_k.o, pf_store.o and pf_idf_k.o): every image K6
builds for one packed and one wide corpus of planted users, checked exactly against the host builder's
QConst, a plain loop's token values and the rows' distinct clubs / friends / tokens as a multiset at their
cuckoo slots, with *fail, the pool's filler between the images and the bisection launch.  The probe's
summary lines are asserted, so a sweep that lost one of its planted categories fails here.

test_planted_users_through_public_calls puts users of the same class-boundary sizes, the retry user and
the ids only the wide format takes through pf_open's resident images and the public calls, against the
oracle bit for bit.  The call that scores through K1' on K6's images is the all-candidates recommender
with topk above the scan kernels' bound (the job pipeline's kDjAll job: every candidate against the
query's resident image); fas_pairs and fas_profile_pairs build their images on the host, and the scan
with topk <= 64 probes no K6 table, so the three paths check one another."""
import os
import re
import subprocess

import numpy as np
import pytest

import pokec_testlib as tl
import query_profile_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "probe", "qimage")
T = 3
WIDE_IDS = [  # (clubs, friends) only the wide format takes
    ([0x80000000], [0]),
    ([0xC0000005], [0x40000005]),
    ([0xFFFFFFFF], []),
    ([0xFFFFFFFF] * 3, []),
    ([], [0xFFFFFFFF]),
    ([0x7FFFFFFF], [0x7FFFFFFF]),
]


def _line(out, part):
    m = re.search(r"^%s ((?:\w+ [\d.]+ ?)+)$" % part, out, re.M)
    assert m, out
    w = m.group(1).split()
    return {w[i]: float(w[i + 1]) for i in range(0, len(w), 2)}


@pytest.mark.gpu
def test_qimage_vs_host_references():
    assert os.path.exists(PROBE), "tools/probe/qimage not built (run __graft_entry__.build())"
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.endswith("\nOK\n"), r.stdout + r.stderr
    for part in ("P", "W"):
        c = _line(r.stdout, part)
        assert min(c["small"], c["big"], c["tokens"], c["entries"], c["dup_words"]) > 0, r.stdout
        assert c["global"] >= 2 and c["scr_nonzero"] >= 1, r.stdout  # the second global build's scratch offset
        assert c["edges"] == 4 and c["retries"] >= 1, r.stdout       # small|big and big|global, by tokens and by friends
        assert c["bisect"] == c["images"] == c["small"] + c["big"] + c["global"], r.stdout
    assert _line(r.stdout, "P")["wrap"] >= 10 and _line(r.stdout, "W")["wide_ids"] == len(WIDE_IDS), r.stdout


def test_qimage_probe_source_present():
    assert os.path.exists(PROBE + ".hip")


# ------------------------------------------------------------------ the same users through the public calls
def _edges():
    """{format: {kind: sizes}} the last size of the lower class at each boundary, from the planner's own rule."""
    out = subprocess.run([PROBE, "--edges"], capture_output=True, text=True, timeout=120, check=True).stdout
    e = {}
    for fmt, tok, fr in re.findall(r"^edges (\w) tokens ([\d ]+) friends ([\d ]+)$", out, re.M):
        e[fmt] = {"tokens": [int(x) for x in tok.split()], "friends": [int(x) for x in fr.split()]}
    assert set(e) == {"P", "W"} and all(len(v) == 2 for f in e.values() for v in f.values()), out
    return e


def _retry_ids(tag):
    """Three club ids whose cuckoo slots at lg 4 under the first multiplier are one {h1, h2} pair."""
    ids = np.arange(1, 1 << 16, dtype=np.uint64)
    x = ((ids | tag) * 0x9E3779B1) & 0xFFFFFFFF
    h1, h2 = x >> 28, (x >> 24) & 15
    pair = np.minimum(h1, h2) * 16 + np.maximum(h1, h2)
    for p in range(256):
        hit = ids[(pair == p) & (h1 != h2)]
        if len(hit) >= 3:
            return [int(v) for v in hit[:3]]
    raise AssertionError("no retry ids")


def _user(clubs=(), friends=(), ntok=0, i=0):
    toks = [dict() for _ in range(T)]
    for j in range(ntok):
        toks[j % T][(j // T) * 3 + j % T] = 1 + (j * 7 + 3) % 200
    return dict(pub=-1 if i % 5 == 0 else i % 2, gen=-1 if i % 3 == 0 else i % 3 - 1, comp=(0, 1, 128, 129, 32767)[i % 5],
                age=(129, 0, 18, 32767, 1)[i % 5], reg=[(3 + i) % 5 if k < i % 4 else -1 for k in range(3)],
                clubs=list(clubs), friends=list(friends), toks=toks)


def planted_corpus(packed, edges):
    """(corpus, planted uids, wide-id uids): users on both sides of every class boundary by tokens and by
    friends, the retry user, in the wide corpus the ids only it takes, and partners that hold the planted
    ids, tokens and friends.  No adjacency, so an all-candidates call ranks everyone but the query."""
    e = edges["P" if packed else "W"]
    us = []
    for n in e["tokens"]:
        us += [_user(ntok=n, i=len(us)), _user(ntok=n + 1, i=len(us) + 1)]
    for n in e["friends"]:
        us += [_user(friends=range(1000, 1000 + 3 * n, 3), i=len(us)), _user(friends=range(1000, 1003 + 3 * n, 3), i=len(us) + 1)]
    us.append(_user(clubs=_retry_ids(0x80000000 if packed else 0), i=len(us)))
    n_planted = len(us)
    wide = []
    if not packed:
        for cl, fr in WIDE_IDS:
            wide.append(len(us))
            us.append(_user(clubs=cl, friends=fr, ntok=2, i=len(us)))
        n_planted = len(us)
        # partners: the planted ids in the same and in the other kind, and the ids their old keys collided with
        us.append(_user(clubs=[0x80000000, 0xFFFFFFFF, 0xC0000005, 0x7FFFFFFF], friends=[0, 0x40000005, 0xFFFFFFFF, 0x7FFFFFFF], i=1))
        us.append(_user(clubs=[0, 0x40000005, 0xFFFFFFFE], friends=[0x80000000, 0xC0000005, 0xFFFFFFFE], i=2))
        us.append(_user(friends=[0], i=3))
        us.append(_user(clubs=[0xFFFFFFFF], friends=[0x7FFFFFFF], ntok=300, i=6))
    else:
        us.append(_user(clubs=[0, (1 << 30) - 1], friends=[(1 << 30) - 1, 0], ntok=7, i=1))
    us.append(_user(clubs=_retry_ids(0x80000000 if packed else 0)[:2], friends=range(1000, 1600, 3), ntok=40, i=2))
    us.append(_user(friends=range(1003, 4000, 6), ntok=500, i=7))
    us.append(_user(ntok=0, i=4))
    if not packed:
        us[-3]["toks"][0][0] = 300  # the corpus is wide by a tf and by its ids
    n = len(us)
    assert n <= 64, n  # the scan's top-64 then holds every candidate
    coff, foff, toff, clubs, friends, tid, tf = [0], [0], [0], [], [], [], []
    for u in us:
        clubs += u["clubs"]
        friends += u["friends"]
        coff.append(len(clubs))
        foff.append(len(friends))
        for t in range(T):
            tid += list(u["toks"][t].keys())
            tf += list(u["toks"][t].values())
            toff.append(len(tid))
    uid = np.arange(1, n + 1) * 2 + 5
    c = tl.Corpus(uid, [u["pub"] for u in us], [u["comp"] for u in us], [u["gen"] for u in us], [u["age"] for u in us],
                  [r for u in us for r in u["reg"]], coff, clubs if clubs else [0], foff, friends if friends else [0], toff, tid, tf,
                  [], [0], [0], T)
    return c, [int(v) for v in uid[:n_planted]], [int(uid[i]) for i in wide]


def test_oracle_keeps_high_ids_distinct():
    """The oracle the device tests lean on scores club / friend ids of 2^31 and above as themselves: a shared
    high id counts, and ids that differ only in bit 31, or by the wrap of id + 1, do not."""
    us = [_user(clubs=[0x80000000], friends=[0xFFFFFFFF]), _user(clubs=[0x80000000], friends=[0xFFFFFFFF]),
          _user(clubs=[0], friends=[0x7FFFFFFF]), _user(clubs=[5], friends=[6]), _user(clubs=[0xFFFFFFFF], friends=[0x80000000])]
    coff = np.arange(len(us) + 1)
    c = tl.Corpus(np.arange(1, len(us) + 1), [1] * 5, [10] * 5, [1] * 5, [20] * 5, [-1] * 15, coff, [u["clubs"][0] for u in us], coff,
                  [u["friends"][0] for u in us], np.zeros(5 * T + 1), [0], [0], [], [0], [0], T)
    s = tl.Oracle(c).fas_pairs([1, 1, 1, 1], [2, 3, 4, 5])
    assert s[0] > s[1] and s[1] == s[2] == s[3], s


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "wide"])
def test_planted_users_through_public_calls(packed):
    pf = tl.product()
    c, planted, wide = planted_corpus(packed, _edges())
    eng, orc = tl.engine(c), tl.Oracle(c)
    try:
        lay = eng.layout()
        assert lay.packed_tokens == (1 if packed else 0)
        assert lay.resident_images == 1, "the resident images were not built at open, or were dropped"
        uids = [int(u) for u in c.uid]
        bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
        want = {a: orc.fas_pairs(np.full(len(uids), a, np.int32), uids) for a in planted}
        # K1' on K6's resident images: every candidate but the query itself, from the job pipeline
        got = eng.recommend_interest(planted, 128, tl.PF_MODE_ALL)
        for a, (ids, sc) in zip(planted, got):
            assert sorted(int(x) for x in ids) == [u for u in uids if u != a], a
            pos = {u: k for k, u in enumerate(uids)}
            ref = want[a][[pos[int(x)] for x in ids]]
            bad = np.nonzero(bits(sc) != bits(ref))[0]
            assert len(bad) == 0, (a, [(int(ids[k]), float(sc[k]), float(ref[k])) for k in bad[:6]])
        # the host-built images of the same users
        for a in planted:
            assert np.array_equal(bits(eng.fas_pairs(np.full(len(uids), a, np.int32), uids)), bits(want[a])), a
        for a in wide:
            i = uids.index(a)
            prof = qc.profile_of_record(pf, qc.record_of_user(c, i))
            assert np.array_equal(bits(eng.fas_profile_pairs(prof, uids)), bits(want[a])), a
            ids, sc = eng.recommend_interest_all([a], 64)[0]  # the scan: no K6 table
            assert sorted(int(x) for x in ids) == [u for u in uids if u != a], a
            assert np.array_equal(bits(sc), bits(want[a][[uids.index(int(x)) for x in ids]])), a
    finally:
        eng.close()
