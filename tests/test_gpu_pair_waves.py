"""The pair kernel K1' (fas_pairs_kernel, csrc/pf_kernels.hip) on planted waves: the wave-level paths
of its packed epilogue (pair_epilogue: the item queue's rounds, the per-lane fallback, the wave's
re-walk of overflowed hit lists), which depend on what the 64 lanes of a wave hold together.

tests/pair_wave_corpus.py plants the corpus and the compositions (lists of candidate classes by lane)
and says why the public call fixes a wave's composition; tests/test_pair_wave_cpu.py guards what every
class and composition claims.  Here every composition is issued as one group of fas_pairs(Q.., b..)
and every score compared bit for bit with the oracle (tl.Oracle(c).fas_pairs, the CPU restatement); a
failure names composition, lane, class, got and want.  The same compositions go
  - under a field selection that changes their kind (against the derived oracle of
    tests/field_select_ref.py, as the existing selection tests do),
  - through fas_profile_pairs (the same kernel on an uploaded by-value image),
  - against QG, whose table is probed in global memory (the GTAB instantiation),
  - onto the wide twin of the corpus (fas_slot<false>, text_terms_slow),
  - and through the job pipeline's K1' route (recommend_interest(.., 128, PF_MODE_ALL): order != nullptr,
    the resident K6 images, one launch per image class).

What confirms the global-table class: for the pair call nothing the engine exposes does (its launch is
GTAB when an image's keys + values exceed the 48 KiB staging limit; tests/test_pair_wave_cpu.py
restates that rule for QG, and QG's token count is asserted above the big | global boundary of
tools/probe/qimage --edges here).  For the job route pf_jobs_stats.pair_dispatches does: the batch
with QG takes one K1' launch more than the batch without it.

What fixes the job route's waves: the all-candidates job lists every profile in idx order with the
query's own entry left in place as an inactive lane, and K9 cuts the list into blocks of 512
(csrc/pf_jobs.hip gather_kernel kDjAll, expand_pairs_kernel).  That was confirmed by reading only.
The 127 users of I(12) and of I(21) have consecutive uids, so at least one whole wave is each class
in idx order; they have one record length each, so the same holds in the store's slot order
(csrc/pf_store.cpp:306-318, recomputed by the CPU guard), which orders the other jobs' candidates.

The summary the last test prints counts the compositions by what the host model says of their waves."""
import os
import re
import subprocess

import numpy as np
import pytest

import field_select_ref as fsr
import pair_wave_corpus as pw
import pokec_testlib as tl
import query_profile_cases as qc

pytestmark = pytest.mark.gpu
PROBE = os.path.join(tl.ROOT, "tools", "probe", "qimage")
CATEGORIES = ("one_round", "two_rounds", "per_lane", "with_overflow", "partial_wave", "selected", "by_value",
              "global_class", "wide", "job_route")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Run:
    """Everything runs once (two engines, a few dozen small launches); the tests read the outcome."""

    def __init__(self):
        self.fail = {}     # suite -> [message]
        self.count = {k: 0 for k in CATEGORIES}
        self.ran = {}      # suite -> compositions checked
        self.notes = {}

    def tally(self, cats, *extra):
        kinds = {c[0] for c in cats}
        for k in ("one_round", "two_rounds", "per_lane"):
            self.count[k] += k in kinds
        self.count["with_overflow"] += any(c[3] for c in cats)
        self.count["partial_wave"] += any(c[4] for c in cats)
        for k in extra:
            self.count[k] += 1

    def check(self, suite, name, pairs, classes, got, want):
        self.ran[suite] = self.ran.get(suite, 0) + 1
        bad = np.nonzero(bits(got) != bits(want))[0]
        for j in bad[:8]:
            self.fail.setdefault(suite, []).append(
                "%s: pair %d (lane %d of its group's block %d) class %s b=%d got %r (%08x) want %r (%08x)"
                % (name, j, classes[j][1] % pw.PAIR_THREADS, classes[j][1] // pw.PAIR_THREADS, classes[j][0], pairs[j][1],
                   float(got[j]), int(bits(got)[j]), float(want[j]), int(bits(want)[j])))
        if len(bad) > 8:
            self.fail[suite].append("%s: %d more" % (name, len(bad) - 8))


def _arrays(pairs):
    return np.array([a for a, _ in pairs], np.int32), np.array([b for _, b in pairs], np.int32)


def _in_group(pairs):
    """(class name, position within its query's group) per pair."""
    inv = {pw.uid_of(n, k): n for n, (cnt, _) in pw.CLASSES.items() for k in range(cnt)}
    at, out = {}, []
    for a, b in pairs:
        out.append((inv[b], at.get(a, 0)))
        at[a] = at.get(a, 0) + 1
    return out


def _run_all():
    R = Run()
    pf = tl.product()
    c, _ = pw.corpus()
    eng, orc = tl.engine(c), tl.Oracle(c)
    try:
        lay = eng.layout()
        assert lay.packed_tokens == 1 and lay.resident_images == 1, (lay.packed_tokens, lay.resident_images)
        # ---- every composition as one group of the pair call
        for name, (q, lanes, _) in pw.COMPOSITIONS.items():
            pairs = pw.lanes_uids(lanes, q)
            a, b = _arrays(pairs)
            R.check("waves", name, pairs, _in_group(pairs), eng.fas_pairs(a, b), orc.fas_pairs(a, b))
            R.tally(pw.categories(c, pairs))
        pairs = pw.interleaved()
        a, b = _arrays(pairs)
        R.check("waves", "interleaved", pairs, _in_group(pairs), eng.fas_pairs(a, b), orc.fas_pairs(a, b))
        R.tally(pw.categories(c, pairs))
        # ---- under a field selection
        for name, (comp, fixed, cols, _, _) in pw.SELECTED.items():
            q, lanes, _ = pw.COMPOSITIONS[comp]
            pairs = pw.lanes_uids(lanes, q)
            a, b = _arrays(pairs)
            sel = pf.FieldSelect.make(fixed=fixed, cols=cols)
            R.check("selected", name, pairs, _in_group(pairs), eng.fas_pairs(a, b, select=sel), fsr.SelRef(c, sel).fas_pairs(a, b))
            R.tally(pw.categories(c, pairs, fixed, cols), "selected")
        # ---- the by-value image of Q
        prof = qc.profile_of_record(pf, qc.record_of_user(c, pw.uid_of("Q") - pw.UID0))
        for comp in (pw.HEAVY_TWO, pw.HEAVY_FALLBACK):
            pairs = pw.lanes_uids(pw.COMPOSITIONS[comp][1], "Q")
            a, b = _arrays(pairs)
            R.check("by_value", comp, pairs, _in_group(pairs), eng.fas_profile_pairs(prof, b), orc.fas_pairs(a, b))
            R.tally(pw.categories(c, pairs), "by_value")
        # ---- the global-table instantiation
        for comp in (pw.HEAVY_TWO, pw.HEAVY_FALLBACK, "ov_all64"):
            pairs = pw.lanes_uids(pw.COMPOSITIONS[comp][1], "QG")
            a, b = _arrays(pairs)
            R.check("global_class", comp, pairs, _in_group(pairs), eng.fas_pairs(a, b), orc.fas_pairs(a, b))
            R.tally(pw.categories(c, pairs), "global_class")
        # ---- the job pipeline's K1' route
        qs = [pw.uid_of("Q"), pw.uid_of("Q1"), pw.uid_of("QG")]
        uids = [int(u) for u in c.uid]
        pos = {u: k for k, u in enumerate(uids)}
        d0 = eng.jobs_stats()["pair_dispatches"]
        eng.recommend_interest(qs[:2], 128, tl.PF_MODE_ALL)
        d1 = eng.jobs_stats()["pair_dispatches"]
        top = eng.recommend_interest(qs, 128, tl.PF_MODE_ALL)
        d2 = eng.jobs_stats()["pair_dispatches"]
        R.notes["dispatches"] = (d1 - d0, d2 - d1)
        everyone = eng.recommend_interest(qs, len(uids), tl.PF_MODE_ALL)
        ref_top = orc.interest(qs, 128, tl.PF_MODE_ALL)
        for q, (ids, sc), (aids, asc), (rids, rsc) in zip(qs, top, everyone, ref_top):
            want = orc.fas_pairs(np.full(len(uids), q, np.int32), uids)
            name = "job_route q=%d" % q
            if [int(x) for x in ids] != [int(x) for x in rids] or not np.array_equal(bits(sc), bits(rsc)):
                R.fail.setdefault("job_route", []).append("%s: the top 128 differ from the oracle's" % name)
            if sorted(int(x) for x in aids) != [u for u in uids if u != q]:
                R.fail.setdefault("job_route", []).append("%s: not every candidate but the query was returned" % name)
                continue
            pairs = [(q, int(x)) for x in aids]
            classes = [(n, pos[b]) for (n, _), (_, b) in zip(_in_group(pairs), pairs)]   # lane = idx % 512
            R.check("job_route", name, pairs, classes, asc, want[[pos[int(x)] for x in aids]])
            R.tally(pw.categories(c, pw.job_route_pairs(c, q)), "job_route")
    finally:
        eng.close()
        orc.close()
    # ---- the wide twin
    w, _ = pw.corpus(wide=True)
    eng, orc = tl.engine(w), tl.Oracle(w)
    try:
        assert eng.layout().packed_tokens == 0
        for comp in pw.OVERFLOW_COMPOSITIONS + [pw.HEAVY_FALLBACK, pw.HEAVY_TWO]:
            q, lanes, _ = pw.COMPOSITIONS[comp]
            pairs = pw.lanes_uids(lanes, q)
            a, b = _arrays(pairs)
            R.check("wide", comp, pairs, _in_group(pairs), eng.fas_pairs(a, b), orc.fas_pairs(a, b))
            R.count["wide"] += 1
    finally:
        eng.close()
        orc.close()
    return R


@pytest.fixture(scope="module")
def R():
    return _run_all()


def _clean(R, suite, at_least):
    assert not R.fail.get(suite), "\n".join(R.fail[suite])
    assert R.ran.get(suite, 0) >= at_least, (suite, R.ran.get(suite, 0))


def test_planted_waves_bit_exact(R):
    """Every composition of pair_wave_corpus.COMPOSITIONS and the two interleaved groups."""
    _clean(R, "waves", len(pw.COMPOSITIONS) + 1)


def test_selected_waves_bit_exact(R):
    _clean(R, "selected", 2)


def test_by_value_image_bit_exact(R):
    _clean(R, "by_value", 2)


def test_global_table_image_bit_exact(R):
    assert os.path.exists(PROBE), "tools/probe/qimage not built (run __graft_entry__.build())"
    out = subprocess.run([PROBE, "--edges"], capture_output=True, text=True, timeout=120, check=True).stdout
    edges = {f: [int(x) for x in tok.split()] for f, tok in re.findall(r"^edges (\w) tokens ([\d ]+) friends", out, re.M)}
    assert set(edges) == {"P", "W"} and all(len(v) == 2 for v in edges.values()), out
    assert pw.GLOBAL_FILL > max(edges["P"][1], edges["W"][1]), (pw.GLOBAL_FILL, edges)   # past big | global
    _clean(R, "global_class", 3)


def test_wide_twin_bit_exact(R):
    _clean(R, "wide", len(pw.OVERFLOW_COMPOSITIONS) + 2)


def test_job_route_bit_exact(R):
    _clean(R, "job_route", 3)
    without, with_qg = R.notes["dispatches"]
    assert with_qg == without + 1, (without, with_qg)   # QG's global-table class is a K1' launch of its own


def test_every_category_was_reached(R):
    print("pair waves: " + " ".join("%s %d" % (k, R.count[k]) for k in CATEGORIES))
    assert all(R.count[k] > 0 for k in CATEGORIES), R.count
