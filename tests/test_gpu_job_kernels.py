"""Device checks of the job pipeline's kernels (pf_jobs.hip) on synthetic plans, each against a serial
host loop inside tools/probe/jobs.hip (built by __graft_entry__.build() through tools/Makefile; it links
the product's own build/pf_jobs_k.o): A K3 gather_kernel at its rounds of 2 x 1024 positions, its
friend-segment scan's trips of 1024, limits on a round's edge, duplicates, views, hash clusters and the
counting-sort path; B K9 expand_pairs_kernel, order_pairs_kernel around its 8 x 1024 kept keys and
slot_class; C K4' collab_kernel bit for bit on inputs whose float sum depends on the summation order,
with the fused top-k hand-off at 1, 2 and 16 blocks per job; D K7 clubs_kernel in its stream order,
acc left zero; E K8 topk_kernel.  The probe's summary lines are asserted, so a sweep that lost one of
its planted categories fails here.

The probe hands the kernels plans of its own; test_planner_sizes_through_api puts the same sizes
through the planner (pf_jobs_plan.cpp) and the public calls, against the oracle."""
import os
import re
import subprocess

import numpy as np
import pytest

import pokec_testlib as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "probe", "jobs")


def _line(out, part):
    """The counters of the probe's summary line of `part`: 'A jobs 607 nf_sweep 84 ...' -> dict."""
    m = re.search(r"^%s ((?:\w+ [\d.]+ ?)+)$" % part, out, re.M)
    assert m, out
    w = m.group(1).split()
    return {w[i]: float(w[i + 1]) for i in range(0, len(w), 2)}


@pytest.mark.gpu
def test_job_kernels_vs_host_references():
    assert os.path.exists(PROBE), "tools/probe/jobs not built (run __graft_entry__.build())"
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.endswith("\nOK\n"), r.stdout + r.stderr
    a = _line(r.stdout, "A")
    # every kind and planted category of K3: raw and filtered lists in both flavours behind each sweep
    assert min(a[k] for k in ("nf_sweep", "total_sweep", "dups", "rowlens", "noprofile", "interest_excl", "views", "hash", "nk",
                              "all", "clubs")) > 0, r.stdout
    assert a["nf_sweep"] >= 7 * 2 * 2 and a["total_sweep"] >= 9 * 2 * 2, r.stdout
    assert min(a["multi_round"], a["edge_limit"], a["sort_path"]) > 0, r.stdout
    assert a["clusters"] >= 2 and a["wrap"] >= 1, r.stdout
    b = _line(r.stdout, "B")
    assert min(b["expand_blocks"], b["run_edges"], b["order_below_8192"], b["order_above_8192"]) > 0, r.stdout
    assert b["slot_values"] >= 41 + 3 * 30 - 3, r.stdout  # 0..40 and 2^k - 1, 2^k, 2^k + 1, less the overlaps below 40
    c = _line(r.stdout, "C")
    assert c["jobs"] >= 8 * 7 and 2 * c["planted_jobs"] >= c["jobs"], r.stdout
    assert c["planted"] > 0 and c["order_sensitive"] >= 0.95 * c["planted"], r.stdout
    assert min(c["same_tile"], c["cross_tile"], c["live"], c["dead"], c["fused_1"], c["fused_2"], c["fused_16"], c["untouched"],
               c["k8_rows"], c["tie_pairs"]) > 0, r.stdout
    d = _line(r.stdout, "D")
    assert d["order_clubs"] >= 8 and d["order_checked"] >= 2 * d["order_clubs"], r.stdout
    assert min(d["clubs_checked"], d["multi_round_items"], d["nan_clubs"], d["acc_zero"]) > 0 and d["launches"] == 2, r.stdout
    assert d["chunk_totals"] >= 5, r.stdout
    e = _line(r.stdout, "E")
    assert e["rows"] >= 3 * 9 * 2 and min(e["club_rows"], e["short_rows"], e["tie_pairs"]) > 0, r.stdout


def test_job_kernels_probe_source_present():
    assert os.path.exists(PROBE + ".hip")


# ------------------------------------------------------------------ the same sizes through the planner
ROUND = 2048  # K3's round: 2 x 1024 positions


def planner_corpus():
    """A 4000-user synthetic corpus whose adj_list is edited so that some users' 2-hop sequences land on
    K3's sizes.  Returns (corpus, {query uid: (friends, graph sequence, collaborative sequence)}).

    One-friend users: the friend's row has `rl` entries (profiles, repeats, uids without a profile and
    the user itself), so the collaborative sequence has rl positions and the graph one rl + 1.
    Many-friend users: nf friends with one-entry rows, nf and 2 nf positions."""
    base = tl.synth.Corpus(n_users=4000, seed=13, edge_cases=1)
    c = tl.corpus_from_desc(base.desc_ptr())
    uids = [int(u) for u in c.uid]
    rng = np.random.default_rng(2048)
    adj, seqs = {}, {}
    for i, rl in enumerate((2047, 2048, 2049, 4095, 4096, 4097)):
        q, f = uids[100 + i], uids[200 + i]
        row = [int(x) for x in rng.integers(1, 6000, rl)]  # uids above the corpus's have no profile
        row[5], row[rl // 2], row[-1] = q, q, row[0]
        adj[q], adj[f] = [f], row
        seqs[q] = (1, [f] + row, list(row))
    pool = uids[1000:1000 + 1025]
    for f in pool:
        adj[f] = [int(rng.integers(1, 6000))]
    for i, nf in enumerate((1023, 1024, 1025)):
        q = uids[300 + i]
        adj[q] = pool[:nf]
        seqs[q] = (nf, [x for f in pool[:nf] for x in (f, adj[f][0])], [adj[f][0] for f in pool[:nf]])
    return tl.with_rows(c, adj=adj), seqs


def _firsts(seq, u):
    out, seen = [], set()
    for x in seq:
        if x != u and x not in seen:
            seen.add(x)
            out.append(x)
    return out


@pytest.mark.gpu
def test_planner_sizes_through_api():
    """fof_candidates in both flavours at the limits 1, total - 1, total, total + 1 and F1 - 1, F1, F1 + 1
    (F1: the first occurrences K3's first round of 2048 positions finds, read off the oracle's list), and
    recommend_collaborative at two of them, on sequences of 2047 ... 4097 positions and 1023 ... 1025
    friends, against the oracle."""
    c, seqs = planner_corpus()
    eng, orc = tl.engine(c), tl.Oracle(c)
    totals, nfs = set(), set()
    for q, (nf, sg, sc) in seqs.items():
        nfs.add(nf)
        for fl, seq in ((tl.PF_FOF_GRAPH, sg), (tl.PF_FOF_COLLAB, sc)):
            total = len(seq)
            totals.add(total)
            full = [int(x) for x in orc.fof(q, 1 << 20, fl)]
            assert full == _firsts(seq, q), (q, fl)  # the oracle walks the sequence this test built
            f1 = len(_firsts(seq[:ROUND], q))
            assert full[:f1] == _firsts(seq[:ROUND], q)
            for lim in sorted({1, total - 1, total, total + 1, f1 - 1, f1, f1 + 1}):
                if lim < 1:
                    continue
                got, ref = eng.fof_candidates(q, lim, fl), orc.fof(q, lim, fl)
                assert list(got) == list(ref), (q, fl, lim, len(got), len(ref))
    assert {2047, 2048, 2049, 4096, 4097} <= totals and {1023, 1024, 1025} <= nfs, (totals, nfs)
    # collaborative sums and top-k over those lists: the one-friend users (the oracle scores each pair on one core)
    qs = [q for q, (nf, sg, sc) in seqs.items() if nf == 1]
    f1 = len(_firsts(seqs[qs[0]][2][:ROUND], qs[0]))
    for lim in (f1, len(seqs[qs[0]][2])):
        for k in (10, 100):
            for u, g, r in zip(qs, eng.recommend_collaborative(qs, k, lim), orc.collab(qs, k, lim)):
                assert list(g[0]) == list(r[0]), (u, lim, k)
                assert np.array_equal(g[1].view(np.uint32), r[1].view(np.uint32)), (u, lim, k)
    eng.close()
