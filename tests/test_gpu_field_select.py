"""The field selection of the all-candidates scans (pf_set_scan_select, pf_fas_pairs_select;
csrc/pf_select.h) against the oracle on the derived corpus of tests/field_select_ref.py (only the
selected columns, every deselected fixed field blanked), bit for bit (tests/gpu_field_select_check.py,
one fresh process per PF_DEBUG setting and path).  Corpora: the edge corpus E, its first 2 / 511 /
512 / 513 / 1025 users, and E plus one user whose K1 / K1' table is probed in global memory.
Selections on E: each fixed field off alone, all seven off, the long column (where K5's rounds
split) alone and left out, the hit-list column and half of the hit-spread columns left out (hits
on deselected columns between hits on selected ones in the K1 / K1' hit lists), a column of each
normaliser mode alone, a prefix of five columns, everything selected (the unselected bits), nothing
selected (every score 0.0, ascending uid), the dense columns left out (the 601 clones: a top-k of
ties), a selection with a filter and against the query's own exclusion row.  Paths: the default
one-query launch, k5_wgs=1 / 7 with 64-candidate blocks (theta warms; pruning under the shrunk
denominator), k5_prune=0, K1, a batch of 8 queries, topk = 100 (the job pipeline), six
scan_keys_async calls with a different selection before each and no synchronisation between them,
both shards merged, the pair call, and the recommenders that never see the selection."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(debug, mode):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_field_select_check.py"), mode], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("stats ")]


@pytest.mark.parametrize("shape", ["", "k5_wgs=1,k5_block=64", "k5_wgs=7,k5_block=64", "k5_prune=0", "scan=stream"])
def test_one_query_scans_obey_the_selection(shape):
    run(shape, "one")


@pytest.mark.parametrize("shape", ["k5_wgs=1,k5_block=64", "k5_wgs=7,k5_block=64"])
def test_pruning_counters_see_every_candidate(shape):
    st = run(shape + ",k5_prune_stats=1", "stats")[0]
    print("pruning counters under selections", shape, st)
    assert st["seen"] == st["scans"] * st["n_users"], st
    assert st["dead_block_start"] + st["dead_round_end"] < st["seen"], st


@pytest.mark.parametrize("mode", ["batch", "topk100", "async", "pairs"])
def test_other_paths_obey_the_selection(mode):
    run("", mode)


@pytest.mark.parametrize("shape", ["", "scan=stream"])
def test_global_table_image(shape):
    run(shape, "gtab")


def test_cpp_facade_selected_overloads(tmp_path):
    """include/pokec/recommender.h: recommend_interest_all(user, topk, FieldSelect[, CandidateFilter])
    and profile_similarity(A, B, FieldSelect) equal the derived oracle; profile_similarity(A, B,
    prefix of the engine's columns) goes through the selection on the one engine (the registry still
    holds one) and equals the oracle's bits for that list; the two-argument recommend_interest_all
    called after a selected one is unselected again."""
    import numpy as np

    import edge_corpus as ec
    import field_select_ref as fsr
    import gpu_scan_filter_check as fchk
    import pokec_testlib as tl
    pf = tl.product()
    exe = str(tmp_path / "facade_select_check")
    pkg = os.path.join(tl.ROOT, "recommendation-system-pokec_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(tl.ROOT, "include"),
                    os.path.join(HERE, "cpp", "facade_select_check.cpp"), "-L" + pkg, "-lpokec_fas",
                    "-Wl,-rpath," + pkg, "-o", exe], check=True)
    d = str(tmp_path / "E")
    os.makedirs(d)
    ec.write_reference_files(d)
    c = tl.read_reference_dir(d)
    S = pf.FieldSelect.make
    sels = [S(fixed=0x7F & ~2), S(fixed=0, cols=[ec.COL_L]), S(cols=[t for t in range(ec.N_COLS) if t not in ec.COLS_HS[::2]]),
            S(fixed=0, cols=0)]
    filt = pf.CandFilter.make(gender=1, age=(20, 29), region=(2,))
    fargs = "1 -1 20 29 1 0 2 -1 -1 0"
    users = [ec.uid_of(i) for i in (1, ec.HIT_Q_SPREAD, ec.EXCL_CLONES_Q, 515)]
    pairs = ec.planted_pairs()[:60] + [(a, b) for a, b, _ in ec.HIT_PAIRS]
    q, want = [], []
    base = fchk.Ref(c, tl.Oracle(c))
    for s in sels:
        ref = fsr.SelRef(c, s)
        for u in users:
            for k in (10, 100):  # 100: the job pipeline's all-candidates jobs
                q.append(f"sel {u} {k} {s.fixed:x} {s.cols:x}")
                want.append(ref.expect(u, k))
            q.append(f"selfilt {u} 10 {s.fixed:x} {s.cols:x} {fargs}")
            want.append(ref.expect(u, 10, fchk.np_pass(c, filt)))
        q.append(f"all {users[0]} 10")  # unselected again
        want.append(base.expect(users[0], np.ones(c.n_users, bool), 10))
        a = np.array([ec.uid_of(x) for x, _ in pairs], np.int32)
        b = np.array([ec.uid_of(y) for _, y in pairs], np.int32)
        for x, y, w in zip(a, b, ref.fas_pairs(a, b)):
            q.append(f"simsel {x} {y} {s.fixed:x} {s.cols:x}")
            want.append(w)
    # profile_similarity(A, B, text_columns) with a proper prefix of the engine's list: the reference's
    # own bits for that list (the derived corpus of the prefix, every fixed field kept)
    for n in (1, 5, ec.COL_HC + 1):
        ref = fsr.SelRef(c, S(cols=range(n)))
        a = np.array([ec.uid_of(x) for x, _ in pairs], np.int32)
        b = np.array([ec.uid_of(y) for _, y in pairs], np.int32)
        for x, y, w in zip(a, b, ref.fas_pairs(a, b)):
            q.append(f"simprefix {x} {y} {n}")
            want.append(w)
    q.append("engines")
    want.append(1)
    r = subprocess.run([exe, d], input="\n".join(q) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(q)
    for line, ask, w in zip(out, q, want):
        p = line.split()
        if ask == "engines":
            assert int(p[1]) == w, line
        elif ask.startswith("sim"):
            assert int(p[1], 16) == int(np.float32(w).view(np.uint32)), (ask, line)
        else:
            ids, sc = w
            assert int(p[3]) == len(ids), ask
            assert [int(x.split(":")[0]) for x in p[4:]] == [int(x) for x in ids], ask
            assert [int(x.split(":")[1], 16) for x in p[4:]] == [int(x) for x in np.asarray(sc, np.float32).view(np.uint32)], ask
