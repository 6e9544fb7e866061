"""The candidate filter of the all-candidates scans (pf_set_scan_filter; csrc/pf_filter.h) against
the oracle's whole ranking cut in numpy (tests/gpu_scan_filter_check.py, one fresh process per
PF_DEBUG setting and path).  Corpora: the edge corpus E, its first 2 / 511 / 512 / 513 / 1025 users
and, on the one-query paths, a seeded 20,000-user corpus with both shards of set_shard(r, 2) merged.
Filters on E: each field, KEEP_MISSING, ages past the sigmoid tables, fewer passing users than k, a
value one user has and a value nobody has, the 601 byte-identical users (a top-k of ties), a filter
that passes everybody (the unfiltered bits) and filters against the query's own exclusion row.
Paths: the default one-query launch, k5_wgs=1 / 7 with 64-candidate blocks (theta warms), k5_prune=0
(the drop mechanics without the bound), blocks that end early switched off, a batch of 8 queries
(the batch instantiation), K1, topk = 100 (the job pipeline) and six scan_keys_async calls with a
different filter before each and no synchronisation between them.  The one-query paths also check
scan_filter_count, the cleared filter, FoF interest / collab / clubs unchanged under a filter, the
malformed filters on a live context, and that the pruning counters still see every candidate.  The C++
facade's filtered overload runs through a driver of its own (tests/cpp/facade_filter_check.cpp)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(debug, mode):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_scan_filter_check.py"), mode], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("stats ")]


@pytest.mark.parametrize("shape", ["", "k5_wgs=1,k5_block=64", "k5_wgs=7,k5_block=64", "k5_prune=0", "k5_filter_blockout=0",
                                   "scan=stream"])
def test_one_query_scans_obey_the_filter(shape):
    pre = shape + "," if shape else ""
    st = run(pre + "k5_prune_stats=1", "one")[0]
    print("pruning counters under filters", shape or "(default shape)", st)
    if "k5_prune=0" in shape or "scan=stream" in shape:  # nothing is counted without the bound / on K1
        assert st["seen"] == 0, st
    else:  # a filtered-out candidate is seen, and dead in neither counter
        assert st["seen"] == st["scans"] * st["n_users"], st
        assert st["dead_block_start"] + st["dead_round_end"] < st["seen"], st


@pytest.mark.parametrize("mode", ["batch", "topk100", "async"])
def test_other_paths_obey_the_filter(mode):
    run("", mode)


def test_cpp_facade_filtered_overload(tmp_path):
    """include/pokec/recommender.h: recommend_interest_all(user, topk, CandidateFilter) equals the
    oracle's whole ranking cut in numpy, and the two-argument overload called after it is unfiltered
    again (the facade restores the filter in force before the call)."""
    import numpy as np

    import edge_corpus as ec
    import gpu_scan_filter_check as chk
    import pokec_testlib as tl
    exe = str(tmp_path / "facade_filter_check")
    pkg = os.path.join(tl.ROOT, "recommendation-system-pokec_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(tl.ROOT, "include"),
                    os.path.join(HERE, "cpp", "facade_filter_check.cpp"), "-L" + pkg, "-lpokec_fas",
                    "-Wl,-rpath," + pkg, "-o", exe], check=True)
    d = str(tmp_path / "E")
    os.makedirs(d)
    ec.write_reference_files(d)
    c = tl.read_reference_dir(d)
    F = chk.pf.CandFilter.make
    # (facade arguments: gender public age_min age_max completion_min completion_max r0 r1 r2 keep, the filter)
    cases = [("1 -1 20 29 1 0 2 -1 -1 0", F(gender=1, age=(20, 29), region=(2,))),
             ("1 -1 1 0 1 0 -1 -1 -1 1", F(gender=1, keep_missing=True)),
             ("-1 -1 1 0 80 2147483647 -1 -1 -1 0", F(completion=(80, None))),
             ("-1 -1 1 0 1 0 3 9 27 0", F(region=(3, 9, 27))),
             ("5 -1 1 0 1 0 -1 -1 -1 0", F(gender=5))]
    users = [ec.uid_of(i) for i in (1, ec.EXCL_CLONES_Q, 515, 1020)]
    q, want = [], []
    ref = chk.Ref(c, tl.Oracle(c))
    for args, f in cases:
        mask = chk.np_pass(c, f)
        for u in users:
            for k in (10, 100):  # 100: the job pipeline's all-candidates jobs
                q.append(f"filt {u} {k} {args}")
                want.append(ref.expect(u, mask, k))
        q.append(f"all {users[0]} 10")
        want.append(ref.expect(users[0], np.ones(c.n_users, bool), 10))
    r = subprocess.run([exe, d], input="\n".join(q) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(q)
    for line, ask, (ids, sc) in zip(out, q, want):
        p = line.split()
        assert int(p[3]) == len(ids), ask
        assert [int(x.split(":")[0]) for x in p[4:]] == [int(x) for x in ids], ask
        assert [int(x.split(":")[1], 16) for x in p[4:]] == [int(x) for x in np.asarray(sc, np.float32).view(np.uint32)], ask
