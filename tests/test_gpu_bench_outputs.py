"""bench.py --dump-outputs on the GPU, at a small corpus: the files hold the last timed step's
results (checked against the engine called directly on the same seeded corpus and queries), the
same arguments give the same files, and --full's extra launches after the timed region do not
change what is written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pokec_testlib as tl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

USERS, STEPS, WARM = 20000, 3, 1


def run_bench(out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARM),
           "--users", str(USERS), "--dump-outputs", str(out), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["steps"] == STEPS and rec["ms_per_step"] > 0
    return rec, {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


@pytest.fixture(scope="module")
def small():
    """bench.py's corpus at USERS users (seed 1) and an engine on it."""
    c = tl.synth.Corpus(n_users=USERS, seed=1, edge_cases=0, threads=16)
    eng = tl.engine(c.desc_ptr())
    yield c, eng
    eng.close()
    c.close()


def test_cfg2_dump_is_last_step_and_repeatable(small, tmp_path):
    _, eng = small
    plain, a = run_bench(tmp_path / "a")
    # the same arguments with the extras: the isolated launches reuse the output buffer after the dump
    full, b = run_bench(tmp_path / "b", "--full", "--no-cpu-baseline", "--no-pmc", "--no-cfg3")
    assert plain["roofline"] is None and plain["topk_selfcheck"] is None
    assert full["topk_selfcheck"] is True and full["roofline"]["isolated_launch"]["launches"] >= 1
    assert sorted(a) == sorted(b) == ["topk_scores", "topk_uids"]
    assert a["topk_uids"].dtype == np.float64 and a["topk_scores"].dtype == np.float32
    for name in a:
        assert a[name].shape == (1, bench.TOPK) and np.array_equal(a[name], b[name]), name
    # the last timed step's query (bench.py's cfg-2 stream, seed 2), asked of the engine directly
    q = int(np.random.default_rng(2).integers(1, USERS + 1, size=(WARM + STEPS, 1))[-1, 0])
    want = bench.topk_arrays(eng.recommend_interest_all([q], bench.TOPK), bench.TOPK)
    assert np.array_equal(a["topk_uids"], want["topk_uids"])
    assert np.array_equal(a["topk_scores"].view(np.uint32), want["topk_scores"].view(np.uint32))
    # and the dumped ids rescored by the pair kernel
    uids = a["topk_uids"][0].astype(np.int32)
    assert (uids > 0).all()
    again = eng.fas_pairs(np.full(len(uids), q, np.int32), uids)
    assert np.array_equal(np.asarray(again, np.float32).view(np.uint32), a["topk_scores"][0].view(np.uint32))


def test_cfg3_dump_is_last_step_of_its_context(small, tmp_path):
    """Two contexts, three steps: the last step (index 2) ran on context 0, after context 1's step 1."""
    _, eng = small
    _, a = run_bench(tmp_path / "c", "--workload", "cfg3", "--contexts", "2")
    mine = bench.cfg3_queries(USERS, WARM, STEPS)[-1]
    want = bench.topk_arrays(eng.recommend_collaborative(mine, bench.TOPK, bench.CFG3_LIMIT), bench.TOPK)
    assert a["topk_uids"].shape == (bench.CFG3_QUERIES, bench.TOPK)
    assert (a["topk_uids"] > 0).any()
    assert np.array_equal(a["topk_uids"], want["topk_uids"])
    assert np.array_equal(a["topk_scores"].view(np.uint32), want["topk_scores"].view(np.uint32))
