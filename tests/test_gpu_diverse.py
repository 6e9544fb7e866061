"""Diverse top-k (pf_diverse_rerank, pf_recommend_diverse_interest / _profile / _group;
csrc/pf_diverse.hip): a scan's neighbours re-ranked by maximal marginal relevance.  Checked against the
definition restated in Python (tests/diverse_ref.py) over the oracle's whole ranking, cut in numpy to the
filter and the window, with Oracle.fas_pairs(picked, pool) as the similarity
(tests/gpu_diverse_check.py, one fresh process per PF_DEBUG setting): ids, float32 bits of the relevance
and the penalty, float64 bits of the value and info equal.  Corpora: the edge corpus E (its 601 tied
users inside a pool of 1024 tie in value across waves), its first 2 / 512 / 513 users, and the seeded
20,000-user synthetic corpus."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(debug, *mode):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_diverse_check.py"), *mode], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("shape", ["", "scan=stream"])
def test_diverse_by_uid(shape):
    run(shape, "full")


@pytest.mark.parametrize("mode", ["state", "profile", "group", "small", "big", "rerank"])
def test_diverse_through(mode):
    run("", mode)


@pytest.mark.parametrize("shape", ["", "scan=stream"])
def test_nothing_sticks_and_refusals(shape):
    run(shape, "sticks")
