"""Clubs by interest (pf_recommend_clubs_interest / _profile / _group; csrc/pf_clubsum.hip): club
recommendations from a collecting scan's neighbours.  Checked against the definition restated in Python
(tests/club_corpus.py) over the oracle's whole ranking, cut in numpy to the filter and the window, and
the corpus's club lists (tests/gpu_club_interest_check.py, one fresh process per PF_DEBUG setting): ids,
counts, info and float32 bits equal.  Corpora: the edge corpus E (its categories are asserted on the CPU
by test_club_interest_cpu), its first 2 / 512 / 513 users, and the seeded 20,000-user synthetic corpus."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(debug, *mode):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_club_interest_check.py"), *mode], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("shape", ["", "scan=stream", "clubs_cutover=2"])
def test_clubs_by_uid(shape):
    run(shape, "full")


@pytest.mark.parametrize("mode", ["state", "profile", "group", "small", "big"])
def test_clubs_through(mode):
    run("", mode)


@pytest.mark.parametrize("shape", ["", "scan=stream"])
def test_nothing_sticks_and_refusals(shape):
    run(shape, "sticks")
