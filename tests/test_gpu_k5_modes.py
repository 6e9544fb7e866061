"""K5's two instantiations against each other and against K1 (tests/gpu_k5_modes_check.py, one
fresh process per PF_DEBUG setting): the one-query claimed launch on the scan lanes and on the
context's own stream, the generic launch, and the record walk, on the edge corpus E and the
2/511/512/513/1025-user corpora.  The generic instantiation runs every 2-query batch, and the
one-query launches whose mode word has bit 3 (every block claimed) clear, which takes k5_dyn=0:
static rounds with the tail claimed (k5_dyn=0), static rounds alone (k5_dyn=0,k5_static=1), finer
claimed tail blocks (k5_dyn=0,k5_tail=128), the XCD order of the static rounds off
(k5_dyn=0,k5_xcd=0).  k5_static=1 alone keeps bit 3 and stays on the claimed instantiation, where
the flag changes nothing.  Launch shapes: k5_wgs 1, 7, 8, 9 and 40 (fewer claim groups than 8, a
non-multiple of 8, more workgroups than E's blocks), on both instantiations, and blocks of 64 and
333 candidates.  Bit-exact ids and scores."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("debug", ["", "k5_static=1", "k5_wgs=1", "k5_wgs=7", "k5_wgs=8", "k5_wgs=9", "k5_wgs=40",
                                   "k5_block=64", "k5_block=333",
                                   "k5_dyn=0", "k5_dyn=0,k5_static=1", "k5_dyn=0,k5_tail=128", "k5_dyn=0,k5_xcd=0",
                                   "k5_dyn=0,k5_wgs=1", "k5_dyn=0,k5_wgs=7", "k5_dyn=0,k5_wgs=40",
                                   "k5_dyn=0,k5_tail=128,k5_block=333"])
def test_k5_instantiations_agree(debug):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_k5_modes_check.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
