"""K5's two instantiations against each other and against K1 (tests/gpu_k5_modes_check.py, one
fresh process per PF_DEBUG setting): the one-query claimed launch on the scan lanes and on the
context's own stream, the batch launch, and the record walk, on the edge corpus E and the
2/511/512/513/1025-user corpora.  The claimed instantiation runs every one-query call, the strided
one every 2-query batch.  Launch shapes of the claimed one: k5_wgs 1, 7, 8, 9 and 40 (fewer claim
groups than 8, a non-multiple of 8, more workgroups than E's blocks).  Of the strided one:
k5_batch_blocks 1 (one block per workgroup), 3 with blocks of 64 candidates (E: 22 blocks on 8
workgroups, so the XCD-contiguous order is taken and the last stride round is partial; 1,025 users:
17 blocks on 6 workgroups, no permutation) and 2 with blocks of 333.  Blocks of 64 and 333
candidates on both.  Five settings still carry retired hand-out switches (k5_static, k5_dyn,
k5_tail): PF_DEBUG ignores a retired name like any unknown one, so each runs as the rest of its
setting does (the default launch, k5_wgs 1 / 7 / 40, blocks of 333), and a retired name in front
of a live one must not disturb it.  Bit-exact ids and scores."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("debug", ["", "k5_wgs=1", "k5_wgs=7", "k5_wgs=8", "k5_wgs=9", "k5_wgs=40",
                                   "k5_block=64", "k5_block=333",
                                   "k5_batch_blocks=1", "k5_batch_blocks=3,k5_block=64",
                                   "k5_batch_blocks=2,k5_block=333",
                                   "k5_static=1", "k5_dyn=0,k5_wgs=1", "k5_dyn=0,k5_wgs=7", "k5_dyn=0,k5_wgs=40",
                                   "k5_dyn=0,k5_tail=128,k5_block=333"])
def test_k5_instantiations_agree(debug):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_k5_modes_check.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
