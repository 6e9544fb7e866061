"""K5's pruning in batch launches (the <false> instantiation: every query of a batch prunes against
its own ScanSync's theta) against the unpruned batches (k5_prune_batch=0) and the oracle, bit for
bit (tests/gpu_k5_prune_batch_check.py, one fresh process per PF_DEBUG setting; batches of 2, 3
and 8 queries, k = 1, 10, 64).  Shapes: the default one (32 blocks of 512 per workgroup: on these
small corpora one workgroup per query); k5_batch_blocks=3,k5_block=64 (several workgroups of
several blocks per query, a partial last stride round); k5_block=64 with k5_batch_blocks above any
block count (one workgroup runs all of a query's blocks in turn: theta warms from the second block
on).  The child covers the same uid twice in one batch, the edge corpus's 601 byte-identical users
(a top-k of ties at the threshold), its empty-field user, the 513- and 1025-user prefixes, a batch
whose queries ask for the corpus's smallest and largest LDS (the engine launches once per LDS
occupancy class; the engine reports no launch count, so the split itself is not asserted), both
shards of a seeded 20,000-user corpus merged against the unsharded rows, one batch under a
candidate filter and one under a field selection.  The counters prove the path live: every
candidate of every batch query seen, none with the switch off, and in the one-workgroup-per-query
shape at k = 1 on the 20,000-user corpus some dropped (after the first block theta is that block's
best score)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ONE_WG = "k5_block=64,k5_batch_blocks=100000"


def run(debug, out):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_k5_prune_batch_check.py"), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    stats = [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("stats ")]
    return np.load(out), stats[0]


@pytest.mark.parametrize("shape", ["", "k5_batch_blocks=3,k5_block=64", ONE_WG])
def test_pruned_batches_equal_unpruned(shape, tmp_path):
    pre = shape + "," if shape else ""
    on, st = run(pre + "k5_prune_stats=1", str(tmp_path / "on.npz"))
    off, st0 = run(pre + "k5_prune_batch=0,k5_prune_stats=1", str(tmp_path / "off.npz"))
    assert sorted(on.files) == sorted(off.files) and len(on.files) > 0
    for f in on.files:
        assert np.array_equal(on[f], off[f]), f
    print("batch pruning counters", shape or "(default shape)", st)
    # live: every candidate of every batch query counted, and none with the switch off
    assert st["seen"] == st["expected_seen"] and st["seen"] > 0, st
    assert st0["seen"] == 0 and st0["dead_block_start"] == 0 and st0["dead_round_end"] == 0 and st0["blocks"] == 0, st0
    if shape == ONE_WG:
        k1 = st["synth_k1"]
        assert k1["dead_block_start"] + k1["dead_round_end"] > 0, st
        assert k1["cold_blocks"] < k1["blocks"], st
