"""K5's pruning (pf_prune.h: candidates that cannot reach the query's shared threshold lose their
text work) against the unpruned kernel and the oracle, bit for bit (tests/gpu_k5_prune_check.py,
one fresh process per PF_DEBUG setting).  A default launch has more workgroups than a small corpus
has blocks, so its threshold stays cold: k5_wgs=1 and k5_wgs=7 with 64-candidate blocks walk the
blocks in turn and prune from the second block on.  The check covers k = 1, 10, 64 and k above the
number of candidates, the edge corpus's 601 byte-identical users (a top-k of ties at the threshold:
the bound's strictness), its 64-200-token columns (a split column across a round end), its three
normaliser modes, a query with every field missing, the 2/511/512/513/1025-user corpora, and both
shards of a seeded 20,000-user corpus merged against the unsharded list.  The counters prove the
path live: every candidate seen, and some dropped where the threshold can warm.  (The batch
instantiation does not prune, so no batch runs here.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(debug, out):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_k5_prune_check.py"), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    stats = [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("stats ")]
    return np.load(out), stats[0]


@pytest.mark.parametrize("shape", ["k5_wgs=1,k5_block=64", "k5_wgs=7,k5_block=64", "", "k5_wgs=1,k5_block=64,k5_prune=1"])
def test_pruned_scan_equals_unpruned(shape, tmp_path):
    pre = shape + "," if shape else ""
    on, st = run(pre + "k5_prune_stats=1", str(tmp_path / "on.npz"))
    off_shape = ",".join(x for x in shape.split(",") if x and not x.startswith("k5_prune="))
    off, st0 = run((off_shape + "," if off_shape else "") + "k5_prune=0,k5_prune_stats=1", str(tmp_path / "off.npz"))
    assert sorted(on.files) == sorted(off.files) and len(on.files) > 0
    for f in on.files:
        assert np.array_equal(on[f], off[f]), f
    print("pruning counters", shape or "(default shape)", st)
    # live: every candidate of every scan counted, and none with the switch off
    assert st["seen"] == st["scans"] * st["n_users"], st
    assert st0["seen"] == 0 and st0["dead_block_start"] == 0 and st0["dead_round_end"] == 0, st0
    if "k5_wgs=1" in shape:
        assert st["dead_block_start"] + st["dead_round_end"] > 0, st
        assert st["cold_blocks"] < st["blocks"], st
