"""The score window of the all-candidates scans (pf_set_scan_window; csrc/pf_window.h): a floor, a
paging cursor and a match count, against the oracle's whole ranking cut in numpy
(tests/gpu_scan_window_check.py, one fresh process per PF_DEBUG setting and path).  Corpus: the edge
corpus E (1,400 users, three K5 blocks) and its first 2 / 511 / 512 / 513 / 1025 users.  The check
first asserts the facts the cases rest on (the 599- and 601-way ties, the users at or above 0.125),
so a changed corpus cannot empty the test.  Cases: pages of k = 7 / 64 / 1 chained by the cursor
through ties that span pages, waves and block edges; cursors that are not members; floors at the
query's own scores, at the tie values and their float neighbours, around the histogram's low edge
2^-3, below it (the unseeded path), above everybody and at 0 / -1 / 1, each with a count; a floor and
a cursor together.  Paths: K5 one-query at the default shape and with k5_wgs=1 / 7 and 64-candidate
blocks (theta warms, so the floor's seed and the cursor meet a live threshold), k5_prune=0, a batch
of 8 queries in one call, K1, the wide store, a candidate filter, a field selection, three shards
merged on the host, scan_keys_async, recommend_profile, recommend_group and explain=True."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(debug, *mode):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_scan_window_check.py"), *mode], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return [json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("stats ")]


@pytest.mark.parametrize("shape", ["", "k5_wgs=1,k5_block=64", "k5_wgs=7,k5_block=64", "scan=stream"])
def test_one_query_scans_obey_the_window(shape):
    run(shape, "full")


@pytest.mark.parametrize("shape,kind", [("k5_prune=0", "one"), ("", "batch"), ("k5_block=64", "batch"), ("", "wide"),
                                        ("scan=stream", "batch")])
def test_other_launch_shapes_obey_the_window(shape, kind):
    run(shape, "path", kind)


@pytest.mark.parametrize("mode", ["state", "profile", "group", "async", "small", "sticks"])
def test_window_through(mode):
    run("", mode)


def test_a_floor_begins_no_block_cold():
    """A floor at or above the histogram's low edge seeds theta before the first block: under
    k5_prune_stats=1 a floored one-query scan counts no block begun without a threshold, and a counted
    one neither (its theta stays at the seed).  Below the low edge (0.1) the scan is unseeded: only
    its result is asserted (in the check)."""
    st = run("k5_wgs=7,k5_block=64,k5_prune_stats=1", "seed")[0]
    print("pruning counters under floors", st)
    assert st["0.2"]["blocks"] > 0 and st["0.2"]["cold_blocks"] == 0, st
    assert st["0.2 counted"]["blocks"] > 0 and st["0.2 counted"]["cold_blocks"] == 0, st
    assert st["0.1"]["blocks"] > 0, st
    st = run("k5_prune_stats=1", "seed")[0]
    assert st["0.2"]["blocks"] > 0 and st["0.2"]["cold_blocks"] == 0, st
