"""Group query (pf_recommend_group, pf_group_scores, pf_group_plan_of): the top-k users most similar
to a set of seed users, by fas_group_kernel (tests/gpu_group_check.py, one fresh process per mode:
the engine reads PF_DEBUG once).

References.  G = 1 with exclude_adj is the by-uid all-candidates scan.  For G > 1 the host model
tests/group_ref.py (per-pair floats from the oracle, or from fas_pairs(select=) under a selection;
tests/test_group_cpu.py checks the model itself) gives the expected ids and score bits: seed sets of
2 .. 200 users with EMPTY_USER, clones, the long-column and hit-list users, noisy seed lists, a
permuted set, 1024 seeds.  The same bits must come out however the seeds are packed into passes
(PF_DEBUG group_tile), with records split over lanes, with the query tables in global memory (all
of them, or some), on the wide store, under a filter, a selection, both, and over shards merged on
the host.  group_scores, the pair-kernel route, must agree with the scan.  Nothing sticks to the
context, and the documented refusals are returned."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(mode, *args, debug=""):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_group_check.py"), mode, *args], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_one_seed_is_the_by_uid_scan():
    run("anchor")


@pytest.mark.parametrize("debug", ["", "group_lds=163840"], ids=["default-budget", "whole-lds"])
def test_groups_against_the_host_model(debug):
    """Under the default LDS budget of a pass, and with a workgroup's whole LDS (many images per pass)."""
    run("model", debug=debug)


def pack(lds, fixed, budget, tile):
    """The packing rule of include/pokec_fas.h: the longest prefix that fits, at least one image."""
    passes, i = 0, 0
    while i < len(lds):
        used, n = 0, 0
        while i < len(lds) and (n == 0 or ((tile == 0 or n < tile) and used + lds[i] + fixed <= budget)):
            used += lds[i]
            n += 1
            i += 1
        passes += 1
    return passes


def test_passes_give_the_same_bits():
    """G = 5 in 5, 3, 2 passes and in the default packing: identical lists, and n_passes follows the
    packing rule recomputed here from the images' sizes."""
    outs = {}
    for tile in (1, 2, 3, 0):
        # the forced runs take a workgroup's whole LDS, so that the cap alone decides the packing
        out = run("passes", debug="group_tile=%d,group_lds=163840" % tile if tile else "")
        outs[tile] = plan_line(out)
    assert [outs[t]["n_passes"] for t in (1, 2, 3)] == [5, 3, 2]
    for tile, o in outs.items():
        assert o["n_seeds"] == 5 and o["n_passes"] >= 1
        assert o["n_passes"] == pack(o["lds"], o["fixed"], o["budget"], tile), (tile, o["n_passes"])
        assert o["lists"] == outs[1]["lists"], tile
        assert o["stream_bytes"] == o["n_passes"] * (outs[1]["stream_bytes"] // 5) > 0
    assert len(outs[1]["lists"]) == 18


def test_split_records():
    run("variant", "packed", "any", debug="tile_steps=1")


def test_tables_in_global_memory():
    run("variant", "packed", "all", debug="stage_limit=0")


def plan_line(out):
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])


def test_some_tables_in_global_memory():
    """A staging limit between two seeds' table sizes: 0 < n_global < G, LDS and global-memory
    images side by side in one pass.  An image's LDS bytes are its constants plus its staged tables;
    under stage_limit=0 every image takes the constants alone, which gives the tables' sizes."""
    o, z = plan_line(run("passes")), plan_line(run("passes", debug="stage_limit=0"))
    assert o["n_global"] == 0 and z["n_global"] == 5 and len(set(z["lds"])) == 1
    assert z["lists"] == o["lists"]
    tables = sorted(x - z["lds"][0] for x in o["lds"])
    assert tables[0] < tables[-1]
    run("variant", "packed", "some", debug="stage_limit=%d" % ((tables[0] + tables[-1]) // 2))


def test_wide_store():
    run("variant", "wide", "any")


def test_filter_selection_and_shards():
    run("state")


def test_group_scores_agree_with_the_scan():
    run("scores")


def test_small_corpora():
    run("small")


def test_nothing_sticks_and_errors():
    run("sticks")
