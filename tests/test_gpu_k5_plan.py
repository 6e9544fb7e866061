"""K5's round planning on the device: the serial next_round and the lane-parallel plan_round
(csrc/pf_plan.h) over the same inputs, one wave per case (tools/probe/k5_plan.hip, built by
__graft_entry__.build() through tools/Makefile): 0, 1, 2, 47 and 48 active columns of 1, 63, 64, 65
and 200 tokens; rounds that end exactly at the entry cap, one entry past it, and on a single token
above it; all-empty lists; 3,000 seeded random cases.  Every round tuple and every round count must
agree, and the sweep must hold cases of three or more rounds and split columns."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "probe", "k5_plan")


@pytest.mark.gpu
def test_lane_planner_equals_serial_planner():
    assert os.path.exists(PROBE), "tools/probe/k5_plan not built (run __graft_entry__.build())"
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\nOK" in r.stdout, r.stdout + r.stderr
    m = re.search(r"cases (\d+) rounds (\d+) max_rounds (\d+) three_plus (\d+) splits (\d+) no_rounds (\d+)", r.stdout)
    assert m, r.stdout
    cases, rounds, max_rounds, three, splits, none = map(int, m.groups())
    assert cases >= 3150 and three > 0 and splits > 0 and max_rounds >= 3 and rounds > cases


def test_k5_plan_probe_source_present():
    assert os.path.exists(PROBE + ".hip")
