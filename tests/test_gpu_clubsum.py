"""Device check of the clubs-by-interest stage (csrc/pf_clubsum.hip) on synthetic ranked keys and club
lists, against the serial loop of its definition inside tools/probe/clubsum.hip (built by
__graft_entry__.build() through tools/Makefile; it links the product's own build/pf_clubsum_k.o).  Sizes on the
stage's edges (nobody, one neighbour, contributions one below / at / one above a workgroup's scan width),
runs of the cut-over length and one either side, one run of every neighbour, every club distinct, own
lists of 0 / 1 / 65,535 entries, club ids up to 2^30 - 1 in a dense order that is not id order, and the
cases that make the order of the adds visible in the float.  The probe's summary line is asserted, so a
sweep that lost one of its categories fails here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "probe", "clubsum")


@pytest.mark.gpu
def test_stage_vs_serial_host_loop():
    assert os.path.exists(PROBE), "tools/probe/clubsum not built (run __graft_entry__.build())"
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.endswith("\nOK\n"), r.stdout + r.stderr
    m = re.search(r"^S ((?:\w+ \d+ ?)+)$", r.stdout, re.M)
    assert m, r.stdout
    w = m.group(1).split()
    s = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    assert s["cases"] >= 27 and s["long_runs"] > 0 and s["short_only"] > 0 and s["ties"] > 0, s
    assert s["own_cases"] >= 2 and s["at_cut"] >= 4 and s["multi_block"] > 0 and s["order_visible"] == 2, s
    # every case well under a second (the first one carries the process's start-up)
    ms = [float(x) for x in re.findall(r" ms ([\d.]+) ok$", r.stdout, re.M)]
    assert len(ms) == s["cases"] and max(ms[2:]) < 500.0, ms


def test_stage_probe_source_present():
    assert os.path.exists(PROBE + ".hip")
