"""Device check of the diverse top-k stage (csrc/pf_diverse.hip) on synthetic pools and pair-score
matrices, against the serial loop of its definition inside tools/probe/diverse.hip (built by
__graft_entry__.build() through tools/Makefile; it links the product's own build/pf_diverse_k.o).  Pools of
1, 2, 63, 64, 65, 128, 1023 and 1024 users, topk 1, 2, 64, M and M + 5, lambda 0, 1, 0.5, 0.7f and the
planted triple's, the pool given as collect keys and as plain arrays; all-equal values, equal maxima in
two waves and in lanes 0 and 63 of one, the winner at position M - 1, matrices that are not symmetric, a
penalty that stays at an earlier value and the rounding-visible triple (tests/diverse_ref.py).  uid, r
and pen are compared by their bits, the value by its 64.  The probe's summary line is asserted, so a
sweep that lost one of its categories fails here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "probe", "diverse")


@pytest.mark.gpu
def test_stage_vs_serial_host_loop():
    assert os.path.exists(PROBE), "tools/probe/diverse not built (run __graft_entry__.build())"
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.endswith("\nOK\n"), r.stdout[-3000:] + r.stderr
    m = re.search(r"^S ((?:\w+ \d+ ?)+)$", r.stdout, re.M)
    assert m, r.stdout[-3000:]
    w = m.group(1).split()
    s = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    assert s["cases"] >= 8 * 5 * 5 * 2 + 16 and s["keys"] > 0 and s["plain"] > 0 and s["multi_wave"] > 0, s
    assert s["ties"] > 0 and s["cross_wave_ties"] > 0 and s["all_equal"] == 2 and s["last_pos"] >= 6 and s["lane_ends"] == 1, s
    assert s["asym"] >= 5 and s["pen_kept"] == 2 and s["rounding"] == 2 and s["past_m"] > 0, s
    # every case well under a second (the first one carries the process's start-up)
    ms = [float(x) for x in re.findall(r" ms ([\d.]+) ok$", r.stdout, re.M)]
    assert len(ms) == s["cases"] and max(ms[2:]) < 500.0, ms


def test_stage_probe_source_present():
    assert os.path.exists(PROBE + ".hip")
