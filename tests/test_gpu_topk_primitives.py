"""Device checks of the primitives every ranked list goes through, each against a plain host
reference inside tools/probe/topk.hip (built by __graft_entry__.build() through tools/Makefile):
(a) pf_device.h topk_push / topk_insert, one wave per case and the whole list after every round, at
k = 1, 2, 3, 4, 5, 31, 32, 33, 63, 64: random, descending and ascending streams, rounds built for
exactly 0, 1, 2, 3, 4, 5, 63 and 64 qualifying lanes at the low, high and scattered lanes, equal
keys, repeats of the threshold, fewer than k keys, keys that differ in one 32-bit half only, real
score keys; (b) pf_types.h score_key / key_score / key_uid on the device and the host; (c)
wave_incl_scan, wave_last, wave_max_u32, lane_rev64, rdlane64 with two waves per block; (d)
pf_block.h block_rank, block_rank2, block_scan_incl at 4 and 16 waves, called twice in a row.

The probe's summary lines are asserted, so a sweep that never took topk_insert's serial path
(1 to 3 qualifying lanes) or its sort-and-merge path (4 to 64) at some k fails here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "probe", "topk")
# per k: random, descending, ascending, 8 counts x 3 placements, equal keys, threshold repeats,
# fewer than k, low word, high word, real keys
CASES_PER_K, KS = 3 + 8 * 3 + 6, 10


@pytest.mark.gpu
def test_topk_key_scan_and_block_primitives():
    assert os.path.exists(PROBE), "tools/probe/topk not built (run __graft_entry__.build())"
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "\nOK" in r.stdout, r.stdout + r.stderr
    m = re.search(r"^topk cases (\d+) rounds (\d+) q0 (\d+) q1 (\d+) q2 (\d+) q3 (\d+) q4plus (\d+) q64 (\d+)$", r.stdout, re.M)
    assert m, r.stdout
    cases, rounds, q0, q1, q2, q3, q4plus, q64 = map(int, m.groups())
    assert min(q0, q1, q2, q3, q4plus, q64) > 0, r.stdout
    assert cases >= CASES_PER_K * KS and rounds >= 8 * cases, r.stdout
    m = re.search(r"^topk_kq_missing (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) == 0, r.stdout
    m = re.search(r"^keys pairs (\d+) equal_pairs (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 13 * 4 and int(m.group(2)) > 0, r.stdout
    m = re.search(r"^wave cases (\d+) waves_per_block (\d+) wrapped (\d+) lane64 (\d+)$", r.stdout, re.M)
    assert m, r.stdout
    wcases, wpb, wrapped, lane64 = map(int, m.groups())
    assert wcases >= 1 + 64 + 1 + 1 + 64 and wpb >= 2 and wrapped > 0 and lane64 >= 128, r.stdout
    m = re.search(r"^block nw4 cases (\d+) nw16 cases (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 4 + 6 and int(m.group(2)) >= 16 + 6, r.stdout


def test_topk_probe_source_present():
    assert os.path.exists(PROBE + ".hip")
