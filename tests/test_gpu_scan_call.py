"""A scan call's options travel by value (csrc/pf_scan_call.h) and the synchronous calls share one
helper (pf_scan_host.cpp SyncScan): counted calls of more than one 256-query chunk, by uid and by value, under
K1 and K5, and one engine serving calls of every kind in turn, each with other options than the one
before (tests/gpu_scan_call_check.py, a fresh process each).  On the edge corpus E, against the
oracle's ranking cut in numpy: ids, float32 bits, totals and the stored results equal."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run(*mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_scan_call_check.py"), *mode],
                       env={**os.environ, "PF_DEBUG": ""}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("kernel", ["auto", "stream"])
def test_counted_call_of_more_than_one_chunk(kernel):
    run("chunks", kernel)


def test_calls_of_every_kind_in_turn_on_one_engine():
    run("mixed")
