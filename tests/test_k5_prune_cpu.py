"""K5's score bound on the CPU: tests/cpp/prune_check.cpp includes csrc/pf_prune.h, the text the
kernel runs, and sweeps need[u] over T in {0, 1, 48}, every u, theta at every histogram bin edge,
its float neighbours and 1.0, and term sums up to need[u] - 1e-9 and the doubles just below it:
the reference formula's float score must stay strictly below theta."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_need_table_is_a_strict_bound(tmp_path):
    exe = str(tmp_path / "prune_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "recommendation-system-pokec_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "prune_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
