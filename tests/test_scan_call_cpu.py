"""A scan call's options on the CPU: tests/cpp/scan_call_check.cpp includes csrc/pf_scan_call.h and
checks the truth table of make_scan_call (no window, a collector over no window and over a floor, a
cursor turned into K5's idx bound on a small uid table, a count without a collector), of the two
accessors' row offsets and of extras_ok, the check every launcher makes before it launches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_call_truth_table(tmp_path):
    exe = str(tmp_path / "scan_call_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "recommendation-system-pokec_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "scan_call_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
