"""K5's theta derivation by slabs on the CPU: tests/cpp/derive_check.cpp includes csrc/pf_prune.h,
the bin arithmetic the kernel's prune_derive runs (slab and lane to bin, the live bins above the
block's theta, the pick of the bin where the count from above reaches k), runs it lane by lane and
compares it with a serial scan from the top bin: random histograms, k in {1, 10, 64}, the block's
theta at 0, at every bin edge hit and one bin either side of the answer, counts that reach k exactly
at a slab boundary, an empty histogram, and a pending record counted in registers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_derivation_equals_serial_scan(tmp_path):
    exe = str(tmp_path / "derive_check")
    subprocess.run(["g++", "-O2", "-std=c++17",
                    "-I" + os.path.join(ROOT, "recommendation-system-pokec_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "derive_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
