"""The host helpers the scan and pair launchers share, on the CPU (g++, no HIP include):
tests/cpp/stage_check.cpp checks csrc/pf_stage.h, the byte layouts of the three staging buffers, against
offsets and totals written out as numbers; tests/cpp/pair_groups_check.cpp checks csrc/pf_pair_groups.h,
the grouping of pairs by their query that decides the pair kernel's waves."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["stage_check", "pair_groups_check"])
def test_host_helper_check(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "recommendation-system-pokec_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
