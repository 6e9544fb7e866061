"""The group query through the front ends: the C++ facade (recommend_for_group, group_similarity;
tests/cpp/facade_group_check.cpp, compiled here), a GROUP transcript through pokec_api_cli, and
app.group_line, which writes the CLI's line.  The expected lists are the engine's own
recommend_group / group_scores, which tests/test_gpu_group.py checks against the host model."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_corpus as ec
import group_ref as gr
import pokec_testlib as tl

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(tl.ROOT, "recommendation-system-pokec_amd")

# (seed set, aggregate, topk, exclude_adj, exclude)
CASES = [("pair", "mean", 10, False, []), ("trio", "min", 20, True, []), ("mixed", "max", 64, False, [gr.U(3), 5]),
         ("n17", "mean", 20, True, [gr.U(9)]), ("clones", "min", 64, True, []), ("excl", "max", 10, True, [])]


def seeds_of(name):
    return gr.model_sets().get(name) or gr.uids(gr.NAMED_SETS[name])


@pytest.fixture(scope="module")
def expected():
    """The engine's lists and fits for CASES, computed once."""
    pf = tl.product()
    eng = tl.engine(tl.golden_corpus("E"))
    try:
        out = []
        for name, agg, k, ea, ex in CASES:
            s = seeds_of(name)
            ids, sc = eng.recommend_group(s, k, agg, exclude=ex, exclude_adj=ea)
            out.append((ids, sc, eng.group_scores(s, ids[:3], agg)))
        return out
    finally:
        eng.close()


def test_cpp_facade_group(tmp_path, expected):
    exe = str(tmp_path / "facade_group_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(tl.ROOT, "include"),
                    os.path.join(HERE, "cpp", "facade_group_check.cpp"), "-L" + PKG, "-lpokec_fas",
                    "-Wl,-rpath," + PKG, "-o", exe], check=True)
    d = str(tmp_path / "E")
    os.makedirs(d)
    ec.write_reference_files(d)
    lines = ["%s %d %d %d %s" % (agg, k, ea, len(ex), " ".join(str(u) for u in ex + seeds_of(name)))
             for name, agg, k, ea, ex in CASES]
    r = subprocess.run([exe, d], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok %d" % len(CASES), r.stdout[-2000:] + r.stderr
    out = r.stdout.splitlines()
    for i, (ids, sc, fit) in enumerate(expected):
        got = [w.split(":") for w in out[2 * i].split()[1:]]
        assert out[2 * i].startswith("list") and [int(a) for a, _ in got] == [int(u) for u in ids], CASES[i]
        assert [int(b, 16) for _, b in got] == [int(x) for x in gr.bits(sc)], CASES[i]
        assert [int(b, 16) for b in out[2 * i + 1].split()[1:]] == [int(x) for x in gr.bits(fit)], CASES[i]


def test_api_cli_group(tmp_path, expected):
    """A GROUP line answers the engine's list in MATCH's list format under the key "group"; a
    malformed line and a refusal answer an error object; the lines around them are answered as ever."""
    sys.path.insert(0, PKG)
    import app as appmod
    exe = os.path.join(PKG, "pokec_api_cli")
    assert os.path.exists(exe), "build with make -C recommendation-system-pokec_amd"
    d = str(tmp_path)
    ec.write_reference_files(d)
    lines = ["PING"]
    for name, agg, k, ea, ex in CASES:
        lines.append(appmod.group_line({"seeds": seeds_of(name), "topk": k, "agg": agg, "exclude": ex, "exclude_adj": ea}))
    lines += ["GROUP", "GROUP 5 median 1003", "GROUP 5 mean", "GROUP 5 mean 1003 colour", "GROUP 5 mean 1003 exclude=7,x",
              "GROUP 65 mean 1003", "GROUP 5 mean " + " ".join(str(gr.U(i)) for i in range(1025)), "GROUP 5 mean 5 7", "PING", "EXIT"]
    p = subprocess.run([exe], cwd=d, input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().splitlines()
    out = out[out.index("READY") + 1:]
    n = len(CASES)
    assert len(out) == len(lines) and out[0] == '{"ok":true}' and out[-2] == '{"ok":true}'
    for line, (ids, sc, _) in zip(out[1:1 + n], expected):
        j = json.loads(line)
        assert list(j) == ["recommendations"] and list(j["recommendations"]) == ["group"]
        got = j["recommendations"]["group"]
        assert [g["id"] for g in got] == [int(i) for i in ids]
        assert ["%.6f" % g["score"] for g in got] == ["%.6f" % float(s) for s in sc]
    assert [json.loads(x)["error"] for x in out[1 + n:8 + n]] == ["bad request"] * 5 + ["engine failure"] * 2
    assert json.loads(out[8 + n]) == {"recommendations": {"group": []}}   # no seed is a user: an empty list
