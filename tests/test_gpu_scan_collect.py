"""The collector of the all-candidates scans (pf_set_scan_collect / pf_scan_collected; csrc/pf_collect.h):
one scan keeps every candidate of its score window, one device sort ranks them.  Checked against the
oracle's whole ranking cut in numpy to the filter and the window (tests/gpu_scan_collect_check.py, one
fresh process per PF_DEBUG setting and path): ids and float32 bits equal, totals exact, order exact, and
the call's own top-k and count what they are without a collector.  Corpora: the edge corpus E (1,400
users, three K5 blocks; 599- and 601-way ties, asserted first), its first 2 / 511 / 512 / 513 / 1025
users, and the seeded 20,000-user synthetic corpus (some 19,700 keys from many workgroups).  The C++ facade's
three collect methods are checked against the C calls by tests/cpp/facade_collect_check.cpp."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "recommendation-system-pokec_amd")


def run(debug, *mode):
    env = {**os.environ, "PF_DEBUG": debug}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_scan_collect_check.py"), *mode], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("shape", ["", "k5_wgs=1,k5_block=64", "k5_wgs=7,k5_block=64", "k5_prune=0", "scan=stream"])
def test_one_query_scans_collect_the_window(shape):
    run(shape, "full")


@pytest.mark.parametrize("mode", ["caps", "state", "profile", "group", "small", "big", "sticks"])
def test_collect_through(mode):
    run("", mode)


def test_group_collects_in_the_last_of_several_passes():
    out = run("group_tile=1", "group")
    assert "5 passes" in out, out


def test_facade_collect_methods_against_the_c_calls(tmp_path):
    import edge_corpus as ec
    d = str(tmp_path / "E")
    os.makedirs(d)
    ec.write_reference_files(d)
    exe = str(tmp_path / "facade_collect_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "facade_collect_check.cpp"), "-L" + PKG, "-lpokec_fas",
                    "-Wl,-rpath," + PKG, "-o", exe], check=True)
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_api_cli_all_word(tmp_path):
    """MATCH / GROUP ... all=<cap> through pokec_api_cli (lines written by app.match_line / app.group_line):
    the reply's list is the engine's own collected window (checked against the oracle above), then
    "total"; a window above the cap answers an empty list, the total and "overflow":true; a line
    without the word answers the line it always did."""
    import json
    import numpy as np
    import edge_corpus as ec
    import group_ref as gr
    import pokec_testlib as tl
    import query_profile_cases as qc
    sys.path.insert(0, PKG)
    import app as appmod
    pf = tl.product()
    d = str(tmp_path / "E")
    os.makedirs(d)
    ec.write_reference_files(d)
    e = tl.read_reference_dir(d)
    r = qc.record_of_user(e, 441)
    body = {"topk": 7, "public": r["pub"], "gender": r["gen"], "completion": r["comp"], "age": r["age"], "region": r["reg"],
            "clubs": r["clubs"], "friends": r["friends"],
            "tokens": {str(t): [list(kv) for kv in m.items()] for t, m in enumerate(r["toks"]) if m}}
    seeds = gr.uids(gr.SEEDS_MIXED)
    gbody = {"seeds": seeds, "topk": 7, "agg": "mean", "exclude_adj": True}
    eng = tl.engine(e)
    try:
        W = pf.ScanWindow.make
        prof = qc.profile_of_record(pf, r)
        m7 = eng.recommend_profile(prof, 7)[0]
        eng.recommend_profile(prof, 7, window=W(min_score=0.125), collect=5000)
        mall = eng.scan_collected()
        g7 = eng.recommend_group(seeds, 7, "mean", exclude_adj=True)
        eng.recommend_group(seeds, 7, "mean", exclude_adj=True, window=W(min_score=0.125), collect=5000)
        gall = eng.scan_collected()
    finally:
        eng.close()
    assert 64 < mall[2] == len(mall[0]) and 64 < gall[2] == len(gall[0])
    lines = [appmod.match_line(body), appmod.match_line({**body, "min_score": 0.125, "all": 5000}),
             appmod.match_line({**body, "min_score": 0.125, "all": 64}), appmod.group_line(gbody),
             appmod.group_line({**gbody, "min_score": 0.125, "all": 5000, "topk": 0}),
             appmod.group_line({**gbody, "min_score": 0.125, "all": 1}), "MATCH 5 all=0", "GROUP 5 mean 1003 all=x", "PING", "EXIT"]
    exe = os.path.join(PKG, "pokec_api_cli")
    p = subprocess.run([exe], cwd=d, input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().splitlines()
    out = out[out.index("READY") + 1:]
    assert len(out) == len(lines) and out[-2] == '{"ok":true}'

    def plain(key, ids, sc):
        return '{"recommendations":{"%s":[%s]}}' % (key, ",".join('{"id":%d,"score":%.6f}' % (int(i), float(s)) for i, s in zip(ids, sc)))
    assert out[0] == plain("interest", *m7) and out[3] == plain("group", *g7)
    assert out[1] == plain("interest", mall[0], mall[1])[:-1] + ',"total":%d}' % mall[2]
    assert json.loads(out[2]) == {"recommendations": {"interest": []}, "total": mall[2], "overflow": True}
    assert out[4] == plain("group", gall[0], gall[1])[:-1] + ',"total":%d}' % gall[2]
    assert json.loads(out[5]) == {"recommendations": {"group": []}, "total": gall[2], "overflow": True}
    assert [json.loads(x).get("error") for x in out[6:8]] == ["bad request"] * 2
