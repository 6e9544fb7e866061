"""The score window through the front ends: MATCH ... after=... and GROUP ... min=... count through
pokec_api_cli and through the FastAPI wrapper (app.match_line / app.group_line write the CLI's
lines), and the C++ facade's ScoreWindow overloads (tests/cpp/facade_window_check.cpp, compiled
here).  The expected lists are the engine's own windowed recommend_profile / recommend_group, which
tests/test_gpu_scan_window.py checks against the oracle; following "next" for three pages of 7
equals one 21-result call; a line without the window's words answers the line it always did."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_corpus as ec
import group_ref as gr
import pokec_testlib as tl
import query_profile_cases as qc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(tl.ROOT, "recommendation-system-pokec_amd")
SEEDS = gr.uids(gr.SEEDS_MIXED)
FLOOR = 0.125


def clone_body(e, idx, topk):
    """A /api/match body copied from stored user idx's rows (no exclusions: the user itself ranks too)."""
    r = qc.record_of_user(e, idx)
    return {"topk": topk, "public": r["pub"], "gender": r["gen"], "completion": r["comp"], "age": r["age"], "region": r["reg"],
            "clubs": r["clubs"], "friends": r["friends"],
            "tokens": {str(t): [list(kv) for kv in m.items()] for t, m in enumerate(r["toks"]) if m}}, r


def list_line(key, ids, sc):
    """The reply line of a MATCH / GROUP request without the window's words, as api_cli has always
    written it."""
    return '{"recommendations":{"%s":[%s]}}' % (key, ",".join('{"id":%d,"score":%.6f}' % (int(i), float(s)) for i, s in zip(ids, sc)))


def token(score, uid):
    return "%08x:%d" % (int(np.float32(score).view(np.uint32)), int(uid))


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    """The corpus directory and the engine's own lists, computed once."""
    pf = tl.product()
    d = str(tmp_path_factory.mktemp("E"))
    ec.write_reference_files(d)
    e = tl.read_reference_dir(d)
    eng = tl.engine(e)
    try:
        W = pf.ScanWindow.make
        body, rec = clone_body(e, 441, 7)
        prof = qc.profile_of_record(pf, rec)
        out = {"dir": d, "body": body}
        out["match21"] = eng.recommend_profile(prof, 21)[0]
        out["match_floor"] = eng.recommend_profile(prof, 10, window=W(min_score=0.3, count=True))[0]
        out["match_floor_total"] = int(eng.scan_window_totals()[0])
        out["group21"] = eng.recommend_group(SEEDS, 21, "mean", exclude_adj=True)
        out["group_floor"] = eng.recommend_group(SEEDS, 10, "max", window=W(min_score=FLOOR, count=True))
        out["group_floor_total"] = int(eng.scan_window_totals()[0])
        out["interest"] = eng.recommend_interest_all([ec.uid_of(1)], 64)[0]
        rank = eng.recommend_interest_all([ec.uid_of(1)], 64, window=W(min_score=0.15, count=True))[0]
        out["interest_floor"], out["interest_floor_total"] = rank, int(eng.scan_window_totals()[0])
        return out
    finally:
        eng.close()


def follow(ask, first, pages=3):
    """Three requests, each with the "next" token of the one before; the lists concatenated."""
    got, tok = [], None
    for _ in range(pages):
        j = ask({**first, **({"after": tok} if tok else {})})
        key = next(iter(j["recommendations"]))
        got += j["recommendations"][key]
        tok = j.get("next")
        assert tok is not None
    return got


def same_list(got, want):
    ids, sc = want
    return [g["id"] for g in got] == [int(i) for i in ids] and ["%.6f" % g["score"] for g in got] == ["%.6f" % float(s) for s in sc]


def test_api_cli_window_words(expected):
    sys.path.insert(0, PKG)
    import app as appmod
    exe = os.path.join(PKG, "pokec_api_cli")
    assert os.path.exists(exe), "build with make -C recommendation-system-pokec_amd"
    body = expected["body"]
    gbody = {"seeds": SEEDS, "topk": 7, "agg": "mean", "exclude_adj": True}
    # the cursors of pages 2 and 3 are known beforehand from the 21-result lists
    m21, g21 = expected["match21"], expected["group21"]
    lines = ["PING", appmod.match_line(body), appmod.match_line({**body, "min_score": 0.0})]
    lines += [appmod.match_line({**body, "after": token(m21[1][j], m21[0][j])}) for j in (6, 13)]
    lines += [appmod.group_line(gbody), appmod.group_line({**gbody, "count": True})]
    lines += [appmod.group_line({**gbody, "after": token(g21[1][j], g21[0][j])}) for j in (6, 13)]
    lines += [appmod.match_line({**body, "topk": 10, "min_score": 0.3, "count": True}),
              appmod.group_line({"seeds": SEEDS, "topk": 10, "agg": "max", "min_score": FLOOR, "count": True}),
              appmod.group_line({"seeds": SEEDS, "topk": 10, "min_score": 0.99, "count": True}),
              "MATCH 5 min=abc", "MATCH 5 after=3eb58a1f", "GROUP 5 mean 1003 after=zzzzzzzz:5", "MATCH 5 min=nan",
              "MATCH 5 after=7fc00000:3", "PING", "EXIT"]
    p = subprocess.run([exe], cwd=expected["dir"], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().splitlines()
    out = out[out.index("READY") + 1:]
    assert len(out) == len(lines) and out[0] == '{"ok":true}' and out[-2] == '{"ok":true}'
    # without the new words: the line it always was, byte for byte
    assert out[1] == list_line("interest", m21[0][:7], m21[1][:7])
    assert out[5] == list_line("group", g21[0][:7], g21[1][:7])
    # with one: the same list, then "next" (and "total" under count), in that order
    j = json.loads(out[2])
    assert list(j) == ["recommendations", "next"] and j["next"] == token(m21[1][6], m21[0][6])
    assert out[2] == list_line("interest", m21[0][:7], m21[1][:7])[:-1] + ',"next":"%s"}' % j["next"]
    j = json.loads(out[6])
    assert list(j) == ["recommendations", "next", "total"] and j["next"] == token(g21[1][6], g21[0][6])
    # three pages by the cursor = one 21-result call
    pages = [json.loads(out[i])["recommendations"]["interest"] for i in (2, 3, 4)]
    assert same_list(pages[0] + pages[1] + pages[2], m21)
    pages = [json.loads(out[i])["recommendations"]["group"] for i in (6, 7, 8)]
    assert same_list(pages[0] + pages[1] + pages[2], g21)
    # floors with counts
    j = json.loads(out[9])
    assert same_list(j["recommendations"]["interest"], expected["match_floor"]) and j["total"] == expected["match_floor_total"]
    j = json.loads(out[10])
    assert same_list(j["recommendations"]["group"], expected["group_floor"]) and j["total"] == expected["group_floor_total"]
    assert expected["group_floor_total"] > 10 and expected["match_floor_total"] > 10
    assert json.loads(out[11]) == {"recommendations": {"group": []}, "next": None, "total": 0}
    assert [json.loads(x).get("error") for x in out[12:17]] == ["bad request"] * 5


def test_fastapi_window_fields(expected):
    from fastapi.testclient import TestClient
    sys.path.insert(0, PKG)
    import app as appmod
    a = appmod.create_app(expected["dir"], cli_cmd=[os.path.join(PKG, "pokec_api_cli")])
    m21, g21 = expected["match21"], expected["group21"]
    with TestClient(a) as c:
        def match(b):
            r = c.post("/api/match", json=b)
            assert r.status_code == 200, r.text
            return r.json()

        def group(b):
            r = c.post("/api/group", json=b)
            assert r.status_code == 200, r.text
            return r.json()
        body = expected["body"]
        assert match(body) == json.loads(list_line("interest", m21[0][:7], m21[1][:7]))
        assert same_list(follow(match, {**body, "min_score": 0.0}), m21)
        gbody = {"seeds": SEEDS, "topk": 7, "agg": "mean", "exclude_adj": True}
        assert group(gbody) == json.loads(list_line("group", g21[0][:7], g21[1][:7]))
        assert same_list(follow(group, {**gbody, "count": True}), g21)
        j = group({"seeds": SEEDS, "topk": 10, "agg": "max", "min_score": FLOOR, "count": True})
        assert same_list(j["recommendations"]["group"], expected["group_floor"]) and j["total"] == expected["group_floor_total"]
        j = match({**body, "topk": 10, "min_score": 0.3, "count": True})
        assert same_list(j["recommendations"]["interest"], expected["match_floor"]) and j["total"] == expected["match_floor_total"]
        for bad in ({**body, "after": "xyz"}, {**body, "min_score": "0.3"}, {**body, "count": 1}, {**gbody, "after": 5}):
            assert c.post("/api/match" if "seeds" not in bad else "/api/group", json=bad).status_code == 422


def test_cpp_facade_window(tmp_path, expected):
    """include/pokec/recommender.h: recommend_interest_all / recommend_for_group with a ScoreWindow: a
    floor with its total, and three pages of 7 by the cursor."""
    exe = str(tmp_path / "facade_window_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(tl.ROOT, "include"),
                    os.path.join(HERE, "cpp", "facade_window_check.cpp"), "-L" + PKG, "-lpokec_fas",
                    "-Wl,-rpath," + PKG, "-o", exe], check=True)
    u = ec.uid_of(1)
    lines = ["floor %d 64 0.15" % u, "pages %d 7 3" % u, "gpages 7 3 " + " ".join(str(s) for s in SEEDS), "plain %d 64" % u]
    r = subprocess.run([exe, expected["dir"]], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)

    def parse(line):
        p = line.split()
        return int(p[0]), [int(x.split(":")[0]) for x in p[1:]], [int(x.split(":")[1], 16) for x in p[1:]]
    bits = lambda sc: [int(x) for x in np.asarray(sc, np.float32).view(np.uint32)]
    total, ids, sc = parse(out[0])
    assert total == expected["interest_floor_total"] and ids == [int(x) for x in expected["interest_floor"][0]]
    assert sc == bits(expected["interest_floor"][1])
    _, ids, sc = parse(out[1])
    assert ids == [int(x) for x in expected["interest"][0][:21]] and sc == bits(expected["interest"][1][:21])
    _, ids, sc = parse(out[2])
    assert ids == [int(x) for x in expected["group21"][0]] and sc == bits(expected["group21"][1])
    _, ids, sc = parse(out[3])  # the overload without a window is what it was
    assert ids == [int(x) for x in expected["interest"][0]] and sc == bits(expected["interest"][1])
