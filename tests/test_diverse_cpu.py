"""Diverse top-k without a GPU: the definition as tests/diverse_ref.py restates it (include/pokec_fas.h,
"Diverse top-k") on planted pools, the rounding-visible triple it commits, and the front ends' words
(app.py diverse_line / match_line / group_line, the /api/diverse route against a stand-in backend)."""
import os
import sys
import textwrap
from fractions import Fraction

import numpy as np
import pytest

import diverse_ref as dr
import pokec_testlib as tl

PKG = os.path.join(tl.ROOT, "recommendation-system-pokec_amd")
sys.path.insert(0, PKG)
f32 = np.float32

ECHO = textwrap.dedent(r'''
    import json, sys
    print("Loaded 2 users total", flush=True)
    print("READY", flush=True)
    for line in sys.stdin:
        if line.split()[:1] == ["EXIT"]:
            print('{"ok":true, "exiting":true}', flush=True)
            break
        print(json.dumps({"line": line.rstrip("\n")}), flush=True)
''')


def matrix_sim(S):
    S = np.asarray(S, f32)
    return lambda s, idx: S[s, idx]


def random_pool(m, seed):
    g = np.random.default_rng(seed)
    return np.arange(100, 100 + m), (g.integers(1, 8, m) / 8).astype(f32), (g.integers(0, 15, (m, m)) / 16).astype(f32)


def test_lambda_one_is_the_pool_prefix():
    u, r, S = random_pool(40, 1)
    r = np.sort(r)[::-1]  # a ranked pool, as a scan gives it: ties in r fall to the position
    ids, rr, pen, val, pos = dr.rerank(u, r, matrix_sim(S), 1.0, 15)
    assert pos == list(range(15)) and list(ids) == list(u[:15]) and np.array_equal(rr, r[:15])
    assert np.array_equal(val, r[:15].astype(np.float64))  # v = r exactly: (1 - 1) * pen is 0


def test_lambda_zero_ignores_relevance_after_the_first_pick():
    u, r, S = random_pool(30, 2)
    ids, rr, pen, val, pos = dr.rerank(u, r, matrix_sim(S), 0.0, 30)
    assert pos[0] == 0 and pen[0] == 0  # everything ties at v = 0: position 0
    # every later pick has the smallest penalty among the unpicked, whatever its relevance; ties by position
    cur, left = np.zeros(30, f32), set(range(30))
    for t, s in enumerate(pos):
        best = min(left, key=lambda i: (cur[i], i))
        assert s == best and pen[t] == cur[s] and val[t] == -np.float64(cur[s])
        left.remove(s)
        cur = np.maximum(cur, S[s])
    r2 = r[::-1].copy()  # other relevances, the same picks
    assert dr.rerank(u, r2, matrix_sim(S), 0.0, 30)[4] == pos


def test_a_penalty_never_falls():
    S = np.zeros((3, 3), f32)
    S[0] = (0, 0.125, 0.75)
    S[1] = (0.5, 0, 0.0625)  # the second pick is far from position 2: its penalty stays 0.75
    ids, rr, pen, val, pos = dr.rerank([7, 8, 9], [0.875, 0.75, 0.5], matrix_sim(S), 0.5, 3)
    assert pos == [0, 1, 2] and list(pen) == [0, f32(0.125), f32(0.75)]
    # and S is read by rows, with the pick on the A side: under the transpose position 1 has pen 0.5 after the
    # first pick and falls behind position 2
    assert dr.rerank([7, 8, 9], [0.875, 0.75, 0.5], matrix_sim(S.T), 0.5, 3)[4] == [0, 2, 1]


def test_ties_go_to_the_lower_position():
    m = 200
    S = np.full((m, m), 0.25, f32)
    ids, rr, pen, val, pos = dr.rerank(np.arange(m)[::-1], np.full(m, 0.5, f32), matrix_sim(S), 0.7, m + 5)
    assert pos == list(range(m)) and list(ids) == list(range(m - 1, -1, -1))  # identical users: the pool's order
    assert len(set(val[1:])) == 1 and val[0] > val[1]
    r = np.full(m, 0.125, f32)
    r[[3, 150]] = 0.875
    assert dr.rerank(np.arange(m), r, matrix_sim(S), 0.5, 3)[4] == [3, 150, 0]
    # -0 and +0 are one value: the lower position wins
    assert dr.rerank([1, 2], [0.0, -0.0], matrix_sim(np.zeros((2, 2))), 1.0, 2)[4] == [0, 1]


def exact_once(lam, r, pen):
    L = Fraction(float(f32(lam)))
    return float(L * Fraction(float(f32(r))) - (1 - L) * Fraction(float(f32(pen))))  # Fraction -> float rounds once, to nearest even


def test_the_planted_triple_makes_the_rounding_visible():
    v = float(dr.value(dr.PLANTED_LAMBDA, dr.PLANTED_R, dr.PLANTED_PEN))
    once = exact_once(dr.PLANTED_LAMBDA, dr.PLANTED_R, dr.PLANTED_PEN)
    assert v == dr.PLANTED_VALUE and once == dr.PLANTED_VALUE_ONCE and v.hex() != once.hex()
    # the same for a - (1 - lambda) * pen contracted into one fused multiply-add
    L = float(dr.PLANTED_LAMBDA)
    fused = float(Fraction(L) * Fraction(float(dr.PLANTED_R)) - Fraction(1.0 - L) * Fraction(float(dr.PLANTED_PEN)))
    assert fused != v
    # as a pool: the second pick carries the value
    S = np.zeros((2, 2), f32)
    S[0, 1] = dr.PLANTED_PEN
    ids, rr, pen, val, pos = dr.rerank([1, 2], [1.0, dr.PLANTED_R], matrix_sim(S), dr.PLANTED_LAMBDA, 2)
    assert pos == [0, 1] and pen[1] == dr.PLANTED_PEN and float(val[1]) == dr.PLANTED_VALUE


def test_the_search_finds_such_triples():
    """How the constants were found: small lambdas, where 1 - lambda itself rounds."""
    g = np.random.default_rng(1)
    found = 0
    for _ in range(400):
        lam = f32(np.ldexp(0.5 + g.random() / 2, -int(g.integers(0, 40))))
        r, pen = f32(g.random()), f32(g.random())
        found += float(dr.value(lam, r, pen)) != exact_once(lam, r, pen)
    assert found > 0


def test_same_compares_bits():
    a = (np.array([1], np.int32), np.array([0.5], f32), np.array([0.0], f32), np.array([0.25]))
    assert dr.same(a, a)
    assert not dr.same(a, (a[0], a[1], np.array([-0.0], f32), a[3]))
    assert not dr.same(a, (a[0], a[1], a[2], np.nextafter(a[3], 1)))


def test_bodies_take_the_diverse_field():
    import app as appmod
    assert appmod.match_line({"topk": 5, "diverse": {"lambda": 0.7}}) == "MATCH 5 diverse=0.7"
    assert appmod.match_line({"topk": 5, "min_score": 0.25, "diverse": {"lambda": 0.5, "pool": 64}}) == "MATCH 5 min=0.25 diverse=0.5 pool=64"
    assert appmod.group_line({"seeds": [3, 4], "diverse": {"lambda": 1, "pool": 1024}}) == "GROUP 20 mean 3 4 diverse=1.0 pool=1024"
    assert appmod.group_line({"seeds": [3], "count": True, "diverse": {"lambda": 0}}) == "GROUP 20 mean 3 count diverse=0.0"
    assert appmod.match_line({"topk": 5}) == "MATCH 5" and appmod.group_line({"seeds": [3]}) == "GROUP 20 mean 3"
    for bad in (0.7, [0.7], {}, {"pool": 5}, {"lambda": -0.1}, {"lambda": 1.5}, {"lambda": float("nan")}, {"lambda": "x"},
                {"lambda": True}, {"lambda": 0.5, "pool": 0}, {"lambda": 0.5, "pool": 1025}, {"lambda": 0.5, "pool": 2.5},
                {"lambda": 0.5, "pool": True}, {"lambda": 0.5, "k": 3}):
        with pytest.raises(ValueError):
            appmod.match_line({"diverse": bad})
        with pytest.raises(ValueError):
            appmod.group_line({"seeds": [3], "diverse": bad})
    for other in ({"all": 100}, {"top_clubs": 4}, {"top_clubs": 4, "neighbours": 9}):  # the reply holds one list
        with pytest.raises(ValueError):
            appmod.match_line({**other, "diverse": {"lambda": 0.5}})
        with pytest.raises(ValueError):
            appmod.group_line({"seeds": [3], **other, "diverse": {"lambda": 0.5}})
    assert appmod.diverse_line(12) == "DIVERSE 20 12 0.7"
    assert appmod.diverse_line(12, 5, 0.25, 64, 0.5) == "DIVERSE 5 12 0.25 pool=64 min=0.5"
    for kw in ({"uid": -1}, {"uid": 1, "topk": -1}, {"uid": 1, "pool": 0}, {"uid": 1, "pool": 1025}, {"uid": 1, "lam": 1.01},
               {"uid": 1, "lam": float("nan")}, {"uid": 1, "lam": "x"}, {"uid": 1, "min_score": float("nan")}, {"uid": 1, "min_score": "x"}):
        with pytest.raises(ValueError):
            appmod.diverse_line(**kw)


def test_diverse_route_against_protocol_stand_in(tmp_path):
    from fastapi.testclient import TestClient
    import app as appmod
    p = tmp_path / "echo_cli.py"
    p.write_text(ECHO)
    a = appmod.create_app(str(tmp_path), cli_cmd=[sys.executable, str(p)], request_timeout=5.0)
    with TestClient(a) as c:
        assert c.get("/api/diverse/12").json() == {"line": "DIVERSE 20 12 0.7"}
        assert c.get("/api/diverse/12", params={"topk": 3, "lam": 0.5, "pool": 100, "min_score": 0.25}).json() == \
            {"line": "DIVERSE 3 12 0.5 pool=100 min=0.25"}
        assert c.get("/api/diverse/12", params={"lam": 2}).status_code == 422
        assert c.get("/api/diverse/12", params={"pool": 0}).status_code == 422
        assert c.get("/api/diverse/abc").status_code == 422
        assert c.post("/api/group", json={"seeds": [1, 2], "diverse": {"lambda": 0.5}}).json() == {"line": "GROUP 20 mean 1 2 diverse=0.5"}
        assert c.post("/api/match", json={"topk": 2, "diverse": {"lambda": 3}}).status_code == 422
