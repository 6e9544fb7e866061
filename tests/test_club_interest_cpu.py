"""Clubs by interest on the CPU: the guard over the inputs of the GPU checks (on the oracle alone, the
edge corpus E must contain every category tests/gpu_club_interest_check.py relies on), the reference
model's own arithmetic on a hand-made case, the three new exports and the unchanged ABI version, and
the binding's argument passing with a stub library (no device is opened)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import club_corpus as cc
import pokec_testlib as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "recommendation-system-pokec_amd")
sys.path.insert(0, PKG)


@pytest.fixture(scope="module")
def facts():
    import gpu_scan_filter_check as fchk
    import pokec_fas as pf
    c = tl.golden_corpus("E")
    ref = fchk.Ref(c, tl.Oracle(c))

    def cut(rank, w):  # gpu_scan_window_check.cut's floor (that module opens the product library's engine helpers)
        ids, sc = np.asarray(rank[0]), np.asarray(rank[1], np.float32)
        m = sc >= np.float32(w.min_score)
        return ids[m], sc[m]
    return cc.guard_facts(c, ref.ranking, cut, pf.ScanWindow.make)


def test_edge_corpus_holds_every_category(facts):
    print(facts)
    assert facts["tie_pairs"] >= 1, "no two clubs with bit-equal scores: the id tie-break is not exercised"
    assert facts["runs_33"] >= 1 and facts["runs_1"] >= 1, "no club with 33 or more contributions, or none with exactly 1"
    assert facts["dup_neighbours"] >= 1, "no neighbour lists a club twice"
    assert facts["clubless_neighbours"] >= 1, "no neighbour without clubs"
    assert facts["zero_neighbours"] >= 1399, "EMPTY_USER's pairs no longer score 0.0"
    assert facts["own_in_top10"] >= 1 and facts["own_left_out"], "no query whose own clubs would be in its top 10"
    sizes = facts["cut_sizes"]
    assert 0 in sizes and 1 in sizes and any(s > 64 for s in sizes), sizes


def test_reference_model_on_a_hand_made_case():
    class C:
        n_users = 4
        uid = np.array([10, 20, 30, 40], np.int32)
        club_off = np.array([0, 2, 5, 5, 7], np.int64)
        clubs = np.array([7, 9, 9, 9, 5, 7, 5], np.uint32)

        def index(self):
            return {10: 0, 20: 1, 30: 2, 40: 3}
    c = C()
    rows = cc.club_rows(c)
    assert rows == [[7, 9], [9, 9, 5], [], [7, 5]]
    rank = (np.array([20, 40, 30, 10]), np.array([0.5, 0.25, 0.25, 0.0], np.float32))
    ids, sc, info = cc.expect(c, rows, rank, set(), 0, 10)
    # 9: 0.5 twice; 5: 0.5 + 0.25; 7: 0.25 (user 10 scores 0.0 and is skipped, user 30 has no clubs)
    assert list(ids) == [9, 5, 7] and list(sc) == [1.0, 0.75, 0.25]
    assert info == {"total": 4, "used": 4, "contributions": 5, "clubs": 3}
    ids, sc, info = cc.expect(c, rows, rank, {9}, 1, 10)
    assert list(ids) == [5] and list(sc) == [0.5] and info == {"total": 4, "used": 1, "contributions": 1, "clubs": 1}
    assert list(cc.expect(c, rows, rank, {9}, 1, 10, keep_own=True)[0]) == [9, 5]
    assert cc.expect(c, rows, rank, set(), 0, 10, cap=3)[2] == {"total": 4, "used": 0, "contributions": 0, "clubs": 0}
    # the order of the adds decides the float: 1.0, 2^-24, then 200 times 2^-60 stays at the tie and rounds to even
    class D(C):
        n_users = 202
        uid = np.arange(202, dtype=np.int32)
        club_off = np.arange(203, dtype=np.int64)
        clubs = np.full(202, 3, np.uint32)

        def index(self):
            return {i: i for i in range(202)}
    d = D()
    sc = np.array([1.0, 2.0 ** -24] + [2.0 ** -60] * 200, np.float32)
    got = cc.expect(d, cc.club_rows(d), (np.arange(202), sc), set(), 0, 1)
    assert got[1][0] == np.float32(1.0) and np.float32(float(sc[2:].astype(np.float64).sum()) + 2.0 ** -24 + 1.0) > np.float32(1.0)


def test_exports_and_abi_version():
    import pokec_fas as pf
    names = ("pf_recommend_clubs_interest", "pf_recommend_clubs_profile", "pf_recommend_clubs_group")
    assert all(n in pf.EXPORTS for n in names)
    hdr = open(os.path.join(ROOT, "include", "pokec_fas.h")).read()
    assert re.search(r"#define\s+PF_ABI_VERSION\s+2\b", hdr), "the ABI version is no longer 2"
    assert re.search(r"#define\s+PF_CLUBS_KEEP_OWN\s+1u", hdr)
    assert ctypes.sizeof(pf.ClubsQuery) == 24 and ctypes.sizeof(pf.ClubsInfo) == 32
    lib = os.path.join(PKG, "libpokec_fas.so")
    if os.path.exists(lib):
        L = ctypes.CDLL(lib)
        assert L.pf_abi_version() == 2 and all(hasattr(L, n) for n in names)
        L.pf_recommend_clubs_interest.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] + [ctypes.c_int32] + \
            [ctypes.c_void_p] * 4
        assert L.pf_recommend_clubs_interest(None, 1, None, 1, None, None, None, None) != 0  # no context: refused


class StubLib:
    def __init__(self):
        self.calls = []

    def _take(self, name, h, arg, q, k, oc, os_, n, info):
        qq = q._obj
        self.calls.append((name, qq.cap, qq.neighbours, qq.flags, qq.window is not None, k))
        ctypes.cast(n, ctypes.POINTER(ctypes.c_int32))[0] = 2
        ctypes.cast(oc, ctypes.POINTER(ctypes.c_int32))[0] = 77
        info._obj.total, info._obj.used = 9, 5
        return 0

    def pf_recommend_clubs_interest(self, *a):
        return self._take("interest", *a)

    def pf_recommend_clubs_group(self, *a):
        return self._take("group", *a)

    def pf_set_scan_filter(self, h, f):
        self.calls.append(("filter", f is not None))
        return 0

    def pf_last_error(self, h):
        return b"stub"


def test_binding_passes_the_query_and_restores_the_filter():
    import pokec_fas as pf
    eng = pf.FasEngine.__new__(pf.FasEngine)
    eng._L, eng.h = StubLib(), 1
    eng._filter = eng._select = eng._window = None
    eng._collect = 0
    ids, sc, info = eng.recommend_clubs_interest(5, 3, neighbours=64, cap=500, window=pf.ScanWindow.make(min_score=0.2), keep_own=True)
    assert list(ids) == [77, 0] and len(sc) == 2 and info == {"total": 9, "used": 5, "contributions": 0, "clubs": 0}
    assert eng._L.calls == [("interest", 500, 64, pf.PF_CLUBS_KEEP_OWN, True, 3)]
    eng._L.calls.clear()
    eng.recommend_clubs_group([3, 4], 2, agg="min", filter=pf.CandFilter.make(gender=1))
    assert [c[0] for c in eng._L.calls] == ["filter", "group", "filter"] and eng._L.calls[1][1:] == (1 << 20, 0, 0, False, 2)
    assert eng._filter is None and eng._window is None and eng._collect == 0


def test_club_words_parse_on_match_and_group(tmp_path):
    import subprocess
    exe = str(tmp_path / "clubs_line_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "clubs_line_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
