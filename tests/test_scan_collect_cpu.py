"""The scans' collector on the CPU: the two new exports and the unchanged ABI version; collect= and
collect_all restore the collector in force, checked with a stub library under a real FasEngine object
(no device is opened); collect_all with cap=None makes exactly one counted call and one collecting call;
the api_cli's all=<cap> word (tests/cpp/collect_line_check.cpp over csrc/match_line.h) and the FastAPI
wrapper's "all" field."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "recommendation-system-pokec_amd")
sys.path.insert(0, PKG)


def test_exports_and_abi_version():
    import pokec_fas as pf
    assert "pf_set_scan_collect" in pf.EXPORTS and "pf_scan_collected" in pf.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "pokec_fas.h")).read()
    assert re.search(r"#define\s+PF_ABI_VERSION\s+2\b", hdr), "the ABI version is no longer 2"
    assert re.search(r"int pf_set_scan_collect\(pf_ctx\* ctx, int64_t cap\);", hdr)
    assert re.search(r"int pf_scan_collected\(pf_ctx\* ctx, int32_t\* out_uid, float\* out_score, int64_t out_cap,\s*int64_t\* n,\s*int64_t\* total\);", hdr)
    # the collector's bit is the device's own: the public window still has three
    assert "PF_WIN_COLLECT" not in hdr and (pf.PF_WIN_MIN | pf.PF_WIN_AFTER | pf.PF_WIN_COUNT) == 7
    lib = os.path.join(PKG, "libpokec_fas.so")
    if os.path.exists(lib):
        import ctypes
        L = ctypes.CDLL(lib)
        assert L.pf_abi_version() == 2
        assert hasattr(L, "pf_set_scan_collect") and hasattr(L, "pf_scan_collected")
        # no context: refused before anything is touched
        L.pf_set_scan_collect.argtypes = [ctypes.c_void_p, ctypes.c_int64]
        assert L.pf_set_scan_collect(None, 5) != 0


class StubLib:
    """What FasEngine's setters call, recorded."""

    def __init__(self):
        self.calls = []

    def pf_set_scan_collect(self, h, cap):
        self.calls.append(("collect", int(cap)))
        return 0 if 0 <= cap <= 2**31 - 1 else 3

    def pf_set_scan_window(self, h, w):
        self.calls.append(("window", None if w is None else w._obj.fields))
        return 0

    def pf_set_scan_filter(self, h, f):
        self.calls.append(("filter",))
        return 0

    def pf_set_scan_select(self, h, s):
        self.calls.append(("select",))
        return 0

    def pf_last_error(self, h):
        return b"stub"


def stub_engine():
    import pokec_fas as pf
    eng = pf.FasEngine.__new__(pf.FasEngine)
    eng._L, eng.h = StubLib(), 1
    eng._filter = eng._select = eng._window = None
    eng._collect = 0
    return pf, eng


def test_collect_scope_restores_the_collector_in_force():
    pf, eng = stub_engine()
    with eng._scoped(collect=100):
        assert eng._collect == 100
    assert eng._collect == 0 and eng._L.calls == [("collect", 100), ("collect", 0)]
    eng._L.calls.clear()
    eng.set_scan_collect(700)
    eng.set_scan_window(min_score=0.2)
    with eng._scoped(window=pf.ScanWindow.make(count=True), collect=5):
        assert eng._collect == 5 and eng._window.fields == pf.PF_WIN_COUNT
    assert eng._collect == 700 and eng._window.fields == pf.PF_WIN_MIN
    # set on the way in after the window, restored on the way out before it
    assert eng._L.calls == [("collect", 700), ("window", 1), ("window", 4), ("collect", 5), ("collect", 700), ("window", 1)]
    # a call that fails inside the scope restores all the same
    with pytest.raises(RuntimeError):
        with eng._scoped(collect=9):
            raise RuntimeError("the call failed")
    assert eng._collect == 700
    # no collect=: the collector is not touched
    eng._L.calls.clear()
    with eng._scoped(window=pf.ScanWindow.make(min_score=0.5)):
        pass
    assert eng._collect == 700 and all(c[0] != "collect" for c in eng._L.calls)
    eng.clear_scan_collect()
    assert eng._collect == 0
    with pytest.raises(pf.FasError):
        eng.set_scan_collect(-3)
    assert eng._collect == 0


def test_collect_all_counts_once_and_collects_once():
    import pokec_fas as pf
    ranking = [(i, np.float32(1.0 - 0.01 * (i // 3))) for i in range(200)]
    seen = []

    def call(w, collect):
        seen.append((None if w is None else (w.fields, w.min_score), collect))
        rest = [r for r in ranking if w is None or not (w.fields & pf.PF_WIN_MIN) or r[1] >= np.float32(w.min_score)]
        if collect is None:
            return np.zeros(0, np.int32), np.zeros(0, np.float32), len(rest)
        if len(rest) > collect:
            rest_out = []
        else:
            rest_out = rest
        return np.array([r[0] for r in rest_out], np.int32), np.array([r[1] for r in rest_out], np.float32), len(rest)

    w = pf.ScanWindow.make(min_score=0.9)
    ids, sc, total = pf.collect_all(call, w)
    assert total == 33 and list(ids) == list(range(33))
    # exactly two calls: a counted one (the caller's window, with the count bit), then a collecting one of the exact size
    assert len(seen) == 2 and seen[0][1] is None and seen[0][0][0] == pf.PF_WIN_MIN | pf.PF_WIN_COUNT
    assert seen[1][1] == 33 and seen[1][0][0] == pf.PF_WIN_MIN and w.fields == pf.PF_WIN_MIN
    seen.clear()
    ids, sc, total = pf.collect_all(call)  # no window: everybody
    assert total == 200 and len(ids) == 200 and seen == [((pf.PF_WIN_COUNT, 0.0), None), (None, 200)]
    seen.clear()
    ids, sc, total = pf.collect_all(call, pf.ScanWindow.make(min_score=2.0))  # nobody: a buffer of one key
    assert total == 0 and len(ids) == 0 and seen[1][1] == 1
    seen.clear()
    ids, sc, total = pf.collect_all(call, w, cap=10)  # a cap given: the one collecting call, which overflows
    assert total == 33 and len(ids) == 0 and len(seen) == 1 and seen[0][1] == 10


def test_collect_call_reads_the_count_or_the_list():
    pf, eng = stub_engine()
    made = []
    eng.scan_window_totals = lambda: np.array([41], np.int64)
    eng.scan_collected = lambda: (np.arange(3, dtype=np.int32), np.ones(3, np.float32), 3)
    call = eng.collect_call(lambda w, c: made.append((w, c)))
    assert call(None, None)[2] == 41 and call(None, 8)[2] == 3 and made == [(None, None), (None, 8)]


def test_all_word_parses_on_match_and_group(tmp_path):
    exe = str(tmp_path / "collect_line_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "collect_line_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_app_bodies_take_all():
    import app as appmod
    assert appmod.match_line({"topk": 5, "all": 1000}) == "MATCH 5 all=1000"
    assert appmod.match_line({"topk": 5, "min_score": 0.25, "all": 7}) == "MATCH 5 min=0.25 all=7"
    assert appmod.group_line({"seeds": [3, 4], "all": 50, "count": True}) == "GROUP 20 mean 3 4 count all=50"
    assert appmod.match_line({"topk": 5}) == "MATCH 5" and appmod.group_line({"seeds": [3]}) == "GROUP 20 mean 3"
    for bad in (0, -1, 2**31, True, "5", 1.5):
        with pytest.raises(ValueError):
            appmod.match_line({"all": bad})
        with pytest.raises(ValueError):
            appmod.group_line({"seeds": [3], "all": bad})
