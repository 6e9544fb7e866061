"""bench.py's --dump-outputs helpers on CPU: the per-query (ids, scores) lists as dense float
arrays, and the files they are written to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_topk_arrays_pad_short_lists():
    rows = [(np.array([7, 1632803, 3], np.int32), np.array([0.5, 0.25, 0.125], np.float32)),
            (np.array([], np.int32), np.array([], np.float32))]
    a = bench.topk_arrays(rows, 4)
    assert a["topk_uids"].dtype == np.float64 and a["topk_scores"].dtype == np.float32
    assert a["topk_uids"].tolist() == [[7, 1632803, 3, -1], [-1, -1, -1, -1]]
    assert a["topk_scores"].tolist() == [[0.5, 0.25, 0.125, 0], [0, 0, 0, 0]]


def test_dump_outputs_writes_one_npy_per_name(tmp_path):
    d = str(tmp_path / "out" / "dir")
    arrays = bench.topk_arrays([(np.array([2, 9], np.int32), np.array([1.5, 0.75], np.float32))], 2)
    bench.dump_outputs(d, arrays)
    assert sorted(os.listdir(d)) == ["topk_scores.npy", "topk_uids.npy"]
    for name, a in arrays.items():
        b = np.load(os.path.join(d, name + ".npy"))
        assert b.dtype == a.dtype and np.array_equal(a, b)
