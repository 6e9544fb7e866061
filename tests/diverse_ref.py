"""The definition of diverse top-k (include/pokec_fas.h, "Diverse top-k") in plain Python and numpy:
float32 penalties, float64 values formed by three separately rounded operations, one at a time.

    rerank(uids, rel, sim, lam, topk) -> (ids int32, r float32, pen float32, value float64, positions)

sim(s, idx) -> float32 array: the similarity of pool position s (the picked user, on the A side) with
each position in the int array idx.  It is called once per pick, for row s only."""
import numpy as np

f32, f64 = np.float32, np.float64


def value(lam, r, pen):
    """v of the definition for float32 lam, r, pen (scalars or arrays): a = lam * r, p = (1 - lam) * pen,
    v = a - p, each a float64 operation of its own."""
    dl = f64(f32(lam))
    a = dl * np.asarray(r, f32).astype(f64)
    om = f64(1.0) - dl
    p = om * np.asarray(pen, f32).astype(f64)
    return a - p


def rerank(uids, rel, sim, lam, topk):
    uids = np.asarray(uids, np.int32)
    rel = np.asarray(rel, f32)
    m = len(uids)
    pen = np.zeros(m, f32)
    picked = np.zeros(m, bool)
    every = np.arange(m)
    out = []
    for _ in range(min(int(topk), m)):
        v = value(lam, rel, pen)
        best = -1
        for i in range(m):  # the largest v; the first position among equals
            if not picked[i] and (best < 0 or v[i] > v[best]):
                best = i
        out.append((int(uids[best]), rel[best], pen[best], v[best], best))
        picked[best] = True
        row = np.asarray(sim(best, every), f32)
        pen = np.where(row > pen, row, pen).astype(f32)
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], f32), np.array([o[2] for o in out], f32),
            np.array([o[3] for o in out], f64), [o[4] for o in out])


def same(got, want):
    """ids equal, float32 bits of r and pen equal, float64 bits of value equal (got / want: the first
    four of rerank's results)."""
    return (list(got[0]) == list(want[0]) and
            np.array_equal(np.asarray(got[1], f32).view(np.uint32), np.asarray(want[1], f32).view(np.uint32)) and
            np.array_equal(np.asarray(got[2], f32).view(np.uint32), np.asarray(want[2], f32).view(np.uint32)) and
            np.array_equal(np.asarray(got[3], f64).view(np.uint64), np.asarray(want[3], f64).view(np.uint64)))


# The planted "rounding-visible" triple (found by test_diverse_cpu's search, committed as constants):
# for these float32 values the separately rounded v differs in its bits from the exact value rounded once.
# 1 - lambda rounds here, so v also differs from a - (1 - lambda) * pen contracted into one FMA.
PLANTED_LAMBDA = f32(float.fromhex("0x1.29207ep-13"))
PLANTED_R = f32(float.fromhex("0x1.083a24p-1"))
PLANTED_PEN = f32(float.fromhex("0x1.da95e6p-4"))
PLANTED_VALUE = float.fromhex("-0x1.da38041f99745p-4")       # the definition's v
PLANTED_VALUE_ONCE = float.fromhex("-0x1.da38041f99746p-4")  # the exact value, rounded once
