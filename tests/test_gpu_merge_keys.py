"""pf_merge_keys_async (topk_merge_kernel, pf_kernels.hip) as an operation: synthetic uint64 keys
parts[nparts][nq][k] in, row q of the result compared with np.sort(parts[:, q, :].ravel())[:k].

The kernel reads blockDim * 8 = 8192 keys per trip of its input loop, so at k = 64 the part counts
127, 128, 129 and 200 are the last fill of one trip, exactly one trip, one key into the second trip
and well past it; the scans' own merges (2 to 8 parts) never leave the first.  Every part count runs
at k = 64 and k = 1 with 3 queries, every k and query count at 3 and at 129 parts.  Contents: unique
random keys, sorted parts with ~0 tails, whole parts of ~0, nothing but ~0, one list in two parts
(duplicates: the multiset's k smallest), the winners all in the last part, one winner per part, keys
that differ only in their low word.  Only an engine's context is needed: the first 2 users of the
edge corpus."""
import tempfile

import numpy as np
import pytest

import edge_corpus as ec
import pokec_testlib as tl

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
KS = (1, 2, 10, 63, 64)
NQS = (1, 3, 17)
NPARTS = (1, 2, 3, 8, 16, 127, 128, 129, 200)
TRIP = 1024 * 8  # keys per trip of the kernel's input loop (kMergeThreads * 8)
SHAPES = sorted(set([(p, 3, k) for p in NPARTS for k in (64, 1)] + [(p, nq, k) for p in (3, 129) for nq in NQS for k in KS]))
CONTENTS = ("unique", "sorted_tails", "empty_parts", "all_empty", "same_list_twice", "winners_in_last_part",
            "one_winner_per_part", "low_word_only")


def test_shapes_cover_the_second_trip():
    assert 127 * 64 < TRIP == 128 * 64 < 129 * 64
    totals = {p * k for p, nq, k in SHAPES}
    assert {127 * 64, TRIP, TRIP + 64, 200 * 64} <= totals and min(totals) == 1
    assert len(SHAPES) == 2 * len(NPARTS) + 2 * len(NQS) * len(KS) - 4


@pytest.fixture(scope="module")
def eng():
    with tempfile.TemporaryDirectory() as d:
        ec.write_reference_files(d, n_first=2)
        c = tl.read_reference_dir(d)
    e = tl.engine(c)
    yield e
    e.close()


def _keys(rng, shape, lo=0, hi=2**64 - 1):
    """Seeded random keys in [lo, hi): never ~0."""
    return rng.integers(lo, hi, size=shape, dtype=np.uint64)


def _build(kind, nparts, nq, k, rng):
    shape = (nparts, nq, k)
    if kind == "unique":
        p = _keys(rng, shape)
        assert len(np.unique(p)) == p.size
        return p
    if kind == "sorted_tails":  # ascending lists with ~0 tails of differing lengths, as the scans write them
        p = np.sort(_keys(rng, shape), axis=2)
        p[np.arange(k)[None, None, :] >= rng.integers(0, k + 1, size=(nparts, nq, 1))] = NONE
        return p
    if kind == "empty_parts":  # whole parts of ~0: at least one, and where there are two parts, one that is not
        p = np.sort(_keys(rng, shape), axis=2)
        empty = rng.integers(0, 2, size=nparts).astype(bool)
        empty[rng.integers(0, nparts)] = True
        if nparts > 1:
            empty[(int(np.flatnonzero(empty)[0]) + 1) % nparts] = False
        p[empty] = NONE
        return p
    if kind == "all_empty":
        return np.full(shape, NONE, np.uint64)
    if kind == "same_list_twice":
        p = np.sort(_keys(rng, shape), axis=2)
        if nparts > 1:
            a, b = rng.choice(nparts, 2, replace=False)
            p[b] = p[a]
        return p
    if kind == "winners_in_last_part":
        p = _keys(rng, shape, 2**63)
        p[-1] = _keys(rng, (nq, k), 0, 2**62)
        return p
    if kind == "one_winner_per_part":  # winner i in part i mod nparts, at a slot of its own
        p = _keys(rng, shape, 2**63)
        for q in range(nq):
            slots = rng.permutation(k)
            start = int(rng.integers(0, nparts))
            for i in range(k):
                p[(start + i) % nparts, q, slots[i]] = rng.integers(0, 2**62, dtype=np.uint64)
        return p
    if kind == "low_word_only":  # one high word; low words on both sides of 2^31
        lo = _keys(rng, shape, 0, 2**32)
        near = rng.integers(0, 2, size=shape).astype(bool)
        lo[near] = (np.uint64(2**31 - 32) + _keys(rng, shape, 0, 64))[near]
        return (np.uint64(0x3F2A5C71) << np.uint64(32)) | lo
    raise AssertionError(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CONTENTS)
def test_merge_equals_sorted_union(eng, kind):
    import torch
    s = torch.cuda.Stream()
    rng = np.random.default_rng(CONTENTS.index(kind) + 1)
    host = [_build(kind, p, nq, k, rng) for p, nq, k in SHAPES]
    dev = [torch.from_numpy(h.view(np.int64)).cuda() for h in host]
    outs = [torch.full((nq, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda") for p, nq, k in SHAPES]
    torch.cuda.synchronize()
    for (p, nq, k), d, o in zip(SHAPES, dev, outs):
        eng.merge_keys_async(d.data_ptr(), p, nq, k, o.data_ptr(), s.cuda_stream)
    s.synchronize()
    for (p, nq, k), h, o in zip(SHAPES, host, outs):
        got = o.cpu().numpy().view(np.uint64)
        for q in range(nq):
            want = np.sort(h[:, q, :].ravel())[:k]
            assert np.array_equal(got[q], want), (kind, p, nq, k, q, got[q], want)
        if kind == "all_empty":
            assert (got == NONE).all()


@pytest.mark.gpu
def test_argument_checks(eng):
    """nparts = 0, topk = 0 and topk = 65 are PF_EINVAL before anything is launched (the output
    stays as it was); nq = 0 is PF_OK."""
    import torch
    pf = tl.product()
    parts = torch.zeros((2, 1, 64), dtype=torch.int64, device="cuda")
    out = torch.full((1, 65), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for nparts, nq, k in ((0, 1, 10), (2, 1, 0), (2, 1, 65)):
        with pytest.raises(pf.FasError) as e:
            eng.merge_keys_async(parts.data_ptr(), nparts, nq, k, out.data_ptr(), 0)
        assert e.value.code == pf.PF_EINVAL, (nparts, nq, k)
    eng.merge_keys_async(parts.data_ptr(), 2, 0, 10, out.data_ptr(), 0)  # PF_OK: raises otherwise
    torch.cuda.synchronize()
    assert (out == 7).all()
