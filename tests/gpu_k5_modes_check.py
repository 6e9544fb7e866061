"""Child process of test_gpu_k5_modes: the engine reads PF_DEBUG once per process, so each launch
shape (k5_wgs, k5_block, k5_batch_blocks) runs in its own.  On the edge corpus "E" and its first 2,
511, 512, 513 and 1025 users, the same queries go through K5's one-query instantiation (every block
claimed) on the scan lanes (one query per call on a caller's stream) and on the context's own stream
(a one-query call), through the batch instantiation (2-query batches: the static stride, with
k5_batch_blocks and k5_block several workgroups of several blocks each) and through K1 (the record
walk); every list must carry the same ids and the same float32 bits.
Exits non-zero on any mismatch."""
import sys
import tempfile

import numpy as np
import torch

import edge_corpus as ec
import pokec_testlib as tl


def same(g, r):
    return list(g[0]) == list(r[0]) and np.array_equal(np.asarray(g[1], np.float32).view(np.uint32),
                                                       np.asarray(r[1], np.float32).view(np.uint32))


def check(c, q, k):
    pf = tl.product()
    eng = tl.engine(c)
    try:
        if eng.layout().scan_kernel != 2:
            print("the corpus does not run on K5", file=sys.stderr)
            return 1
        eng.set_scan_kernel(1)
        ref = eng.recommend_interest_all(q, k)                       # K1
        eng.set_scan_kernel(2)
        own = [eng.recommend_interest_all([u], k)[0] for u in q]      # one query, the context's stream
        pairs = [eng.recommend_interest_all([u, q[(i + 1) % len(q)]], k) for i, u in enumerate(q)]  # batches of 2
        s = torch.cuda.Stream()
        rows = torch.full((len(q), k), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for i, u in enumerate(q):                                     # one query per call: the scan lanes
            eng.scan_keys_async([u], k, rows[i].data_ptr(), s.cuda_stream)
        s.synchronize()
        keys = rows.cpu().numpy().view(np.uint64)
        for i, u in enumerate(q):
            got = {"own stream": own[i], "lanes": pf.decode_keys(keys[i]), "batch first": pairs[i][0],
                   "batch second": pairs[i - 1][1]}
            for name, g in got.items():
                if not same(g, ref[i]):
                    print(f"mismatch n={c.n_users} uid={u} k={k}: {name} vs K1", file=sys.stderr)
                    return 1
        if c.n_users > 2 and not any(len(r[0]) for r in ref):
            print(f"n={c.n_users}: every list is empty", file=sys.stderr)
            return 1
        return 0
    finally:
        eng.set_scan_kernel(0)
        eng.close()


def main():
    e = tl.golden_corpus("E")
    q = [ec.uid_of(i) for i in sorted(set(ec.PLANTED_QUERIES[::3]) | set(range(0, ec.N_USERS, 97)))]
    if check(e, q, 64) or check(e, q[::4], 10):
        return 1
    for n in (2, 511, 512, 513, 1025):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        qs = [ec.uid_of(i) for i in range(0, n, max(1, n // 12))] + [ec.uid_of(n - 1)]
        if check(c, qs, 64):
            return 1
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
