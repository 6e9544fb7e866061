"""Child process of test_gpu_k5_prune: the engine reads PF_DEBUG once per process, so each launch
shape runs once with K5's pruning on (the default, with k5_prune_stats=1) and once with k5_prune=0.
Every query goes through the one-query instantiation (one query per call: the pruned kernel) and is
compared with the oracle here, ids and float32 bits; the lists are also written to argv[1] (npz) so
the test can compare the two processes' bytes.  Corpora: the edge corpus E, its first 2 / 511 /
512 / 513 / 1025 users, and synth.Corpus(20000, seed=3, edge_cases=1), where both shards of
set_shard(r, 2) are merged and compared with the unsharded list and the pruning counters are
printed (`stats` line).  Exits non-zero on any mismatch."""
import json
import sys
import tempfile

import numpy as np

import edge_corpus as ec
import pokec_testlib as tl


def same(g, r):
    return list(g[0]) == list(r[0]) and np.array_equal(np.asarray(g[1], np.float32).view(np.uint32),
                                                       np.asarray(r[1], np.float32).view(np.uint32))


OUT = {}


def keep(tag, g):
    OUT[tag + ".ids"] = np.asarray(g[0], np.int64)
    OUT[tag + ".bits"] = np.asarray(g[1], np.float32).view(np.uint32)


def check(name, c, q, ks):
    eng, orc = tl.engine(c), tl.Oracle(c)
    try:
        if eng.layout().scan_kernel != 2:
            print(f"{name}: the corpus does not run on K5", file=sys.stderr)
            return 1
        for k in ks:
            ref = orc.interest(q, k, tl.PF_MODE_ALL, 0)
            for rep in range(2):  # the second pass starts from the rendezvous state the first one left
                for u, r in zip(q, ref):
                    g = eng.recommend_interest_all([u], k)[0]
                    if not same(g, r):
                        print(f"mismatch {name} uid={u} k={k} rep={rep}", file=sys.stderr)
                        return 1
                    keep(f"{name}.{k}.{u}.{rep}", g)
        return 0
    finally:
        eng.close()


def merged(parts, k):
    rows = sorted(((-float(s), int(u), np.float32(s)) for g in parts for u, s in zip(g[0], g[1])), key=lambda x: x[:2])[:k]
    return [r[1] for r in rows], np.asarray([r[2] for r in rows], np.float32)


def check_synth():
    c = tl.synth.Corpus(n_users=20000, seed=3, edge_cases=1)
    ptr = c.desc_ptr()
    eng, orc = tl.engine(ptr), tl.Oracle(None, desc_ptr=ptr)
    try:
        q = [1, 8, 77, 1500, 2999, 10000, 19999, 20000]
        eng.k5_prune_stats(reset=True)
        scans = 0
        for k in (1, 10, 64):
            ref = orc.interest(q, k, tl.PF_MODE_ALL, 0)
            for u, r in zip(q, ref):
                g = eng.recommend_interest_all([u], k)[0]
                scans += 1
                if not same(g, r):
                    print(f"mismatch synth uid={u} k={k}", file=sys.stderr)
                    return 1
                keep(f"synth.{k}.{u}", g)
                if k == 10:
                    parts = []
                    for r_ in range(2):
                        eng.set_shard(r_, 2)
                        parts.append(eng.recommend_interest_all([u], k)[0])
                    eng.set_shard(0, 1)
                    scans += 1  # the two shards together are one pass over the candidates
                    if not same(merged(parts, k), r):
                        print(f"mismatch synth shards uid={u} k={k}", file=sys.stderr)
                        return 1
        st = eng.k5_prune_stats()
        print("stats " + json.dumps({**st, "scans": scans, "n_users": 20000}))
        return 0
    finally:
        eng.close()


def main():
    e = tl.golden_corpus("E")
    idx = sorted(set(ec.PLANTED_QUERIES) | set(ec.CLONE_QUERIES) | {ec.EMPTY_USER, ec.EXCL_CLONES_Q} |
                 set(range(0, ec.N_USERS, 97)))
    q = [ec.uid_of(i) for i in idx]
    if check("E", e, q, (1, 10, 64)):
        return 1
    for n in (2, 511, 512, 513, 1025):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        qs = [ec.uid_of(i) for i in range(0, n, max(1, n // 12))] + [ec.uid_of(n - 1)]
        if check(f"n{n}", c, qs, (10, 64)):  # k = 64 > the candidates of the 2-user corpus
            return 1
    if check_synth():
        return 1
    if len(sys.argv) > 1:
        np.savez(sys.argv[1], **OUT)
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
