"""Child process of test_gpu_edge_domain.test_forced_variants_on_edge_corpus: the engine reads
PF_DEBUG once per process, so each forced variant (K5 block sizes, few workgroups, per-call query
images, K1 with split records and global tables) runs the edge corpus "E" in its own process:
all-candidates top-64 and top-10 for the planted queries and every 9th user, twice (the second
pass reuses the rendezvous state), the golden pairs, and the three recommenders, against the
oracle and the reference's goldens.  Exits non-zero on any mismatch."""
import sys

import numpy as np

import edge_corpus as ec
import pokec_testlib as tl


def same(g, r):
    return list(g[0]) == list(r[0]) and np.array_equal(g[1].view(np.uint32), r[1].view(np.uint32))


def main():
    c = tl.golden_corpus("E")
    eng, orc = tl.engine(c), tl.Oracle(c)
    q = [ec.uid_of(i) for i in sorted(set(ec.PLANTED_QUERIES) | set(range(0, ec.N_USERS, 9)))]
    for k in (64, 10):
        ref = orc.interest(q, k, tl.PF_MODE_ALL, 0)
        for rep in range(2):
            for u, g, r in zip(q, eng.recommend_interest_all(q, k), ref):
                if not same(g, r):
                    print(f"mismatch uid={u} k={k} rep={rep}", file=sys.stderr)
                    return 1
    a, b, s = tl.golden_pairs("E")
    nbad = int(np.count_nonzero(eng.fas_pairs(a, b).view(np.uint32) != s))
    if nbad:
        print(f"{nbad} pair mismatches", file=sys.stderr)
        return 1
    qc = q[::5]
    for name, fe, fo in (("collab", eng.recommend_collaborative, orc.collab), ("clubs", eng.recommend_clubs_collab, orc.clubs)):
        for u, g, r in zip(qc, fe(qc, 20, 1000), fo(qc, 20, 1000)):
            if not same(g, r):
                print(f"{name} mismatch uid={u}", file=sys.stderr)
                return 1
    for u, g, r in zip(qc, eng.recommend_interest(qc, 20, tl.PF_MODE_FOF, 1000), orc.interest(qc, 20, tl.PF_MODE_FOF, 1000)):
        if not same(g, r):
            print(f"interest mismatch uid={u}", file=sys.stderr)
            return 1
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
