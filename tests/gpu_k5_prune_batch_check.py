"""Child process of test_gpu_k5_prune_batch: the engine reads PF_DEBUG once per process, so each
launch shape runs once with the batches' pruning on (the default, with k5_prune_stats=1) and once
with k5_prune_batch=0.  Every query goes through the batch instantiation (2, 3 or 8 queries per
call, never one) and is compared with the oracle here, ids and float32 bits; the lists are also
written to argv[1] (npz) so the test can compare the two processes' bytes.

Corpora: the edge corpus E, its first 513 / 1025 users, E with one user's friends column replaced
by every friend id of the corpus (the largest LDS a query of E can ask for, next to the empty-field
user's smallest in one batch: the engine launches a batch once per LDS occupancy class), and
synth.Corpus(20000, seed=3, edge_cases=1), where both shards of set_shard(r, 2) are merged and
compared with the unsharded rows.  On E one batch runs under a candidate filter and one under a
field selection.  The pruning counters of the whole process and of the 20,000-user corpus at k = 1
are printed (`stats` line).  Exits non-zero on any mismatch."""
import json
import sys
import tempfile

import numpy as np

import edge_corpus as ec
import field_select_ref as fsr
import gpu_scan_filter_check as fchk
import pokec_testlib as tl
from gpu_k5_prune_check import merged, same

pf = tl.product()
OUT = {}
SEEN = [0]  # candidates the batches must have counted: queries x users of their corpus (two shards: one pass)
HUB = ec.uid_of(700)  # a plain user (no clone, not planted)


def keep(tag, g):
    OUT[tag + ".ids"] = np.asarray(g[0], np.int64)
    OUT[tag + ".bits"] = np.asarray(g[1], np.float32).view(np.uint32)


def fail(*a):
    print("mismatch", *a, file=sys.stderr)
    return 1


def batches(q):
    """q in batches of 2, 3, 8, 2, ... queries; a last batch of one is filled up from the front."""
    out, i, sizes = [], 0, (2, 3, 8)
    while i < len(q):
        n = sizes[len(out) % 3]
        b = q[i:i + n]
        if len(b) < 2:
            b = b + q[:2 - len(b)]
        out.append(b)
        i += n
    return out


def run_batches(name, eng, n_users, bs, k, expect):
    for bi, b in enumerate(bs):
        got = eng.recommend_interest_all(b, k)
        SEEN[0] += len(b) * n_users
        for j, (u, g) in enumerate(zip(b, got)):
            if not same(g, expect(u)):
                return fail(name, "uid", u, "k", k, "batch", bi, list(g[0])[:4], list(expect(u)[0])[:4])
            keep(f"{name}.{k}.{bi}.{j}", g)
    return 0


def check(name, c, q, ks, twice=()):
    eng, orc = tl.engine(c), tl.Oracle(c)
    try:
        if eng.layout().scan_kernel != 2:
            return fail(f"{name}: the corpus does not run on K5")
        for k in ks:
            ref = dict(zip(q, orc.interest(q, k, tl.PF_MODE_ALL, 0)))
            bs = batches(q)
            if len(q) <= 8:
                bs.append(list(q))  # and all of them in one call
            if twice:  # the same uid twice in one batch: two ScanSyncs, equal rows
                bs += [[twice[0], twice[1], twice[0]], [twice[1], twice[1]]]
            for rep in range(2 if k == 10 else 1):  # the second pass reuses the pool the first one left
                if run_batches(f"{name}.r{rep}", eng, c.n_users, bs, k, lambda u: ref[u]):
                    return 1
        return 0
    finally:
        eng.close()


def check_filter_select(c, q8):
    """One batch under a candidate filter (<false, true>), one under a field selection (<false, false, true>)."""
    eng, orc = tl.engine(c), tl.Oracle(c)
    try:
        f = fchk.F(gender=1, keep_missing=True)
        mask, ref = fchk.np_pass(c, f), fchk.Ref(c, orc)
        s = pf.FieldSelect.make(cols=[t for t in range(ec.N_COLS) if t not in ec.COLS_HS[::2]])
        sref = fsr.SelRef(c, s)
        for k in (1, 10, 64):
            got = eng.recommend_interest_all(q8, k, filter=f)
            SEEN[0] += len(q8) * c.n_users
            for u, g in zip(q8, got):
                if not same(g, ref.expect(u, mask, k)):
                    return fail("E filtered batch", u, k)
                keep(f"Ef.{k}.{u}", g)
            got = eng.recommend_interest_all(q8, k, select=s)
            SEEN[0] += len(q8) * c.n_users
            for u, g in zip(q8, got):
                if not same(g, sref.expect(u, k, None)):
                    return fail("E selected batch", u, k)
                keep(f"Es.{k}.{u}", g)
        return 0
    finally:
        eng.close()


def check_synth():
    n = 20000
    c = tl.synth.Corpus(n_users=n, seed=3, edge_cases=1)
    ptr = c.desc_ptr()
    eng, orc = tl.engine(ptr), tl.Oracle(None, desc_ptr=ptr)
    try:
        q = [1, 8, 77, 1500, 2999, 10000, 19999, 20000]
        k1 = None
        for k in (1, 10, 64):
            ref = dict(zip(q, orc.interest(q, k, tl.PF_MODE_ALL, 0)))
            st0 = eng.k5_prune_stats()
            if run_batches("synth", eng, n, [q, q[:3], q[3:5], q[5:]], k, lambda u: ref[u]):
                return 1
            if k == 1:
                st1 = eng.k5_prune_stats()
                k1 = {x: st1[x] - st0[x] for x in st1}
            if k == 10:
                parts = []
                for r_ in range(2):
                    eng.set_shard(r_, 2)
                    parts.append(eng.recommend_interest_all(q, k))
                eng.set_shard(0, 1)
                SEEN[0] += len(q) * n  # the two shards together are one pass over the candidates
                for j, u in enumerate(q):
                    if not same(merged([parts[0][j], parts[1][j]], k), ref[u]):
                        return fail("synth shards", u, k)
        st = eng.k5_prune_stats()
        print("stats " + json.dumps({**st, "expected_seen": SEEN[0], "synth_k1": k1}))
        return 0
    finally:
        eng.close()


def main():
    e = tl.golden_corpus("E")
    idx = sorted(set(ec.PLANTED_QUERIES) | set(ec.CLONE_QUERIES) | {ec.EMPTY_USER, ec.EXCL_CLONES_Q} |
                 set(range(0, ec.N_USERS, 97)))
    q = [ec.uid_of(i) for i in idx]
    eng0 = tl.engine(e)
    eng0.k5_prune_stats(reset=True)  # the counters are the process's: zeroed once, read at the end
    eng0.close()
    if check("E", e, q, (1, 10, 64), twice=(ec.uid_of(ec.CLONE_QUERIES[2]), ec.uid_of(ec.Q_LONG[200]))):
        return 1
    if check_filter_select(e, [ec.uid_of(i) for i in (ec.Q_LONG[129], ec.Q_TWO_LONG, ec.EMPTY_USER, ec.EXCL_CLONES_Q,
                                                       ec.CLONE_QUERIES[0], ec.CLONE_QUERIES[4], 44, 679)]):
        return 1
    # the hub: every friend id anybody of E holds, in one user's friends column (one set list each)
    hub = tl.with_rows(e, user=HUB, friends=np.unique(e.friends))
    print("hub friend ids", len(np.unique(e.friends)), file=sys.stderr)
    hq = [HUB, ec.uid_of(ec.EMPTY_USER), ec.uid_of(ec.Q_LONG[200]), ec.uid_of(ec.CLONE_QUERIES[1]), HUB,
          ec.uid_of(ec.EXCL_CLONES_Q), ec.uid_of(ec.Q_TWO_LONG), ec.uid_of(3)]
    if check("Ehub", hub, hq, (1, 10, 64)):
        return 1
    for n in (513, 1025):
        with tempfile.TemporaryDirectory() as d:
            ec.write_reference_files(d, n_first=n)
            c = tl.read_reference_dir(d)
        qs = [ec.uid_of(i) for i in range(0, n, max(1, n // 12))] + [ec.uid_of(n - 1)]
        if check(f"n{n}", c, qs, (1, 10, 64)):
            return 1
    if check_synth():
        return 1
    if len(sys.argv) > 1:
        np.savez(sys.argv[1], **OUT)
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
