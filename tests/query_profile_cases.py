"""Cases of the query-by-profile tests (tests/test_query_profile_cpu.py, tests/gpu_query_profile_check.py):
the two users Y and Z that the edge corpus E does not hold, the corpus C+ = E + {Y, Z} the oracle is
opened on, and QueryProfile copies of stored users.

Y sits on the branches only a by-value profile reaches: a gender no E user has, an age no E user has
(below the sigmoid tables' end in one variant, past it in the other), a club nobody holds and a club
listed three times, a column of token ids the corpus does not hold (one above the column's largest),
a column mixing held and novel ids with a tf = 0 token, a column of 70 tokens (two K5 rounds of 64),
and 44 empty columns.  Z is entirely empty: every score is 0 and the order is by uid.
tests/test_query_profile_cpu.py asserts each of these against E's own values."""
import numpy as np

import edge_corpus as ec
import pokec_testlib as tl

UID_Y, UID_Z = 500001, 500002
Y_GENDER = 5
Y_AGES = {"in_table": 100, "past_table": 300}      # kValTab = 128
CLUB_NOBODY, CLUB_TRIPLE = 654321, 12
COL_NOVEL, COL_MIXED, COL_LONG = ec.COL_HC, 7, ec.COL_L
NOVEL_TIDS = [40, 5999, 99999]                     # COL_HC holds 1 .. 30 and 6000 .. 6024 only
MIXED = [(3, 1), (4, 2), (500000, 3), (5, 0)]      # 3, 4: every clone's; 500000: nobody's; 5: tf = 0
LONG = [(tok, 1 + (k * 3) % 5) for k, tok in enumerate(ec.L_TOKENS[:70])]
ADJ_Y = [ec.uid_of(441), ec.uid_of(3), ec.uid_of(1020), 123456789]   # the last has no profile


def y_record(variant="in_table"):
    toks = [dict() for _ in range(ec.N_COLS)]
    toks[COL_NOVEL] = {t: 2 for t in NOVEL_TIDS}
    toks[COL_MIXED] = dict(MIXED)
    toks[COL_LONG] = dict(LONG)
    return {"pub": 1, "comp": 88, "gen": Y_GENDER, "age": Y_AGES[variant], "reg": [3, 9, 27],
            "clubs": [11, CLUB_TRIPLE, CLUB_NOBODY, CLUB_TRIPLE, CLUB_TRIPLE], "friends": [ec.uid_of(70), 424242],
            "toks": toks}


def z_record():
    return {"pub": -1, "comp": -1, "gen": -1, "age": 0, "reg": [-1, -1, -1], "clubs": [], "friends": [],
            "toks": [dict() for _ in range(ec.N_COLS)]}


def profile_of_record(pf, r, exclude=()):
    return pf.QueryProfile.make(public_flag=None if r["pub"] < 0 else r["pub"], gender=None if r["gen"] < 0 else r["gen"],
                                completion=r["comp"] if r["comp"] > 0 else None, age=r["age"] if r["age"] > 0 else None,
                                region=[None if x < 0 else x for x in r["reg"]], clubs=r["clubs"], friends=r["friends"],
                                tokens={t: list(m.items()) for t, m in enumerate(r["toks"]) if m}, exclude=exclude)


def record_of_user(c, i):
    """User i (position in corpus c's arrays) as a record."""
    T = c.n_cols
    toks = []
    for t in range(T):
        a, b = int(c.tok_off[i * T + t]), int(c.tok_off[i * T + t + 1])
        toks.append({int(k): int(v) for k, v in zip(c.tok_tid[a:b], c.tok_tf[a:b])})
    return {"pub": int(c.pub[i]), "comp": int(c.comp[i]), "gen": int(c.gen[i]), "age": int(c.age[i]),
            "reg": [int(x) for x in c.region[3 * i:3 * i + 3]],
            "clubs": [int(x) for x in c.clubs[c.club_off[i]:c.club_off[i + 1]]],
            "friends": [int(x) for x in c.friends[c.friend_off[i]:c.friend_off[i + 1]]], "toks": toks}


def adj_row(c, uid):
    j = np.nonzero(c.adj_uid == uid)[0]
    return [] if len(j) == 0 else [int(x) for x in c.adj_nbr[c.adj_off[j[0]]:c.adj_off[j[0] + 1]]]


def clone_profile(pf, c, uid):
    """A QueryProfile copied from stored user uid's rows, excluding adj[uid] + {uid}: what the by-uid
    all-candidates scan of that user sees.  A stored completion <= 0 / age <= 0 is missing either way."""
    i = int(np.nonzero(c.uid == uid)[0][0])
    return profile_of_record(pf, record_of_user(c, i), exclude=adj_row(c, uid) + [uid])


def append_users(c, recs):
    """Copy of numpy Corpus c with the (uid, record) pairs appended."""
    uid, pub, comp, gen, age, reg = list(c.uid), list(c.pub), list(c.comp), list(c.gen), list(c.age), list(c.region)
    co, cl, fo, fr = list(c.club_off), list(c.clubs), list(c.friend_off), list(c.friends)
    to, tid, tf = list(c.tok_off), list(c.tok_tid), list(c.tok_tf)
    for u, r in recs:
        uid.append(u); pub.append(r["pub"]); comp.append(r["comp"]); gen.append(r["gen"]); age.append(r["age"])
        reg += r["reg"]
        cl += r["clubs"]; co.append(len(cl))
        fr += r["friends"]; fo.append(len(fr))
        for t in range(c.n_cols):
            for k, v in r["toks"][t].items():
                tid.append(k); tf.append(v)
            to.append(len(tid))
    return tl.Corpus(uid, pub, comp, gen, age, reg, co, cl, fo, fr, to, tid, tf, c.adj_uid, c.adj_off, c.adj_nbr,
                     c.n_cols, c.norm_present, c.norm_mean, c.norm_sd, c.median, c.col_names)


def e_explicit():
    """E with the golden explicit idf map: what the engine is opened on."""
    return tl.explicit_idf_corpus("E")


def c_plus(variant="in_table"):
    """C+ = E + {Y, Z}, Y's adj_list row ADJ_Y, under E's explicit idf map and normalisers: what the
    oracle is opened on.  With an explicit map both sides read the same idf."""
    c = append_users(tl.golden_corpus("E"), [(UID_Y, y_record(variant)), (UID_Z, z_record())])
    c = tl.with_rows(c, adj={UID_Y: ADJ_Y})
    present, entries = tl.golden_explicit_idf("E")
    return c.set_explicit_idf(present, entries)


def clone_query_uids():
    """E's planted query users: the A sides of planted_pairs(), the planted queries (the long-column
    users among them) and the clones whose 601 results tie."""
    idx = sorted({a for a, _ in ec.planted_pairs()} | set(ec.PLANTED_QUERIES) | set(ec.CLONE_QUERIES))
    return [ec.uid_of(i) for i in idx]
