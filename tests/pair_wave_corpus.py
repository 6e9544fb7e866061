"""Planted waves for the pair kernel K1' (fas_pairs_kernel, csrc/pf_kernels.hip): a closed-formula corpus
whose candidates produce a known number of epilogue items against the query Q, the compositions of 64
lanes the GPU tests issue (tests/test_gpu_pair_waves.py), and a plain host model of pair_epilogue's
split of a wave into queue rounds.  tests/test_pair_wave_cpu.py guards every planted number.

Why whole waves: pair_epilogue is not a per-pair function.  Every dense lane turns its hits into items
(one per hit column the query selects, one for a non-empty club intersection, one for a friend
intersection), the items of a wave share a queue of kQueue = 384 entries, lanes past the queue take a
second round, a wave whose second round overflows too falls back to the per-lane epilogue, and a lane
whose hit list reached kHitCap is re-walked by the whole wave.  The public call fixes which 64 pairs
share a wave: pf_fas_pairs groups the pairs by query in order of first appearance, keeps each group's
pairs in the caller's order and cuts a group into blocks of kPairThreads = 512 (csrc/pf_pair_groups.h
PairGroups, csrc/pf_pairs_host.cpp pair_chunks), so pair j of a group is lane j % 512 of block j // 512, wave (j % 512) // 64.

Users (uid = UID0 + position; no adjacency, so an all-candidates call ranks everyone but the query):
  Q    one token in each of the T = 22 columns, 70 more in column COL_LONG, three clubs, four friends
  Q1   30 tokens in column COL_Q1 (the one-column overflow), one of Q's tokens, two clubs, one friend
  QG   Q's record plus GLOBAL_FILL tokens nobody else holds: its table is probed in global memory
  I(n) n = 0 .. 21: exactly n items against Q (n - 2 hit columns, one shared club, one shared friend),
       127 users each of I(12) and I(21) with consecutive uids and equal record length, four of the others
  variants with the club / friend field but nothing shared, without the field, and with a header alone
  OV20, OV21 (20 / 21 hit columns), MT (more than 64 shared tokens, nset = 64), UA (the same record with
  nset = 5: the wave's re-walk starts unaligned), OVQ1 (25 of Q1's tokens)
  fillers that only vary the document frequencies of Q's tokens.
A shared column of a candidate holds Q's token and a private one, with tf values that depend on the
column and on the user, and every column's df differs, so no two text terms of a pair are equal (a
column with the shared token alone would have cosine 1 whatever its tf); half of the columns have a
normaliser.  Headers cycle through completion / age 0, 1, 128, 129, 32767 and missing public / gender
/ region parts, as tests/test_gpu_qimage.py's users do.

The model classifies compositions only.  It never produces an expected score: those are the oracle's.
Run as a script, the module prints the model's census of the waves the suite's other pair calls make."""
import numpy as np

import pokec_testlib as tl

T = 22
# the kernels' limits, as their sources state them
HIT_CAP = 20                       # csrc/pf_types.h:19-22 PF_HIT_CAP / kHitCap
HIT_SLOTS = HIT_CAP + 4            # csrc/pf_types.h:28 kHitSlots = kHitCap + 4 + PF_QUEUE_EXTRA (0)
WAVE = 64                          # csrc/pf_types.h:11 kWave
QUEUE = HIT_SLOTS * WAVE // 4      # csrc/pf_kernels.hip:517 kQueue = kHitSlots * 64 / 4
PAIR_THREADS = 512                 # csrc/pf_kernels.h kPairThreads: pairs of a block
MAX_DENSE_ITEMS = HIT_CAP - 1 + 2  # a list of kHitCap hits already reads as overflowed (pf_kernels.hip:717-718)
STAGE_LIMIT = 48 * 1024            # csrc/pf_scan_host.cpp kStageLimit, csrc/pf_jobs_plan.cpp:30 kStageLimitJobs
assert T >= HIT_CAP + 2 and QUEUE == 384 and MAX_DENSE_ITEMS == 21

UID0 = 100
COL_LONG, COL_Q1 = 10, 2
N_LONG, N_Q1 = 70, 30
GLOBAL_FILL = 1700                 # above the packed big | global boundary of tools/probe/qimage --edges (1638)
N_RUN = 127                        # users of I(12) and of I(21): a whole wave of the class in any alignment
Q_CLUBS, Q_FRIENDS = [7, 11, 13], [900001, 900002, 900003, 900004]


def q_tid(t):
    return 100 + t


def _header(i):
    return dict(pub=-1 if i % 5 == 0 else i % 2, gen=-1 if i % 3 == 0 else i % 3 - 1, comp=(0, 1, 128, 129, 32767)[i % 5],
                age=(129, 0, 128, 32767, 1)[i % 5], reg=[(3 + i) % 5 if k < i % 4 else -1 for k in range(3)])


def _private(t):
    return 50 + t if t % 2 else 1000 + t   # below / above Q's token of the column


def _candidate(i, cols, club, friend, n_clubs=1, n_friends=1, plain=None):
    """cols: the columns sharing Q's token; club / friend: "shared", "other" (the field, nothing shared)
    or "none"; n_clubs / n_friends: the field's length; plain: columns with a private token only (a
    common column without a hit: its s = 0 term sits between the hit columns' terms)."""
    toks = [dict() for _ in range(T)]
    if plain is None:
        plain = [t for t in range(T) if t not in cols and (t + len(cols)) % 3 == 0]
    for t in cols:
        toks[t][q_tid(t)] = 1 + (3 * t + i) % 7
        toks[t][_private(t)] = 1 + (5 * t + 2 * i) % 11
    for t in plain:
        toks[t][_private(t)] = 1 + (5 * t + 2 * i) % 11
    for t in range(T):
        toks[t] = dict(sorted(toks[t].items()))
    u = _header(i)
    u["clubs"] = {"shared": [Q_CLUBS[i % 3]], "other": [999], "none": []}[club]
    u["friends"] = {"shared": [Q_FRIENDS[i % 4]], "other": [800000], "none": []}[friend]
    if u["clubs"]:
        u["clubs"] += [2000 + k for k in range(n_clubs - 1)]
    if u["friends"]:
        u["friends"] += [700000 + k for k in range(n_friends - 1)]
    u["toks"] = toks
    return u


def item_cols(n):
    """The hit columns of I(n): spread over the T columns, another set for every n."""
    return sorted((k * 7 + n) % T for k in range(max(n - 2, 0)))


def _class_I(n, i):
    if n >= 2:
        # the set sizes alternate from user to user (so their terms do) at a constant record length
        return _candidate(i, item_cols(n), "shared", "shared", 1 + n % 3 + i % 2, 2 + n % 2 - i % 2)
    return _candidate(i, [8] if n == 1 else [], "other", "other", 2, 1)


def _long_overflow(i, nc, nf):
    """MT / UA: Q's tokens of columns 3, COL_LONG and 17, 66 of Q's 70 further tokens of COL_LONG and
    private tokens around them: 119 token words, so the wave's re-walk takes two or three 64-word
    trips and COL_LONG's run of 77 words crosses a trip edge wherever the tokens start."""
    u = _candidate(i, [3, COL_LONG, 17], "shared", "shared", nc, nf, plain=[])
    for k in range(38):
        u["toks"][3][2000 + k] = 1 + (k + i) % 5
    for k in range(66):
        u["toks"][COL_LONG][300 + k] = 1 + (2 * k + i) % 6
    for k in range(9):
        u["toks"][COL_LONG][400 + 3 * k] = 1 + k % 3
    for t in (3, COL_LONG):
        u["toks"][t] = dict(sorted(u["toks"][t].items()))
    return u


def _query_q(i):
    u = dict(pub=1, gen=1, comp=50, age=30, reg=[3, 4, 0], clubs=list(Q_CLUBS), friends=list(Q_FRIENDS),
             toks=[{q_tid(t): 1 + (5 * t) % 9} for t in range(T)])
    for k in range(N_LONG):
        u["toks"][COL_LONG][300 + k] = 1 + k % 4
    return u


def _query_q1(i):
    toks = [dict() for _ in range(T)]
    toks[COL_Q1] = {200 + k: 1 + k % 3 for k in range(N_Q1)}
    toks[5] = {q_tid(5): 2}
    return dict(pub=0, gen=0, comp=129, age=1, reg=[4, -1, -1], clubs=[7, 21], friends=[900001], toks=toks)


def _query_qg(i):
    u = _query_q(i)
    u.update(comp=77, age=128)
    for j in range(GLOBAL_FILL):
        u["toks"][j % T][5000 + j // T] = 1 + (j * 7 + 3) % 200
    return u


def _ovq1(i):
    u = _candidate(i, [4], "shared", "other", 2, 1, plain=[0, 9])
    u["clubs"][0] = 7
    u["toks"][COL_Q1] = {200 + k: 1 + (k + i) % 5 for k in range(25)}
    u["toks"][COL_Q1][999] = 3
    return u


def _filler(j):
    u = _candidate(1000 + j, [t for t in range(T) if j % (t % 5 + 2) == 0], "other", "none", 1, 0)
    return u


# name -> (users of the class, builder(i)); i = the user's position within the class + the class's offset
CLASSES = {"Q": (1, _query_q), "Q1": (1, _query_q1), "QG": (1, _query_qg)}
for _n in range(MAX_DENSE_ITEMS + 1):
    CLASSES["I%d" % _n] = (N_RUN if _n in (12, 21) else 4, (lambda n: lambda i: _class_I(n, i + 2 * n))(_n))
CLASSES.update({
    "club_other": (2, lambda i: _candidate(i + 1, [4, 19], "other", "shared", 2, 1)),     # 3 items, sig0 clubs term
    "friend_other": (2, lambda i: _candidate(i + 2, [13], "shared", "other", 1, 3)),      # 2 items, sig0 friends term
    "no_clubs": (2, lambda i: _candidate(i + 3, [0, 6, 21], "none", "shared", 0, 2)),     # 4 items, no clubs field
    "no_friends": (2, lambda i: _candidate(i + 4, [], "shared", "none", 2, 0)),           # 1 item, no friends field
    "no_sets": (2, lambda i: _candidate(i + 6, [1, 2], "none", "none")),                  # 2 items, neither field
    "header_only": (1, lambda i: _candidate(7, [], "none", "none", plain=[])),             # 0 items, no record words
    "OV20": (3, lambda i: _candidate(i + 5, [t for t in range(T) if t not in (6, 15)], "shared", "shared", 2, 2)),
    "OV21": (3, lambda i: _candidate(i + 7, [t for t in range(T) if t != 11], "shared", "shared", 2, 2)),
    "MT": (2, lambda i: _long_overflow(i + 8, 40, 24)),
    "UA": (2, lambda i: _long_overflow(i + 9, 2, 3)),
    "OVQ1": (2, _ovq1),
    "filler": (24, _filler),
})
# what each class is planted for against Q: (items, token hits, overflowed); tests/test_pair_wave_cpu.py
# recomputes all three from the corpus arrays
EXPECT = {"I%d" % n: (n, max(n - 2, 0) if n != 1 else 1, False) for n in range(MAX_DENSE_ITEMS + 1)}
EXPECT.update({"club_other": (3, 2, False), "friend_other": (2, 1, False), "no_clubs": (4, 3, False),
               "no_friends": (1, 0, False), "no_sets": (2, 2, False), "header_only": (0, 0, False),
               "OV20": (0, 20, True), "OV21": (0, 21, True), "MT": (0, 69, True), "UA": (0, 69, True),
               "OVQ1": (2, 1, False)})
EXPECT_Q1 = {"OVQ1": (0, 25, True)}   # against Q1: one column's 25 hits


def users():
    """[(class name, instance, record)] in uid order."""
    out = []
    for name, (count, make) in CLASSES.items():
        for k in range(count):
            out.append((name, k, make(k)))
    return out


_CACHE = {}


def corpus(wide=False):
    """(tl.Corpus, {(class, instance): uid}).  wide: the twin a tf of 300 keeps out of the packed format."""
    if wide in _CACHE:
        return _CACHE[wide]
    us = users()
    if wide:
        name, k, u = us[-1]
        assert name == "filler"
        t = next(t for t in range(T) if u["toks"][t])
        u["toks"][t][_private(t)] = 300
    coff, foff, toff, clubs, friends, tid, tf = [0], [0], [0], [], [], [], []
    for _, _, u in us:
        clubs += u["clubs"]
        friends += u["friends"]
        coff.append(len(clubs))
        foff.append(len(friends))
        for t in range(T):
            tid += list(u["toks"][t].keys())
            tf += list(u["toks"][t].values())
            toff.append(len(tid))
    uid = UID0 + np.arange(len(us))
    K = tl.NUM_FIXED + T
    present, mean, sd = np.zeros(K, np.uint8), np.zeros(K, np.float32), np.zeros(K, np.float32)
    for t in range(T):
        if t % 2:
            present[tl.NUM_FIXED + t], mean[tl.NUM_FIXED + t], sd[tl.NUM_FIXED + t] = 1, 0.25 + 0.01 * t, 0.15 + 0.01 * t
    c = tl.Corpus(uid, [u["pub"] for _, _, u in us], [u["comp"] for _, _, u in us], [u["gen"] for _, _, u in us],
                  [u["age"] for _, _, u in us], [r for _, _, u in us for r in u["reg"]], coff, clubs, foff, friends, toff, tid, tf,
                  [], [0], [0], T, present, mean, sd)
    _CACHE[wide] = (c, {(name, k): int(uid[j]) for j, (name, k, _) in enumerate(us)})
    return _CACHE[wide]


def uid_of(name, k=0):
    return UID0 + _first(name) + k % CLASSES[name][0]


def _first(name):
    at = 0
    for n, (count, _) in CLASSES.items():
        if n == name:
            return at
        at += count
    raise KeyError(name)


# ------------------------------------------------------------------ what a pair's lane holds
def record(c, uid):
    """uid's rows in corpus c: (clubs, friends, [column -> {tid: tf}])."""
    if not hasattr(c, "_pw_pos"):
        c._pw_pos = c.index()
    i = c._pw_pos[int(uid)]
    toks = []
    for t in range(c.n_cols):
        a, b = int(c.tok_off[i * c.n_cols + t]), int(c.tok_off[i * c.n_cols + t + 1])
        toks.append(dict(zip(c.tok_tid[a:b].tolist(), c.tok_tf[a:b].tolist())))
    return (c.clubs[c.club_off[i]:c.club_off[i + 1]].tolist(), c.friends[c.friend_off[i]:c.friend_off[i + 1]].tolist(), toks)


def lane_of_pair(c, q_uid, b_uid, fixed=0x7F, cols=~0):
    """(items, token hits, overflowed, hit columns) of the packed K1' lane scoring (q, b) under a field
    selection, from the corpus arrays.  The walk finds every token word of b whose (column, tid) the
    query's table holds, whatever the selection (pf_kernels.hip row_step); a list that reached kHitCap
    reads as overflowed (:717-718); a dense lane makes one item per hit column of the query's selected
    columns (:503-507), one for clubs when the query has the field selected and b shares an id (:511),
    one for friends (:512); an overflowed lane makes none (:513)."""
    qc_, qf, qt = record(c, q_uid)
    bc, bf, bt = record(c, b_uid)
    hit_cols = [t for t in range(c.n_cols) if any(k in qt[t] for k in bt[t])]
    nh = sum(1 for t in range(c.n_cols) for k in bt[t] if k in qt[t])
    overflow = nh >= HIT_CAP
    ncol = sum(1 for t in hit_cols if (cols >> t) & 1)
    club = bool((fixed >> 5) & 1) and bool(qc_) and any(x in qc_ for x in bc)
    friend = bool((fixed >> 6) & 1) and bool(qf) and any(x in qf for x in bf)
    return (0 if overflow else ncol + club + friend), nh, overflow, hit_cols


# ------------------------------------------------------------------ the host model of the split
def classify(items, overflow=None, inactive=None):
    """pair_epilogue's split of one wave (csrc/pf_kernels.hip:510-535), restated: items[l] = lane l's item
    count, overflow[l] / inactive[l] its flags (such a lane contributes no items, :510-513).
      x = the wave-inclusive scan of the counts (:514-515); base = x - nit, total = x of lane 63 (:516)
      a lane with x > kQueue runs in round 1 (:521); total0 = base of the first such lane, or total when
      there is none (:522-523); total1 = total - total0 (:524)
      total1 > kQueue: the whole wave takes the per-lane epilogue (:532-535)
    Returns (kind, total0, total1), kind one of "one_round", "two_rounds", "per_lane"."""
    n = len(items)
    assert n == WAVE
    overflow = overflow if overflow is not None else [False] * n
    inactive = inactive if inactive is not None else [False] * n
    x, total0 = 0, None
    for l in range(n):
        nit = 0 if (overflow[l] or inactive[l]) else items[l]
        base = x
        x += nit
        if x > QUEUE and total0 is None:
            total0 = base
    total = x
    if total0 is None:
        return "one_round", total, 0
    total1 = total - total0
    return ("per_lane" if total1 > QUEUE else "two_rounds"), total0, total1


def waves_of(pairs):
    """The waves pf_fas_pairs makes of pairs = [(query key, b key)] (csrc/pf_pair_groups.h PairGroups: groups
    by query in order of first appearance, each group's pairs in the caller's order; pair_chunks: a
    group cut into blocks of kPairThreads; the kernel: lane i of a block scores its pair i): a list
    of (query key, [b key per active lane]) with 1 .. 64 lanes each, in block order."""
    groups = {}
    for q, b in pairs:
        groups.setdefault(q, []).append(b)
    out = []
    for q, bs in groups.items():
        for b0 in range(0, len(bs), PAIR_THREADS):
            blk = bs[b0:b0 + PAIR_THREADS]
            out += [(q, blk[w:w + WAVE]) for w in range(0, len(blk), WAVE)]
    return out


def categories(c, uid_pairs, fixed=0x7F, cols=~0):
    """[(kind, total0, total1, overflowed lanes, inactive lanes)] per wave of the call fas_pairs(a, b)
    with uid_pairs = [(a uid, b uid)] on the packed corpus c (b uid None: an inactive lane in place)."""
    out, memo = [], {}
    for q, bs in waves_of(uid_pairs):
        st = []
        for b in bs:
            if b is not None and (q, b) not in memo:
                memo[(q, b)] = lane_of_pair(c, q, b, fixed, cols)[:3]
            st.append(memo[(q, b)] if b is not None else (0, 0, False))
        pad = WAVE - len(bs)
        kind, t0, t1 = classify([s[0] for s in st] + [0] * pad, [s[2] for s in st] + [False] * pad,
                                [b is None for b in bs] + [True] * pad)
        out.append((kind, t0, t1, sum(1 for s in st if s[2]), pad + sum(1 for b in bs if b is None)))
    return out


def job_route_pairs(c, q_uid):
    """The pairs of the job pipeline's all-candidates job of q_uid (kDjAll: the recommender with topk above
    the scan kernels' bound), as K1' sees them: the gather lists every profile in idx order and leaves
    the query's own entry in place as slot -1, an inactive lane (csrc/pf_jobs.hip:148-169), and K9 cuts
    the job's region into blocks of kPairThreads (csrc/pf_jobs.hip:971-986).  b = None: that lane."""
    return [(int(q_uid), None if int(u) == int(q_uid) else int(u)) for u in sorted(c.uid.tolist())]


# ------------------------------------------------------------------ the compositions
def _w(*parts):
    """A lane list from (count, class) parts."""
    out = []
    for n, name in parts:
        out += [name] * n
    return out


def _put(lanes, at, name):
    lanes = list(lanes)
    lanes[at] = name
    return lanes


LIGHT = _w((16, "I1"), (16, "I2"), (8, "I0"), (8, "club_other"), (8, "no_sets"), (8, "I3"))   # 112 items
FALLBACK_MIX = _w((20, "I21"), (2, "OV20"), (4, "I0"), (4, "no_clubs"), (4, "no_friends"), (1, "MT"), (1, "header_only"),
                  (27, "I21"), (1, "UA"))
TWO_ROUND_OV0 = _put(_w((64, "I10")), 5, "OV21")     # an overflowed lane among the round-0 lanes
TWO_ROUND_OV1 = _put(_w((64, "I10")), 50, "OV20")    # ... among the round-1 lanes

# name -> (query key, lanes, the kinds of its waves the CPU guard asserts, in wave order)
COMPOSITIONS = {
    # one round
    "full_384": ("Q", _w((64, "I6")), ["one_round"]),
    "385_lane63": ("Q", _put(_w((64, "I6")), 63, "I7"), ["two_rounds"]),
    "385_lane0": ("Q", _put(_w((64, "I6")), 0, "I7"), ["two_rounds"]),
    "385_lane31": ("Q", _put(_w((64, "I6")), 31, "I7"), ["two_rounds"]),
    "light": ("Q", LIGHT, ["one_round"]),
    # two rounds
    "two_640": ("Q", _w((64, "I10")), ["two_rounds"]),
    "two_full_768": ("Q", _w((64, "I12")), ["two_rounds"]),
    # zero items at the split: the I0 lane ends exactly at the queue's end (x = 384, round 0); is the
    # lane after the first round-1 lane; follows a round-1 start that is not at a lane multiple
    "zero_at_split": ("Q", _w((32, "I12"), (1, "I0"), (31, "I7")), ["two_rounds"]),
    "zero_after_split": ("Q", _w((32, "I12"), (1, "I7"), (1, "I0"), (30, "I7")), ["two_rounds"]),
    "zero_after_odd_split": ("Q", _w((31, "I12"), (1, "I13"), (1, "I0"), (31, "I9")), ["two_rounds"]),
    # per-lane fallback
    "fallback_385_second": ("Q", _put(_w((64, "I12")), 40, "I13"), ["per_lane"]),
    "fallback_385_first": ("Q", _put(_w((64, "I12")), 9, "I13"), ["per_lane"]),
    "fallback_all21": ("Q", _w((64, "I21")), ["per_lane"]),
    "fallback_mix": ("Q", FALLBACK_MIX, ["per_lane"]),
    "fallback_partial": ("Q", _w((40, "I21")), ["per_lane"]),
    # overflowed lanes in dense waves
    "ov_lane0": ("Q", _put(LIGHT, 0, "OV20"), ["one_round"]),
    "ov_lane63": ("Q", _put(LIGHT, 63, "OV21"), ["one_round"]),
    "ov_three": ("Q", _put(_put(_put(LIGHT, 3, "OV20"), 31, "OV21"), 32, "OV20"), ["one_round"]),
    "ov_all64": ("Q", _w((22, "OV20"), (22, "OV21"), (10, "MT"), (10, "UA")), ["one_round"]),
    "ov_round0_of_two": ("Q", TWO_ROUND_OV0, ["two_rounds"]),
    "ov_round1_of_two": ("Q", TWO_ROUND_OV1, ["two_rounds"]),
    "ov_multi_trip": ("Q", _put(_put(LIGHT, 7, "MT"), 40, "MT"), ["one_round"]),
    "ov_unaligned": ("Q", _put(_put(LIGHT, 8, "UA"), 63, "UA"), ["one_round"]),
    "ov_q1_column": ("Q1", _put(_put(LIGHT, 1, "OVQ1"), 62, "OVQ1"), ["one_round"]),
    # position in the block: heavy waves 0, 3 and 7 of a 512-pair block, light ones between
    "block_two_rounds_037": ("Q", _w((64, "I12")) + LIGHT * 2 + TWO_ROUND_OV1 + LIGHT * 3 + _w((64, "I12")),
                             ["two_rounds", "one_round", "one_round", "two_rounds", "one_round", "one_round", "one_round", "two_rounds"]),
    "block_fallback_037": ("Q", _w((64, "I21")) + LIGHT * 2 + FALLBACK_MIX + LIGHT * 3 + _w((64, "I21")),
                           ["per_lane", "one_round", "one_round", "per_lane", "one_round", "one_round", "one_round", "per_lane"]),
    "group_513": ("Q", (_w((64, "I12")) + LIGHT + _w((64, "I21")) + LIGHT) * 2 + ["I21"],
                  ["two_rounds", "one_round", "per_lane", "one_round"] * 2 + ["one_round"]),
    "group_1025": ("Q", (_w((64, "I21")) + LIGHT + TWO_ROUND_OV0 + LIGHT) * 4 + ["OV21"],
                   ["per_lane", "one_round", "two_rounds", "one_round"] * 4 + ["one_round"]),
}
HEAVY_TWO, HEAVY_FALLBACK = "two_full_768", "fallback_mix"
OVERFLOW_COMPOSITIONS = [n for n in COMPOSITIONS if n.startswith("ov_")]
# selections (fixed mask, column mask): the composition's kind without and with it
SELECTED = {
    "select_two_to_one": ("two_640", 0x7F, sum(1 << t for t in range(0, T, 2)), "two_rounds", "one_round"),
    "select_per_lane_to_dense": ("fallback_all21", 0x7F & ~(1 << 5) & ~(1 << 6), sum(1 << t for t in range(T) if t % 3), "per_lane", "two_rounds"),
}


def lanes_uids(lanes, q="Q"):
    """[(a uid, b uid)] of a lane list: lane l takes instance l of its class (the headers and tf values
    then differ from lane to lane), instance l % count where the class has fewer."""
    return [(uid_of(q), uid_of(name, l)) for l, name in enumerate(lanes)]


def interleaved():
    """Two groups in one call, their pairs alternating in the input arrays (so the results scatter back
    through where[]): Q's two-round wave with an overflowed lane and Q1's wave with its one-column overflow."""
    a = lanes_uids(TWO_ROUND_OV1, "Q")
    b = lanes_uids(COMPOSITIONS["ov_q1_column"][1], "Q1")
    return [p for ab in zip(a, b) for p in ab]


# ------------------------------------------------------------------ a census of other pair calls
def census(c, uid_pairs):
    """{kind: waves} plus "with_overflow", "partial_wave", "waves", "max_items" (a wave's total) and
    "items_per_lane" for the call fas_pairs(a, b) on a packed corpus c: what the model says of the waves
    an existing test's pairs make.  `python tests/pair_wave_corpus.py` prints it for the golden pair
    files and the random pair batches of the earlier tests."""
    cat = categories(c, uid_pairs)
    out = {k: sum(1 for x in cat if x[0] == k) for k in ("one_round", "two_rounds", "per_lane")}
    out["with_overflow"] = sum(1 for x in cat if x[3])
    out["partial_wave"] = sum(1 for x in cat if x[4])
    out["waves"] = len(cat)
    out["max_items"] = max((x[1] + x[2] for x in cat), default=0)
    out["items_per_lane"] = round(sum(x[1] + x[2] for x in cat) / max(1, sum(WAVE - x[4] for x in cat)), 2)
    return out


def is_packed(c):
    """csrc/pf_store.cpp:270-276: 0 <= tf <= 255 and club / friend ids below 2^30 (column ranks never
    reach 2^18 - 1 on the test corpora)."""
    return bool(len(c.tok_tf) == 0 or (c.tok_tf.min() >= 0 and c.tok_tf.max() <= 255)) and \
        bool(len(c.clubs) == 0 or c.clubs.max() < 2**30) and bool(len(c.friends) == 0 or c.friends.max() < 2**30)


def _main():
    import edge_corpus as ec
    rows = []
    for name in ("A", "B", "E"):
        c = tl.golden_corpus(name)
        a, b, _ = tl.golden_pairs(name)
        rows.append(("golden %s pairs.txt (%d pairs)" % (name, len(a)), c, list(zip(a.tolist(), b.tolist()))))
    E = tl.golden_corpus("E")
    rows.append(("E planted + hit pairs", E, [(ec.uid_of(x), ec.uid_of(y)) for x, y in
                                              ec.planted_pairs() + [(p, q) for p, q, _ in ec.HIT_PAIRS] + [(q, p) for p, q, _ in ec.HIT_PAIRS]]))
    for q in (1, ec.HIT_Q_SPREAD, ec.EXCL_CLONES_Q, 515):   # the users of the selection tests' topk = 100 calls
        rows.append(("E all-candidates job of idx %d" % q, E, job_route_pairs(E, ec.uid_of(q))))
    for n, seed, npairs, rs in ((3000, 3, 4096, 0), (20000, 77, 20000, 11)):   # smoke(), gpu_variant_check.py
        sc = tl.synth.Corpus(n_users=n, seed=seed, edge_cases=1)
        c = tl.corpus_from_desc(sc.desc_ptr())
        rng = np.random.default_rng(rs)
        if rs == 11:
            rng.integers(1, n + 1, 6), rng.integers(1, n + 1, 16)   # the draws that precede the pairs there
        a, b = rng.integers(1, n + 1, npairs), rng.integers(1, n + 1, npairs)
        rows.append(("synth n=%d seed=%d, %d random pairs" % (n, seed, npairs), c, list(zip(a.tolist(), b.tolist()))))
    for title, c, pairs in rows:
        pos = c.index()
        pairs = [(a, b) for a, b in pairs if a in pos and (b is None or b in pos)]
        print("%-44s packed=%d %s" % (title, is_packed(c), census(c, pairs)))
    c, _ = corpus()
    pairs = [p for q, lanes, _ in COMPOSITIONS.values() for p in lanes_uids(lanes, q)]
    print("%-44s packed=%d %s" % ("the planted compositions (one call each)", is_packed(c),
                                  {k: sum(census(c, lanes_uids(l, q))[k] for q, l, _ in COMPOSITIONS.values())
                                   for k in ("one_round", "two_rounds", "per_lane", "with_overflow", "partial_wave", "waves")}))


if __name__ == "__main__":
    _main()
