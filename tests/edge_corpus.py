"""Edge corpus "E": a small deterministic corpus whose values sit on the branches the scan and
pair kernels take and that the seeded generator (tools/pokec_synth.cpp) never reaches: columns
split over K5 rounds (by token count and by entry count), runs at kItemRunMax, hit lists at
kHitCap / kHitSlots, values past the sigmoid tables, the encoding limits of the packed store,
hundreds of tied scores over block edges, sparse unordered uids.

Pure integer arithmetic (closed formulas, no random module, no numpy.random), so the files are
byte-identical anywhere.  write_reference_files() writes the reference's on-disk layout; tests
parse it back with pokec_testlib.read_reference_dir, so the reference, the oracle and the engine
see one corpus.  Every planted case is a named constant or table below; tests/test_edge_corpus_cpu.py
asserts each of them on the parsed corpus.

Users are laid out by idx, the rank of their uid (the engine's candidate order); K5 scores blocks
of 512 consecutive idx.
"""
import os

N_USERS = 1400
N_COLS = 48
BLOCK = 512                      # K5 block (pf_types.h kBlockCands)
DENSE = (512, 1024)              # idx range of the dense block: one whole K5 block
UID_MAX = 2_000_000_000          # largest uid (idx N_USERS - 1)
COLS = ["c%02d" % t for t in range(N_COLS)]


def uid_of(i):
    """Sparse ascending uids: steps of 7..11, the last user far away."""
    return UID_MAX if i == N_USERS - 1 else 1000 + 7 * i + (i * i) % 5


def mix(i, salt):
    """Closed-form scrambler (integer only)."""
    x = (i * 2654435761 + salt * 40503 + 12345) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 2246822519) & 0xFFFFFFFF
    x ^= x >> 13
    return x


# ---------------------------------------------------------------- columns
COL_D1, COL_D4, COL_D5, COL_D200 = 2, 3, 4, 5   # dense-block columns (entry-count splits)
COL_L, COL_L2 = 8, 9                           # long query columns (token-count splits), adjacent
COL_HC = 12                                    # hit-list column (one column, many tokens)
COLS_HS = list(range(20, 45))                  # hit-list spread: one token in each of 25 columns
COL_TF0 = 14                                   # the tf = 0 only user's column
D_TOKENS = {COL_D1: [9001], COL_D4: list(range(9100, 9104)), COL_D5: list(range(9200, 9205)),
            COL_D200: list(range(9300, 9500))}
L_TOKENS = list(range(7000, 7200))
L2_TOKENS = list(range(7500, 7600))
HC_TOKENS = list(range(6000, 6025))
HS_TOKEN = 5000                                # + column

# normalisers: z mode of each split column's own term (refcpu z_of / recommender_similarity.cpp)
NORM_ABSENT = [COL_D5, COL_L2, 17, 33]         # no line in column_normalizers.csv
NORM_SD0 = [COL_D200, 21]                      # present with sd = 0
# COL_D4, COL_D1, COL_L: present with sd > 0
SPLIT_Z_MODES = {"absent": COL_D5, "present": COL_D4, "sd0": COL_D200}
FIXED_NORMS = {"public": ("0.5", "0.25"), "completion": ("0.75", "0.125"), "age": ("0.8", "0.1"),
               "clubs": ("0.05", "0"), "friends": ("0.03", "0.0625")}   # gender, region absent

# ---------------------------------------------------------------- planted users (idx)
Q_LONG = {64: 1, 65: 2, 128: 3, 129: 4, 200: 5}     # tokens of COL_L -> query idx
Q_TWO_LONG = 6                                     # 100 tokens in COL_L and 100 in COL_L2
P_TWO_LONG = 7                                     # its partner: 50 and 70 of them
P_200 = 8                                          # shares all 200 COL_L tokens with Q_LONG[200]
RUN_Q = Q_LONG[64]
RUNS = {31: 10, 32: 11, 33: 12, 64: 13}             # shared tokens of COL_L with RUN_Q -> candidate idx
HIT_Q_ONE, HIT_Q_SPREAD = 15, 16                    # 25 tokens in COL_HC / one token in 25 columns
HITS_ONE = {19: 17, 20: 18, 21: 19, 24: 20, 25: 21}  # shared with HIT_Q_ONE -> idx
HITS_SPREAD = {19: 22, 20: 23, 21: 24, 24: 25, 25: 26}
HIT_PAIRS = ([(HIT_Q_ONE, i, k) for k, i in HITS_ONE.items()] +
             [(HIT_Q_SPREAD, i, k) for k, i in HITS_SPREAD.items()] + [(Q_LONG[200], P_200, 200)])
VALS = [1, 127, 128, 129, 200, 32767]
VAL_USERS = {30 + j: (VALS[j], VALS[(j + 1) % 6]) for j in range(6)}   # idx -> (age, completion)
VAL_USERS.update({36 + j: (VALS[j], VALS[j]) for j in range(6)})
COMP_ZERO, COMP_MINUS1 = 42, 43
FLAG_USERS = {44: (2, 77), 45: (77, 2), 46: (2, 2)}                    # idx -> (public, gender)
REGION_USERS = {47: (2_000_000_000, 2_000_000_000, 2_000_000_000), 48: (5, 5, -1), 49: (-1, -1, 7),
                50: (2_000_000_000, 5, 5), 51: (-1, -1, -1)}
EMPTY_USER = 52                                    # every field missing
TF0_USER = 53                                      # its only text: one token with tf = 0
ID_TOP = 2**30 - 1                                 # largest id of the packed set store
CLUB_X, CLUB_Y, FRIEND_X, FRIEND_Y = 700001, 700002, 800001, 800002
SET_USERS = {55: ("clubs", CLUB_X, 2), 56: ("clubs", CLUB_Y, 255), 57: ("friends", FRIEND_X, 2),
             58: ("friends", FRIEND_Y, 255)}          # idx -> (field, id, repeats)
SET_PARTNER = 59                                   # holds all four ids and ID_TOP in both fields
SET_TOP = 60                                       # holds ID_TOP in both fields
DUP_LINE_USER = 61                                 # its uid has an earlier line in the file; the later wins
EXCL_RUN_Q = 62                                    # adjacency row = idx 500..530 (crosses the 512 edge)
EXCL_RUN = (500, 531)
EXCL_CLONES_Q = 466                                # a clone whose adjacency row names most clones
N_PLANTED = 64                                     # idx below this are planted or spare

CLONE_RANGE = (440, 1192)                          # clones: idx in the range with idx % 5 != 0


def is_clone(i):
    return CLONE_RANGE[0] <= i < CLONE_RANGE[1] and i % 5 != 0


CLONES = [i for i in range(N_USERS) if is_clone(i)]
CLONE_QUERIES = [441, 511, 513, 766, 1023, 1026, 1191]
EXCL_CLONES_KEPT = [i for k, i in enumerate(CLONES) if k % 8 == 3]   # clones EXCL_CLONES_Q does not exclude

PLANTED_QUERIES = (sorted(Q_LONG.values()) + [Q_TWO_LONG, P_200, HIT_Q_ONE, HIT_Q_SPREAD] + sorted(VAL_USERS) +
                   [COMP_ZERO, COMP_MINUS1] + sorted(FLAG_USERS) + sorted(REGION_USERS) +
                   [EMPTY_USER, TF0_USER] + sorted(SET_USERS) + [SET_PARTNER, DUP_LINE_USER, EXCL_RUN_Q,
                                                                 EXCL_CLONES_Q, 515, 520, 1020] + CLONE_QUERIES)


def planted_pairs():
    """(a idx, b idx) pairs appended to the golden pair list, each in both orders."""
    pairs = [(q, c) for q, c, _ in HIT_PAIRS]
    pairs += [(RUN_Q, c) for c in RUNS.values()] + [(Q_TWO_LONG, P_TWO_LONG)]
    lq = sorted(Q_LONG.values())
    pairs += [(a, b) for a in lq for b in lq if a < b]
    v = sorted(VAL_USERS)
    pairs += [(a, b) for a in v for b in v if a <= b]
    pairs += [(a, b) for a in v for b in (COMP_ZERO, COMP_MINUS1, EMPTY_USER, 515)]
    f = sorted(FLAG_USERS) + sorted(REGION_USERS)
    pairs += [(a, b) for a in f for b in f if a <= b]
    s = sorted(SET_USERS) + [SET_PARTNER, SET_TOP]
    pairs += [(a, b) for a in s for b in s if a <= b]
    pairs += [(EMPTY_USER, b) for b in (EMPTY_USER, TF0_USER, 441, 515)] + [(TF0_USER, b) for b in (TF0_USER, 70, 441)]
    d = [515, 520, 525, 1020, 441, 766, 1191, Q_LONG[200]]
    pairs += [(a, b) for a in d for b in d if a <= b]
    return pairs + [(b, a) for a, b in pairs if a != b]


# ---------------------------------------------------------------- profiles
def _blank():
    return {"pub": None, "comp": None, "gen": None, "age": None, "reg": (-1, -1, -1), "clubs": [], "friends": [],
            "toks": {}}


def _tf(i, k):
    return 1 + mix(i, k) % 5


def _background(i):
    """Ordinary user: a few tokens in a few columns, some clubs / friends."""
    p = _blank()
    p["pub"], p["gen"] = mix(i, 1) % 2, mix(i, 2) % 2
    if mix(i, 3) % 11 == 0:
        p["gen"] = None
    p["comp"] = 1 + mix(i, 4) % 100
    p["age"] = 14 + mix(i, 5) % 60 if mix(i, 6) % 9 else None
    p["reg"] = (1 + mix(i, 7) % 4, 1 + mix(i, 8) % 12, 1 + mix(i, 9) % 40)
    p["clubs"] = [1 + mix(i, 20 + k) % 60 for k in range(mix(i, 10) % 5)]
    p["friends"] = [uid_of(mix(i, 30 + k) % (N_USERS - 1)) for k in range(mix(i, 11) % 6)]
    for k in range(3 + mix(i, 12) % 6):
        t = mix(i, 40 + k) % N_COLS
        m = p["toks"].setdefault(t, {})
        for j in range(1 + mix(i, 60 + k) % 4):
            m[1 + mix(i, 80 + 7 * k + j) % 30] = 1 + mix(i, 120 + 7 * k + j) % 3
    return p


def _dense_tokens(p, i, clone):
    """The dense block's columns: every member holds the same tokens; tf cycles over 0..255
    (a clone's tf is fixed)."""
    for t, toks in D_TOKENS.items():
        p["toks"][t] = {tok: (3 if clone else (i * 7 + k * 13 + t) % 256) for k, tok in enumerate(toks)}


def _clone():
    p = _blank()
    p["pub"], p["gen"], p["comp"], p["age"], p["reg"] = 1, 0, 88, 129, (3, 9, 27)
    p["clubs"] = [11, 12, 12, 13]
    p["friends"] = [uid_of(70), uid_of(71), 999]
    _dense_tokens(p, 0, True)
    p["toks"][7] = {3: 2, 4: 1}
    return p


def _base(i):
    """Plain fixed fields for a planted user, so that only its planted part varies."""
    p = _blank()
    p["pub"], p["gen"], p["comp"], p["age"], p["reg"] = i % 2, (i // 2) % 2, 50 + i % 40, 20 + i % 30, (2, 4, 8 + i % 3)
    return p


def profile(i):
    """Profile of the user at idx i."""
    if is_clone(i):
        return _clone()
    if DENSE[0] <= i < DENSE[1]:
        p = _background(i)
        for t in D_TOKENS:
            p["toks"].pop(t, None)
        _dense_tokens(p, i, False)
        if i % 3 == 0:
            p["age"], p["comp"] = VALS[(i // 3) % 6], VALS[(i // 15) % 6]
        return p
    if i >= N_PLANTED or i in (0, 9, 14, 27, 28, 29, 54, 63):
        p = _background(i)
        for t in list(D_TOKENS) + [COL_L, COL_L2]:      # these columns stay sparse outside the planted users
            if i % 16 != 7:
                p["toks"].pop(t, None)
        return p
    p = _base(i)
    for n, q in Q_LONG.items():
        if i == q:
            p["toks"][COL_L] = {tok: _tf(i, k) for k, tok in enumerate(L_TOKENS[:n])}
    if i == Q_LONG[200]:
        _dense_tokens(p, 5, False)                 # a block-0 query on every dense column
        p["toks"][COL_D200] = {tok: 1 + (k * 5) % 255 for k, tok in enumerate(D_TOKENS[COL_D200])}
    if i == Q_TWO_LONG:
        p["toks"][COL_L] = {tok: _tf(i, k) for k, tok in enumerate(L_TOKENS[:100])}
        p["toks"][COL_L2] = {tok: _tf(i, 300 + k) for k, tok in enumerate(L2_TOKENS)}
    if i == P_TWO_LONG:
        p["toks"][COL_L] = {tok: _tf(i, k) for k, tok in enumerate(L_TOKENS[:50])}
        p["toks"][COL_L2] = {tok: _tf(i, 300 + k) for k, tok in enumerate(L2_TOKENS[:70])}
    if i == P_200:
        p["toks"][COL_L] = {tok: 1 + (k * 11) % 255 for k, tok in enumerate(L_TOKENS)}
    for n, c in RUNS.items():
        if i == c:
            p["toks"][COL_L] = {tok: _tf(i, k) for k, tok in enumerate(L_TOKENS[:n])}
    if i == HIT_Q_ONE:
        p["toks"][COL_HC] = {tok: _tf(i, k) for k, tok in enumerate(HC_TOKENS)}
    for n, c in HITS_ONE.items():
        if i == c:
            p["toks"][COL_HC] = {tok: _tf(i, k) for k, tok in enumerate(HC_TOKENS[:n])}
    if i == HIT_Q_SPREAD:
        for t in COLS_HS:
            p["toks"][t] = {HS_TOKEN + t: _tf(i, t)}
    for n, c in HITS_SPREAD.items():
        if i == c:
            for t in COLS_HS[:n]:
                p["toks"][t] = {HS_TOKEN + t: _tf(i, t)}
    if i in VAL_USERS:
        p["age"], p["comp"] = VAL_USERS[i]
    if i == COMP_ZERO:
        p["comp"] = 0
    if i == COMP_MINUS1:
        p["comp"] = -1
    if i in FLAG_USERS:
        p["pub"], p["gen"] = FLAG_USERS[i]
    if i in REGION_USERS:
        p["reg"] = REGION_USERS[i]
    if i == EMPTY_USER:
        return _blank()
    if i == TF0_USER:
        p["toks"][COL_TF0] = {17: 0}
    if i in SET_USERS:
        field, x, rep = SET_USERS[i]
        p[field] = [5, x] + [x] * (rep - 1) + [6]
    if i == SET_PARTNER:
        p["clubs"] = [CLUB_X, CLUB_Y, ID_TOP, 6]
        p["friends"] = [FRIEND_X, FRIEND_Y, ID_TOP, ID_TOP]
    if i == SET_TOP:
        p["clubs"] = [ID_TOP, ID_TOP - 1]
        p["friends"] = [ID_TOP]
    if i == DUP_LINE_USER:
        p["toks"][COL_HC] = {HC_TOKENS[0]: 4, HC_TOKENS[3]: 1}
        p["clubs"] = [5, 6]
    if i == EXCL_RUN_Q:
        _dense_tokens(p, 62, False)
    return p


def adjacency(i):
    """adj_list row of the user at idx i (uids), or None for no row."""
    if i == EXCL_RUN_Q:
        return [uid_of(j) for j in range(*EXCL_RUN)]
    if i == EXCL_CLONES_Q:
        kept = set(EXCL_CLONES_KEPT)
        return [uid_of(j) for j in CLONES if j not in kept and j != i]
    if i == EMPTY_USER or i % 29 == 13:
        return None
    row = [uid_of((i * 3 + 1) % N_USERS), uid_of((i * 7 + 2) % N_USERS), uid_of((i + 1) % N_USERS)]
    row += [uid_of(mix(i, 200 + k) % N_USERS) for k in range(mix(i, 13) % 7)]
    if i % 31 == 4:
        row += [123456789, row[0]]                 # a uid without a profile, a duplicate
    return row


# ---------------------------------------------------------------- files
def _field(v):
    return "" if v is None else str(v)


def _line(uid, p):
    reg = ";".join("" if r < 0 else str(r) for r in p["reg"])
    out = [str(uid), _field(p["pub"]), _field(p["comp"]), _field(p["gen"]), reg, _field(p["age"]),
           ";".join(str(c) for c in p["clubs"]), ";".join(str(f) for f in p["friends"])]
    for t in range(N_COLS):
        out.append(";".join("%d:%d" % kv for kv in p["toks"].get(t, {}).items()))
    return ",".join(out)


def file_order():
    """idx in file order: not ascending (a stride coprime to N_USERS)."""
    return [(i * 577 + 300) % N_USERS for i in range(N_USERS)]


def write_reference_files(root, n_first=None):
    """data/ + config/ as the reference reads them.  n_first: only the users of idx < n_first
    (adjacency rows of other uids dropped; neighbours outside the slice stay, as unknown uids)."""
    n = N_USERS if n_first is None else n_first
    os.makedirs(os.path.join(root, "data"), exist_ok=True)
    os.makedirs(os.path.join(root, "config"), exist_ok=True)
    with open(os.path.join(root, "config", "text_columns.txt"), "w") as f:
        f.write("".join(c + "\n" for c in COLS))
    with open(os.path.join(root, "data", "users_encoded.csv"), "w") as f:
        f.write("user_id,public,completion_percentage,gender,region,age,clubs,friends" +
                "".join(",%s_tokens" % c for c in COLS) + "\n")
        for pos, i in enumerate(file_order()):
            if pos == 40 and DUP_LINE_USER < n:     # an earlier line of DUP_LINE_USER's uid: every field is replaced
                junk = _background(900)
                junk["clubs"] = [CLUB_Y] * 256
                junk["age"] = 40000
                f.write(_line(uid_of(DUP_LINE_USER), junk) + "\n")
            if i < n:
                f.write(_line(uid_of(i), profile(i)) + "\n")
    with open(os.path.join(root, "data", "adjacency.csv"), "w") as f:
        for i in reversed(range(n)):
            row = adjacency(i)
            if row is not None:
                f.write(",".join(str(x) for x in [uid_of(i)] + row) + "\n")
    with open(os.path.join(root, "data", "median_age.txt"), "w") as f:
        f.write("0\n")                                  # a missing age stays missing
    with open(os.path.join(root, "data", "column_normalizers.csv"), "w") as f:
        f.write("column,mean,stddev\n")
        for k, (m, s) in FIXED_NORMS.items():
            f.write("%s,%s,%s\n" % (k, m, s))
        for t, c in enumerate(COLS):
            if t in NORM_ABSENT:
                continue
            sd = "0" if t in NORM_SD0 else ["0.125", "0.25", "0.1875"][t % 3]
            f.write("%s,%s,%s\n" % (c, ["0.0625", "0.125", "0.03125", "0.25"][t % 4], sd))
    with open(os.path.join(root, "data", "tokens.csv"), "w") as f:
        f.write("column,token,tid,df\n")
    with open(os.path.join(root, "data", "clubs_map.csv"), "w") as f:
        f.write("club_id,slug,title\n")
    # the planted queries and pairs for the golden harness (oracle/ref_fixture.cpp)
    if n_first is None:
        with open(os.path.join(root, "queries.txt"), "w") as f:
            f.write("".join("%d\n" % uid_of(i) for i in PLANTED_QUERIES))
        with open(os.path.join(root, "pairs_extra.txt"), "w") as f:
            f.write("".join("%d %d\n" % (uid_of(a), uid_of(b)) for a, b in planted_pairs()))
    return root
