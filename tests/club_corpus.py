"""Clubs by interest (include/pokec_fas.h "Clubs by interest"): the definition restated in Python, and
the cases the tests share.  Nothing here runs the engine.

The expected list of a case is built from a whole ranking (the oracle's, cut to the filter and the
window by gpu_scan_window_check.cut) and the corpus's club lists: per club a Python float (a double)
takes the neighbours' scores in rank order, a neighbour scoring <= 0 is skipped, a club counts as often
as it is listed, and the sum is cast with np.float32.  The list is (score desc, club id asc).

The edge corpus E already holds every category the checks need (guard_facts asserts each one on the
oracle alone, and test_club_interest_cpu fails when one goes missing), so nothing is planted: E's
ordinary users draw 0 to 4 clubs from 60 with repeats, its 601 identical users share theirs, EMPTY_USER
scores 0.0 against everybody, and the clone 441 holds the clubs its nearest neighbours would put on top."""
import numpy as np

import edge_corpus as ec

f32 = np.float32
# the collect test's queries (gpu_scan_window_check.Q_IDX)
Q_IDX = (441, 1, 30, ec.EMPTY_USER, ec.EXCL_CLONES_Q)
NEIGHBOURS = (1, 10, 64, 65, 0)   # 0: the whole window
OWN_Q = 441                       # a clone: the clubs it shares with its 599 nearest neighbours would lead its list


def club_rows(c):
    """Per profile index: its club ids in profile order (duplicates kept)."""
    return [[int(x) for x in c.clubs[c.club_off[i]:c.club_off[i + 1]]] for i in range(c.n_users)]


def own_clubs(c, rows, uids):
    """The union of the stored users' clubs (unknown uids dropped)."""
    pos = c.index()
    own = set()
    for u in uids:
        if int(u) in pos:
            own.update(rows[pos[int(u)]])
    return own


def expect(c, rows, rank, own, neighbours=0, topk=10, keep_own=False, cap=1 << 20, detail=False):
    """(club ids, float32 scores, info) of the definition for the window's ranking `rank` = (ids, scores).
    detail: also the per-club contribution counts."""
    ids, sc = np.asarray(rank[0]), np.asarray(rank[1], np.float32)
    total = len(ids)
    info = {"total": total, "used": 0, "contributions": 0, "clubs": 0}
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float32), info)
    if total == 0 or total > cap or topk == 0:
        if topk == 0:
            info["total"] = 0   # topk = 0 scans nothing
        return empty + ({},) if detail else empty
    used = min(neighbours, total) if neighbours > 0 else total
    pos = c.index()
    acc, cnt, adds = {}, {}, 0
    for u, s in zip(ids[:used], sc[:used]):
        w = float(s)
        if w <= 0.0:
            continue
        for club in rows[pos[int(u)]]:
            if club in own and not keep_own:
                continue
            acc[club] = acc.get(club, 0.0) + w
            cnt[club] = cnt.get(club, 0) + 1
            adds += 1
    items = sorted(((f32(a), club) for club, a in acc.items()), key=lambda t: (-float(t[0]), t[1]))
    info.update(used=used, contributions=adds, clubs=len(items))
    out = (np.array([t[1] for t in items[:topk]], np.int32), np.array([t[0] for t in items[:topk]], np.float32), info)
    return out + (cnt,) if detail else out


def floors_of(sc):
    """Floors that leave nobody, the head of the ranking, ten, the 0.125 crowd: as float32 values."""
    sc = np.asarray(sc, np.float32)
    fl = [np.nextafter(sc[0], f32(np.inf)), sc[0], f32(0.125)]
    if len(sc) > 9:
        fl.append(sc[9])
    return fl


def same(got, want):
    """ids, float bits and info equal."""
    return (list(got[0]) == list(want[0]) and
            np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)) and
            dict(got[2]) == dict(want[2]))


def guard_facts(c, ranking, cut, window):
    """What E's queries contain, from the oracle alone.  ranking(uid) -> (ids, scores, idx); cut and
    window are gpu_scan_window_check.cut and ScanWindow.make.  Returns a dict of counts."""
    rows = club_rows(c)
    facts = {"tie_pairs": 0, "runs_33": 0, "runs_1": 0, "dup_neighbours": 0, "clubless_neighbours": 0, "zero_neighbours": 0,
             "own_in_top10": 0, "cut_sizes": set()}
    for i in Q_IDX:
        u = ec.uid_of(i)
        ids, sc, idx = ranking(u)
        own = own_clubs(c, rows, [u])
        facts["dup_neighbours"] += sum(1 for x in idx if len(set(rows[x])) < len(rows[x]))
        facts["clubless_neighbours"] += sum(1 for x in idx if not rows[x])
        facts["zero_neighbours"] += int((sc == 0.0).sum())
        for m in NEIGHBOURS:
            gi, gs, info, cnt = expect(c, rows, (ids, sc), own, m, topk=1 << 20, detail=True)
            facts["tie_pairs"] += int((gs[1:].view(np.uint32) == gs[:-1].view(np.uint32)).sum())
            facts["runs_33"] += sum(1 for v in cnt.values() if v >= 33)
            facts["runs_1"] += sum(1 for v in cnt.values() if v == 1)
        for fl in floors_of(sc):
            facts["cut_sizes"].add(len(cut((ids, sc), window(min_score=fl))[0]))
        if i == OWN_Q:
            kept = expect(c, rows, (ids, sc), own, 0, topk=10, keep_own=True)[0]
            left = expect(c, rows, (ids, sc), own, 0, topk=10)[0]
            facts["own_in_top10"] = len(own & set(int(x) for x in kept))
            facts["own_left_out"] = len(own & set(int(x) for x in left)) == 0
    return facts
