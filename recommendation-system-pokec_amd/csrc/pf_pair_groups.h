// pf_pair_groups.h — pairs (A, B) grouped by their A side for the pair kernels (pf_pairs_host.cpp): the
// groups in order of first appearance, a group's pairs in the caller's order, and where each pair's
// result goes.  That order decides the waves the pair kernel sees (tests/pair_wave_corpus.py models
// it).  Plain C++ with no HIP include, so the CPU test (tests/cpp/pair_groups_check.cpp) compiles it
// with g++.
#pragma once
#include <stdint.h>

#include <unordered_map>
#include <utility>
#include <vector>

namespace pf {

struct PairGroups {
    std::vector<int32_t> qidx;                // group g's A side (a corpus index, or 0 for a by-value profile)
    std::vector<std::vector<int32_t>> slots;  // group g's B sides, as store slots
    std::vector<std::vector<int64_t>> dest;   // the caller's position of each of them
    // per_pair (the score calls: one float per pair, random queries make a group of nearly every pair):
    // dest stays empty, so a group costs no allocation of its own, and add_uids records
    // where[i - i0] = (group, position) of pair i instead, (-1, -1) for a pair in no group
    std::vector<std::pair<int32_t, int32_t>> where;

    explicit PairGroups(bool per_pair = false) : per_pair_(per_pair) {}

    // returns the pair's (group, position)
    std::pair<int32_t, int32_t> add(int32_t ia, int32_t slot, int64_t to) {
        auto it = group_.find(ia);
        if (it == group_.end()) {
            it = group_.emplace(ia, (int32_t)qidx.size()).first;
            qidx.push_back(ia);
            slots.emplace_back();
            if (!per_pair_) dest.emplace_back();
        }
        slots[it->second].push_back(slot);
        if (!per_pair_) dest[it->second].push_back(to);
        return {it->second, (int32_t)slots[it->second].size() - 1};
    }
    // Pairs (a[i], b[i]), i in [i0, i1), by uid: idx_of(uid) is the corpus index (< 0: unknown) and
    // slot_of(idx) its store slot.  a == nullptr: every pair is group 0's (one by-value profile, or
    // candidates shared by every seed of a group).  A pair with an unknown side enters no group:
    // unknown(i) is called for it.
    template <class IdxOf, class SlotOf, class Unknown>
    void add_uids(const int32_t* a, const int32_t* b, int64_t i0, int64_t i1, IdxOf idx_of, SlotOf slot_of, Unknown unknown) {
        if (per_pair_) where.assign((size_t)(i1 - i0), {-1, -1});
        for (int64_t i = i0; i < i1; ++i) {
            const int32_t ia = a ? idx_of(a[i]) : 0, ib = idx_of(b[i]);
            if (ia < 0 || ib < 0) unknown(i);
            else if (per_pair_) where[(size_t)(i - i0)] = add(ia, slot_of(ib), i);
            else add(ia, slot_of(ib), i);
        }
    }

private:
    std::unordered_map<int32_t, int32_t> group_;  // A side -> group
    bool per_pair_;
};

}  // namespace pf
