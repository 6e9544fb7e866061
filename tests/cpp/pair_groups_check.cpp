// CPU check of csrc/pf_pair_groups.h: pairs grouped by their A side keep the order of first appearance
// for the groups and the caller's order inside a group (the order the pair kernel's waves are cut from),
// every pair remembers its place in the call, and a pair with an unknown side enters no group and is
// reported to the caller instead.
#include <cstdio>
#include <utility>
#include <vector>

#include "pf_pair_groups.h"

namespace {

int bad = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
            ++bad;                                                    \
        }                                                             \
    } while (0)

// uids 100, 200, 300, ... have the corpus indices 1, 2, 3, ...; anything else is unknown
int32_t idx_of(int32_t uid) { return uid > 0 && uid % 100 == 0 ? uid / 100 : -1; }
int32_t slot_of(int32_t idx) { return 1000 + idx; }  // a store slot that is not the index

using V32 = std::vector<int32_t>;
using V64 = std::vector<int64_t>;

V64 unknown;  // the pairs reported as unknown, in order
void note(int64_t i) { unknown.push_back(i); }

}  // namespace

int main() {
    {  // no pairs
        pf::PairGroups g;
        g.add_uids(nullptr, nullptr, 0, 0, idx_of, slot_of, note);
        EXPECT(g.qidx.empty() && g.slots.empty() && g.dest.empty() && unknown.empty());
    }
    {  // every uid unknown, on either side
        const int32_t a[3] = {7, 100, 9}, b[3] = {200, 11, 13};
        pf::PairGroups g;
        g.add_uids(a, b, 0, 3, idx_of, slot_of, note);
        EXPECT(g.qidx.empty() && g.slots.empty() && g.dest.empty());
        EXPECT((unknown == V64{0, 1, 2}));
        unknown.clear();
        pf::PairGroups p;  // one group (a by-value profile): the B sides alone
        p.add_uids(nullptr, b + 1, 0, 2, idx_of, slot_of, note);
        EXPECT(p.qidx.empty() && p.slots.empty() && p.dest.empty());
        EXPECT((unknown == V64{0, 1}));
        unknown.clear();
    }
    {  // queries interleaved (a, b, a, c, b), pair 2's B side unknown
        const int32_t a[5] = {300, 100, 300, 200, 100}, b[5] = {400, 500, 77, 600, 700};
        pf::PairGroups g;
        g.add_uids(a, b, 0, 5, idx_of, slot_of, note);
        EXPECT((unknown == V64{2}));
        unknown.clear();
        EXPECT((g.qidx == V32{3, 1, 2}));  // first appearance
        EXPECT(g.slots.size() == 3 && g.dest.size() == 3);
        if (g.slots.size() == 3 && g.dest.size() == 3) {
            EXPECT((g.slots[0] == V32{1004}) && (g.dest[0] == V64{0}));  // pair 2 is in no group
            EXPECT((g.slots[1] == V32{1005, 1007}) && (g.dest[1] == V64{1, 4}));  // caller order
            EXPECT((g.slots[2] == V32{1006}) && (g.dest[2] == V64{3}));
        }
        size_t pairs = 0;
        for (const auto& s : g.slots) pairs += s.size();
        EXPECT(pairs == 4);
        // the same B sides as one group, from position 1 on: group 0, positions as the caller's
        pf::PairGroups p;
        p.add_uids(nullptr, b, 1, 5, idx_of, slot_of, note);
        EXPECT((unknown == V64{2}));
        EXPECT((p.qidx == V32{0}));
        EXPECT(p.slots.size() == 1 && (p.slots[0] == V32{1005, 1006, 1007}) && (p.dest[0] == V64{1, 3, 4}));
    }
    {  // the same interleaved pairs in per-pair mode: the same groups, no per-group destinations, where[i] instead
        const int32_t a[5] = {300, 100, 300, 200, 100}, b[5] = {400, 500, 77, 600, 700};
        unknown.clear();
        pf::PairGroups g(true);
        g.add_uids(a, b, 0, 5, idx_of, slot_of, note);
        EXPECT((unknown == V64{2}) && g.dest.empty());
        EXPECT((g.qidx == V32{3, 1, 2}) && g.slots.size() == 3);
        const std::vector<std::pair<int32_t, int32_t>> want = {{0, 0}, {1, 0}, {-1, -1}, {2, 0}, {1, 1}};
        EXPECT(g.where == want);
        if (g.slots.size() == 3) EXPECT((g.slots[0] == V32{1004}) && (g.slots[1] == V32{1005, 1007}) && (g.slots[2] == V32{1006}));
        pf::PairGroups p(true);  // a range that does not start at 0: where is indexed from i0
        p.add_uids(nullptr, b, 1, 5, idx_of, slot_of, note);
        const std::vector<std::pair<int32_t, int32_t>> wantp = {{0, 0}, {-1, -1}, {0, 1}, {0, 2}};
        EXPECT(p.where == wantp);
    }
    if (bad) return 1;
    std::printf("ok pair groups\n");
    return 0;
}
