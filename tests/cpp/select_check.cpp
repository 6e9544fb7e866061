// CPU sweep of csrc/pf_select.h, the text the kernels run: select_apply on a copy of a query's
// constants against a plain restatement of the rule (pokec_fas.h "Field selection"): a deselected
// fixed field reads as missing on the query's side, the column mask loses the deselected columns,
// and n_cols becomes the number of selected columns of the engine's T.  Every subset of the seven
// fixed bits x column masks of 0, each single bit, every prefix, all of T, all 64 bits and bits
// above T only, for T = 1 / 48 / 64.  Prints "sizeof <public> <device>" and "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pf_select.h"
#include "pokec_fas.h"

namespace {

// the members of pf::QConst (pf_types.h) the selection touches, and two it must leave alone
struct Q {
    uint64_t colmask;
    int32_t comp, age;
    int32_t reg[3];
    uint32_t pubcode, gencode;
    int32_t a_regcnt;
    int32_t n_clubs, n_friends;
    int32_t lg;
    int32_t n_cols;
    double sqrt_clubs;
};

Q make(int T, uint64_t colmask) {
    Q q{};
    q.colmask = colmask;
    q.comp = 77;
    q.age = 31;
    q.reg[0] = 2; q.reg[1] = 4; q.reg[2] = 9;
    q.pubcode = 1;
    q.gencode = 0;
    q.a_regcnt = 3;
    q.n_clubs = 4;
    q.n_friends = 9;
    q.lg = 6;
    q.n_cols = T;
    q.sqrt_clubs = 2.0;
    return q;
}

// the rule, restated without pf_select.h's helpers
Q expect(const Q& in, uint32_t fixed, uint64_t cols) {
    Q q = in;
    if (!((fixed >> PF_F_PUBLIC) & 1u)) q.pubcode = 0xFFu;
    if (!((fixed >> PF_F_GENDER) & 1u)) q.gencode = 0xFFu;
    if (!((fixed >> PF_F_COMPLETION) & 1u)) q.comp = 0;
    if (!((fixed >> PF_F_AGE) & 1u)) q.age = 0;
    if (!((fixed >> PF_F_REGION) & 1u)) q.a_regcnt = 0;
    if (!((fixed >> PF_F_CLUBS) & 1u)) q.n_clubs = 0;
    if (!((fixed >> PF_F_FRIENDS) & 1u)) q.n_friends = 0;
    int n = 0;
    uint64_t cm = 0;
    for (int t = 0; t < 64; ++t) {
        const bool sel = (cols >> t) & 1ull;
        if (sel && t < in.n_cols) ++n;
        if (sel && ((in.colmask >> t) & 1ull)) cm |= 1ull << t;
    }
    q.colmask = cm;
    q.n_cols = n;
    return q;
}

bool same(const Q& a, const Q& b) {
    return a.colmask == b.colmask && a.comp == b.comp && a.age == b.age && !std::memcmp(a.reg, b.reg, sizeof a.reg) &&
           a.pubcode == b.pubcode && a.gencode == b.gencode && a.a_regcnt == b.a_regcnt && a.n_clubs == b.n_clubs &&
           a.n_friends == b.n_friends && a.lg == b.lg && a.n_cols == b.n_cols && a.sqrt_clubs == b.sqrt_clubs;
}

}  // namespace

int main() {
    std::printf("sizeof %zu %zu\n", sizeof(pf_field_select), sizeof(pf::FieldSel));
    long cases = 0;
    const int Ts[3] = {1, 48, 64};
    for (int T : Ts) {
        const uint64_t all = T >= 64 ? ~0ull : ((1ull << T) - 1ull);
        std::vector<uint64_t> masks = {0ull, all, ~0ull, ~all, all & 0x5555555555555555ull, all & 0xAAAAAAAAAAAAAAAAull};
        for (int t = 0; t < 64; ++t) masks.push_back(1ull << t);                    // one bit, above T included
        for (int t = 1; t <= T; ++t) masks.push_back(t >= 64 ? ~0ull : ((1ull << t) - 1ull));  // prefixes
        masks.push_back((all >> 1) | ~all);                                        // a prefix plus bits above T
        // the query's own non-empty columns: none, all of T, every third
        const uint64_t qcols[3] = {0ull, all, all & 0x9249249249249249ull};
        for (uint64_t qc : qcols)
            for (uint32_t fixed = 0; fixed <= PF_SEL_FIXED_ALL; ++fixed)
                for (uint64_t cols : masks) {
                    const Q in = make(T, qc);
                    Q got = in;
                    pf::FieldSel s{fixed, 1u, cols};
                    pf::select_apply(got, s);
                    const Q want = expect(in, fixed, cols);
                    ++cases;
                    if (!same(got, want)) {
                        std::printf("mismatch T=%d fixed=%02x cols=%016llx qcols=%016llx: n_cols %d / %d colmask %016llx / %016llx\n",
                                    T, fixed, (unsigned long long)cols, (unsigned long long)qc, got.n_cols, want.n_cols,
                                    (unsigned long long)got.colmask, (unsigned long long)want.colmask);
                        return 1;
                    }
                    // everything selected leaves the constants as they were, and is recognised as such
                    const bool is_all = fixed == PF_SEL_FIXED_ALL && (cols & all) == all;
                    if (is_all != pf::select_is_all(fixed, cols, T) || (is_all && !same(got, in))) {
                        std::printf("everything selected: T=%d fixed=%02x cols=%016llx\n", T, fixed, (unsigned long long)cols);
                        return 1;
                    }
                    if (pf::select_ncols(cols, T) != want.n_cols) {
                        std::printf("select_ncols T=%d cols=%016llx\n", T, (unsigned long long)cols);
                        return 1;
                    }
                }
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
