// pf_select.h — per-call field selection of FAS (DESIGN.md "Field selection"): the device form of
// pf_field_select and the one function that applies it to a copy of a query's constants.  Plain
// C++ on both sides, so the CPU test (tests/cpp/select_check.cpp) runs the text the kernels run.
// Templated on the constants' type: the kernels pass the staged QConst (pf_types.h), the CPU test
// a struct with the same member names.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_SHD __host__ __device__
#else
#define PF_SHD
#endif

namespace pf {

// fixed-field bits: bit k = PF_F_* (pokec_fas.h; pf_api.cpp asserts they agree)
constexpr uint32_t kSelPublic = 1u << 0, kSelGender = 1u << 1, kSelCompletion = 1u << 2, kSelAge = 1u << 3,
                   kSelRegion = 1u << 4, kSelClubs = 1u << 5, kSelFriends = 1u << 6;
constexpr uint32_t kSelFixedAll = 0x7Fu;
// header code of a missing public / gender value (pf_types.h kCodeMissing)
constexpr uint32_t kSelCodeMissing = 0xFFu;

// Passed by value as a kernel argument.  on == 0: no selection (the launch reads no other word).
// cols: bit t = text column t of the engine's list; bits at or above the query's n_cols are ignored.
struct FieldSel {
    uint32_t fixed, on;
    uint64_t cols;
};
static_assert(sizeof(FieldSel) == 16, "FieldSel is a 16-B kernel argument");

// the low n bits (n <= 64)
PF_SHD inline uint64_t select_low(int n) { return n >= 64 ? ~0ull : ((1ull << (n < 0 ? 0 : n)) - 1ull); }
// bits set, in plain C++ (the host side has no __popcll)
PF_SHD inline int select_popcount(uint64_t x) {
    int n = 0;
    for (; x; x &= x - 1ull) ++n;
    return n;
}
// T' of a selection over an engine of T columns: the denominator's 7 + T'
PF_SHD inline int select_ncols(uint64_t cols, int T) { return select_popcount(cols & select_low(T)); }

// The selection applied to a copy of the query's constants (never to a query image): a deselected
// fixed field reads as missing on the query's side, exactly as for a user who left it empty
// (recommender_similarity.cpp:38-91: public / gender < 0, completion / age = 0, no region part, an
// empty club / friend list), a deselected column as one the query has no token in, and n_cols,
// which the kernels only ever read as FAS's denominator 7 + T, becomes the selected columns'
// count.  Everything selected leaves q as it was.
template <class Q>
PF_SHD inline void select_apply(Q& q, const FieldSel& s) {
    if (!(s.fixed & kSelPublic)) q.pubcode = kSelCodeMissing;
    if (!(s.fixed & kSelGender)) q.gencode = kSelCodeMissing;
    if (!(s.fixed & kSelCompletion)) q.comp = 0;
    if (!(s.fixed & kSelAge)) q.age = 0;
    if (!(s.fixed & kSelRegion)) q.a_regcnt = 0;
    if (!(s.fixed & kSelClubs)) q.n_clubs = 0;
    if (!(s.fixed & kSelFriends)) q.n_friends = 0;
    const int T = q.n_cols;
    q.colmask &= s.cols;
    q.n_cols = select_ncols(s.cols, T);
}

// whether a selection leaves out nothing of an engine of T columns (then it is cleared)
PF_SHD inline bool select_is_all(uint32_t fixed, uint64_t cols, int T) {
    return (fixed & kSelFixedAll) == kSelFixedAll && (cols & select_low(T)) == select_low(T);
}

}  // namespace pf
