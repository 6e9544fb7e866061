// pf_window.h — the scans' score window (pokec_fas.h pf_scan_window): a floor, a paging cursor and a
// match count, as two bounds in the space of the top-k keys.  Plain C++ on both sides, so the CPU
// test (tests/cpp/window_check.cpp) runs the text the kernels run.
#pragma once
#include <stdint.h>

#include "pf_prune.h"

namespace pf {

constexpr uint32_t kWinMin = 1u, kWinAfter = 2u, kWinCount = 4u;  // = PF_WIN_* (pf_api.cpp asserts it)
constexpr uint32_t kWinAllFields = kWinMin | kWinAfter | kWinCount;
// device-only: the launch appends every in-window key to the context's collector (pf_collect.h).  Never
// taken from the public struct (pf_set_scan_window refuses it); a collecting call's options carry it,
// with kWinCount (pf_scan_call.h make_scan_call, the one place that sets it).
constexpr uint32_t kWinCollect = 8u;

// What a launch carries, by value in its arguments.  A key (pf_types.h score_key: ascending key =
// score desc, id asc) is in the window when lo <= key <= hi.
//   lo   the first key after the cursor: the cursor's own key + 1, so a carry out of the id word
//        (after_uid == INT32_MAX) moves on to the next lower score by itself; 0 without a cursor.
//   hi   the last key at the floor: (min_score, the highest id); ~0 without a floor.  ~0 itself is
//        the top-k lists' empty slot and no candidate's key (its score word would be a negative NaN).
//   theta0  K5's seed (window_theta0), 0 without a floor.
//   fields  the window's PF_WIN_* bits; 0 = no window: lo = 0, hi = ~0 and every key passes.
// K1 and the group kernel key by uid, K5 by idx (idx order is uid order): window_for_idx turns the
// cursor's uid into K5's bound.
struct ScanWindow {
    uint64_t lo = 0ull, hi = ~0ull;
    uint32_t theta0 = 0u, fields = 0u;
};
static_assert(sizeof(ScanWindow) == 24, "ScanWindow rides in the launches' arguments");

PF_HD inline uint32_t window_bits(float f) {
    union { float f; uint32_t u; } v;
    v.f = f;
    return v.u;
}
// score_key's upper word: ascending = score descending, -0.0 taken as 0.0
PF_HD inline uint32_t window_score_word(float s) {
    uint32_t b = window_bits(s);
    if ((b & 0x7FFFFFFFu) == 0u) b = 0u;
    const uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ~ord;
}
PF_HD inline uint64_t window_key(float s, int32_t id) {
    return ((uint64_t)window_score_word(s) << 32) | (uint32_t)((uint32_t)id ^ 0x80000000u);
}

// K5's seed: the highest histogram bin edge <= min_score, so a theta of the usual form (a bin's lower
// edge, its low kPruneShift bits clear: prune_derive packs k there) that drops nobody at or above the
// floor.  0 below the histogram's low edge 2^-3 and for a non-positive floor: such a scan is unseeded.
PF_HD inline uint32_t window_theta0(float min_score) {
    const int b = prune_bin(window_bits(min_score));
    return b < 0 ? 0u : prune_edge(b);
}

// The uid-keyed window of the public struct's members (validated by the caller: no NaN).
PF_HD inline ScanWindow window_make(uint32_t fields, float min_score, float after_score, int32_t after_uid) {
    ScanWindow W;
    W.fields = fields & kWinAllFields;
    if (fields & kWinMin) {
        W.hi = window_key(min_score, INT32_MAX);
        W.theta0 = window_theta0(min_score);
    }
    if (fields & kWinAfter) W.lo = window_key(after_score, after_uid) + 1ull;
    return W;
}
// The same window for keys that carry an idx: first_idx = the first idx whose uid exceeds after_uid
// (n when none does: no candidate has that idx, and the tie at after_score is then empty).
PF_HD inline ScanWindow window_for_idx(ScanWindow W, float after_score, uint32_t first_idx) {
    if (W.fields & kWinAfter) W.lo = ((uint64_t)window_score_word(after_score) << 32) | (first_idx ^ 0x80000000u);
    return W;
}

PF_HD inline bool window_pass(uint64_t key, const ScanWindow& W) { return key >= W.lo && key <= W.hi; }

}  // namespace pf
