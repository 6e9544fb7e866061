// pf_prune.h — K5's score bound (DESIGN.md "K5 pruning"): the shared threshold's histogram bins
// and the table need[u] a candidate's term sum must reach.  Plain C++ on both sides, so the CPU
// test (tests/cpp/prune_check.cpp) runs the text the kernel runs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_HD __host__ __device__
#else
#define PF_HD
#endif

namespace pf {

// Histogram of recorded scores: 256 bins per binade over [2^-3, 1) (bin = float bits >> 15, minus
// the base), one more for scores >= 1; smaller scores are not recorded.
constexpr uint32_t kPruneShift = 15;
constexpr uint32_t kPruneLowBits = 0x3E000000u;                   // 2^-3
constexpr uint32_t kPruneOneBits = 0x3F800000u;                   // 1.0
constexpr int kPruneBase = (int)(kPruneLowBits >> kPruneShift);
constexpr int kPruneBins = (int)(kPruneOneBits >> kPruneShift) - kPruneBase + 1;  // 769

// the bin of a score's float bits, or -1 (below 2^-3, negative)
PF_HD inline int prune_bin(uint32_t bits) {
    if (bits < kPruneLowBits || bits >= 0x80000000u) return -1;
    const uint32_t b = bits >> kPruneShift, top = kPruneOneBits >> kPruneShift;
    return (int)(b < top ? b : top) - kPruneBase;
}
// float bits of a bin's lower edge
PF_HD inline uint32_t prune_edge(int bin) { return (uint32_t)(bin + kPruneBase) << kPruneShift; }

PF_HD inline float prune_float(uint32_t bits) {
    union { uint32_t u; float f; } v;
    v.u = bits;
    return v.f;
}

// Deriving theta from the histogram, by one wave in slabs of 64 bins from the top: slab i is bins
// top - 64 i .. top - 64 i - 63 and lane l takes bin top - 64 i - l, so one load instruction of the
// wave covers two 128-B lines.  A derived theta is used only if it exceeds thb, the theta the block
// began with (0, or a bin's lower edge), so only the bins above prune_bin(thb) can yield it: the
// slabs that hold none of them are not read, and a lane at or below that bin counts 0.  With the
// counts from above accumulated slab by slab, the answer is the one bin where they reach k; if the
// live bins never reach k the block keeps thb.  (tests/cpp/derive_check.cpp runs these functions
// lane by lane against a serial scan from the top bin.)
constexpr int kPruneSlab = 64;
constexpr int kPruneSlabs = (kPruneBins + kPruneSlab - 1) / kPruneSlab;  // 13
// the bin of slab i's lane l (negative past the histogram's low end, in the last slab)
PF_HD inline int prune_slab_bin(int slab, int lane) { return kPruneBins - 1 - (kPruneSlab * slab + lane); }
// the bin counts for a block that began with thb: above thb's own bin (thb = 0: every bin)
PF_HD inline bool prune_bin_live(int bin, uint32_t thb) { return bin > prune_bin(thb); }
// slabs with at least one live bin: 0 (thb in the top bin) .. kPruneSlabs (thb = 0)
PF_HD inline int prune_slabs(uint32_t thb) { return (kPruneBins - 1 - prune_bin(thb) + kPruneSlab - 1) / kPruneSlab; }
// this lane's bin is the answer: `above` = the count of the slabs before, incl = the inclusive sum
// over the slab's lanes up to this one, c = its own count
PF_HD inline bool prune_pick(uint32_t above, uint32_t incl, uint32_t c, uint32_t k) {
    return above + incl >= k && above + incl - c < k;
}

// need[u]: what the term sum of a candidate with u terms used must reach for its score to reach
// theta (float bits; 0 = no threshold yet: 0, nothing is dropped).  nterms = 7 + T.
//
// The score is f = (float)(2 S F / (S + F)), S = acc / u, F = u / nterms (recommender_similarity.cpp:
// 114-123), increasing in S, and g(S) = 2SF/(S+F) = t exactly at S = tF / (2F - t) (2F > t; with
// 2F <= t no S <= 1 reaches t: g(1) = 2F/(1+F) < 2F).  With t = theta (1 - 2^-20):
//   acc + 1e-9 < need[u] = u t F / (2F - t)
//     => exact S < tF/(2F - t) - 1e-9/u: the 1e-9 outweighs the rounding of need (four double
//        operations, < 1e-13) and of acc (<= 55 additions of values <= 1, < 1e-14)
//     => exact g(S) < t; the computed one (four roundings) < t (1 + 2^-50) < theta (1 - 2^-21)
//     => its float cast (relative error <= 2^-24) is below theta's float predecessor's upper
//        neighbourhood, that is < theta: a candidate scoring exactly theta is never dropped.
// A term is a sigmoid value, (1 or e) / (1 + e) with e >= 0, at most 1.0 as computed, so
// acc so far + the number of terms still to come bounds the final acc.
// theta itself is valid because only keyed candidates are recorded in the histogram: an excluded
// candidate, and one the scan's candidate filter drops (pf_filter.h), is never keyed, so at least k
// candidates that can be ranked score >= theta, with or without a filter.
PF_HD inline double prune_need(uint32_t theta_bits, int u, int nterms) {
    if (theta_bits == 0u) return 0.0;
    const double t = (double)prune_float(theta_bits) * (1.0 - 1.0 / 1048576.0);
    const double F = (double)u / (double)nterms;
    const double d = 2.0 * F - t;
    if (!(d > 0.0)) return __builtin_huge_val();
    return (double)u * (t * F) / d;
}

// the candidate cannot reach theta: acc so far, `remaining` terms still to come (each <= 1)
PF_HD inline bool prune_dead(double acc, double remaining, double need) { return acc + remaining + 1e-9 < need; }

}  // namespace pf
