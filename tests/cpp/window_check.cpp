// Host check of the scans' score window (csrc/pf_window.h, the text the kernels run).
//   1. window_pass against the plain tuple comparison: a candidate (score, id) is in the window when
//      score >= min_score (under a floor) and (score < after_score or score == after_score and id >
//      after_id) (under a cursor), -0.0 taken as 0.0; over edge scores x edge ids, with and without a
//      floor and a cursor and each combined with the other, in the uid-keyed form and in K5's idx form.
//   2. window_theta0 at every histogram bin edge, its float neighbours, 1.0 and values around the
//      histogram's ends: a bin edge with its low 15 bits clear, <= min_score, 0 below 2^-3; and with
//      need[] = prune_need(theta0, u, 7 + T) for T in {0, 1, 48} and every u, no term sum whose
//      reference float score is >= min_score is prune_dead (prune_check.cpp's sweep with the floor in
//      theta's place).
//   3. the ABI: pf_scan_window is 24 B and its bits are pf_window.h's.
// Prints "ok <cases>" or the first violation.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pf_window.h"
#include "pokec_fas.h"

static_assert(sizeof(pf_scan_window) == 24, "pf_scan_window is 24 B");
static_assert(PF_WIN_MIN == pf::kWinMin && PF_WIN_AFTER == pf::kWinAfter && PF_WIN_COUNT == pf::kWinCount, "window bits");

static float from_bits(uint32_t b) { return pf::prune_float(b); }

static bool ref_pass(float s, int64_t id, bool has_min, float mn, bool has_after, float as, int64_t aid) {
    if (has_min && !(s >= mn)) return false;  // (IEEE: -0.0 >= 0.0 and 0.0 >= -0.0)
    if (has_after && !(s < as || (s == as && id > aid))) return false;
    return true;
}

static float ref_score(double acc, int u, int nterms) {
    if (u <= 0) return 0.0f;
    const double S = acc / (double)u;
    const double F = (double)u / (double)nterms;
    return (S <= 0.0 && F <= 0.0) ? 0.0f : (float)((2.0 * S * F) / (S + F));
}

int main() {
    long cases = 0;
    // ---- 1. window_pass
    const float lowe = from_bits(pf::kPruneLowBits);
    const std::vector<float> scores = {0.0f, -0.0f, from_bits(1u), from_bits(0x007FFFFFu), std::nextafter(lowe, 0.0f), lowe,
                                       std::nextafter(lowe, 1.0f), 0.10361052f, 0.14928986f, 0.35457027f,
                                       std::nextafter(0.35457027f, 0.0f), std::nextafter(0.35457027f, 1.0f),
                                       std::nextafter(1.0f, 0.0f), 1.0f, std::nextafter(1.0f, 2.0f), 1.5f, 3.0e38f, -0.25f};
    const std::vector<int32_t> ids = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 2000000000, INT32_MAX - 1, INT32_MAX};
    std::vector<float> bounds = scores;
    bounds.push_back(INFINITY);
    bounds.push_back(-INFINITY);
    for (int has_min = 0; has_min < 2; ++has_min)
        for (int has_after = 0; has_after < 2; ++has_after)
            for (float mn : bounds) {
                if (!has_min && mn != bounds[0]) continue;
                for (float as : bounds)
                    for (int32_t aid : ids) {
                        if (!has_after && (as != bounds[0] || aid != ids[0])) continue;
                        const uint32_t fields = (has_min ? pf::kWinMin : 0u) | (has_after ? pf::kWinAfter : 0u);
                        const pf::ScanWindow W = pf::window_make(fields, mn, as, aid);
                        if (!has_min && (W.hi != ~0ull || W.theta0 != 0u)) { std::printf("no floor: hi / theta0 set\n"); return 1; }
                        if (!has_after && W.lo != 0ull) { std::printf("no cursor: lo set\n"); return 1; }
                        for (float s : scores)
                            for (int32_t id : ids) {
                                ++cases;
                                const bool want = ref_pass(s, id, has_min, mn, has_after, as, aid);
                                const uint64_t key = pf::window_key(s, id);
                                if (key == ~0ull) { std::printf("a candidate's key is the empty slot\n"); return 1; }
                                if (pf::window_pass(key, W) != want) {
                                    std::printf("uid form: s=%a id=%d min=%d:%a after=%d:%a:%d: got %d want %d\n", s, id, has_min, mn,
                                                has_after, as, aid, (int)!want, (int)want);
                                    return 1;
                                }
                            }
                        // K5's form: the ids above are the uids of idx 0 .. 7 (ascending); a candidate's
                        // key carries its idx, the cursor's uid becomes the first idx whose uid exceeds it
                        const uint32_t first = (uint32_t)(std::upper_bound(ids.begin(), ids.end(), aid) - ids.begin());
                        const pf::ScanWindow P = pf::window_for_idx(W, as, first);
                        for (float s : scores)
                            for (size_t x = 0; x < ids.size(); ++x) {
                                ++cases;
                                const bool want = ref_pass(s, ids[x], has_min, mn, has_after, as, aid);
                                if (pf::window_pass(pf::window_key(s, (int32_t)x), P) != want) {
                                    std::printf("idx form: s=%a idx=%zu min=%d:%a after=%d:%a:%d: want %d\n", s, x, has_min, mn,
                                                has_after, as, aid, (int)want);
                                    return 1;
                                }
                            }
                    }
            }
    // a cursor between two stored uids, below all and above all, in idx form
    {
        const std::vector<int32_t> uids = {10, 20, 30};
        const int32_t cur[] = {5, 10, 15, 30, 35, INT32_MAX, INT32_MIN};
        for (int32_t a : cur) {
            const uint32_t first = (uint32_t)(std::upper_bound(uids.begin(), uids.end(), a) - uids.begin());
            const pf::ScanWindow P = pf::window_for_idx(pf::window_make(pf::kWinAfter, 0.f, 0.5f, a), 0.5f, first);
            for (size_t x = 0; x < uids.size(); ++x) {
                ++cases;
                if (pf::window_pass(pf::window_key(0.5f, (int32_t)x), P) != (uids[x] > a)) { std::printf("idx cursor %d\n", a); return 1; }
                if (!pf::window_pass(pf::window_key(0.25f, (int32_t)x), P) || pf::window_pass(pf::window_key(0.75f, (int32_t)x), P)) {
                    std::printf("idx cursor %d: other scores\n", a);
                    return 1;
                }
            }
        }
    }
    // ---- 2. window_theta0
    std::vector<uint32_t> floors;
    for (int b = 0; b < pf::kPruneBins; ++b) {
        const uint32_t e = pf::prune_edge(b);
        floors.push_back(e - 1);
        floors.push_back(e);
        floors.push_back(e + 1);
    }
    floors.push_back(pf::kPruneOneBits);
    floors.push_back(0x3F800001u);
    floors.push_back(0x40000000u);  // 2.0
    floors.push_back(0x7F800000u);  // +inf
    floors.push_back(0u);
    floors.push_back(1u);
    floors.push_back(0x3DD43216u);  // ~0.1036, below the histogram
    floors.push_back(0x80000000u);  // -0.0
    floors.push_back(0xBE800000u);  // -0.25
    const uint32_t lowmask = (1u << pf::kPruneShift) - 1u;
    const int Ts[3] = {0, 1, 48};
    long sweep = 0;
    for (uint32_t fb : floors) {
        const float mn = from_bits(fb);
        const uint32_t t0 = pf::window_theta0(mn);
        ++cases;
        if (t0 & lowmask) { std::printf("theta0(%a) = %08x: low bits set\n", mn, t0); return 1; }
        const bool below = !(mn >= lowe);
        if (below != (t0 == 0u)) { std::printf("theta0(%a) = %08x: zero exactly below 2^-3\n", mn, t0); return 1; }
        if (t0 != 0u) {
            const int b = pf::prune_bin(t0);
            if (b < 0 || pf::prune_edge(b) != t0) { std::printf("theta0(%a) = %08x: no bin edge\n", mn, t0); return 1; }
            if (!(from_bits(t0) <= mn)) { std::printf("theta0(%a) = %a above the floor\n", mn, from_bits(t0)); return 1; }
            // the highest such edge
            if (b + 1 < pf::kPruneBins && from_bits(pf::prune_edge(b + 1)) <= mn) { std::printf("theta0(%a): a higher edge fits\n", mn); return 1; }
        }
        // nobody at or above the floor dies: for every u, the sums around need[u] (prune_check's grid)
        for (int T : Ts) {
            const int nterms = 7 + T;
            for (int u = 0; u <= nterms; ++u) {
                const double need = pf::prune_need(t0, u, nterms);
                if (std::isinf(need)) {
                    ++sweep;
                    if (ref_score((double)u, u, nterms) >= mn) { std::printf("floor %a T=%d u=%d: need = inf but S = 1 reaches it\n", mn, T, u); return 1; }
                    continue;
                }
                std::vector<double> accs;
                for (int i = 0; i <= 32; ++i) accs.push_back((double)u * (double)i / 32.0);
                double x = need - 1e-9;
                for (int i = 0; i < 8; ++i) { accs.push_back(x); x = std::nextafter(x, -1.0); }
                x = need - 1e-9;
                for (int i = 0; i < 8; ++i) { accs.push_back(x); x = std::nextafter(x, 1e300); }
                for (double acc : accs) {
                    if (!(acc >= 0.0) || acc > (double)u) continue;
                    ++sweep;
                    if (ref_score(acc, u, nterms) >= mn && pf::prune_dead(acc, 0.0, need)) {
                        std::printf("floor %a T=%d u=%d acc=%a: scores %a >= floor but is dropped (need %a)\n", mn, T, u, acc,
                                    ref_score(acc, u, nterms), need);
                        return 1;
                    }
                }
            }
        }
    }
    std::printf("ok %ld window cases, %ld floor sums\n", cases, sweep);
    return 0;
}
