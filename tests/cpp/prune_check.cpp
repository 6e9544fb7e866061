// Host check of K5's score bound (csrc/pf_prune.h, the text the kernel runs): for every column
// count T in {0, 1, 48}, every number of used terms u, and theta at every histogram bin edge, its
// float neighbours and 1.0, a term sum below need[u] - 1e-9 must score strictly below theta by the
// reference's formula (recommender_similarity.cpp:114-123), and a u whose need is +infinity must
// score below theta even at S = 1.  Prints "ok <cases>" or the first violation.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pf_prune.h"

static float ref_score(double acc, int u, int nterms) {
    if (u <= 0) return 0.0f;
    const double S = acc / (double)u;
    const double F = (double)u / (double)nterms;
    return (S <= 0.0 && F <= 0.0) ? 0.0f : (float)((2.0 * S * F) / (S + F));
}

int main() {
    std::vector<uint32_t> thetas;
    for (int b = 0; b < pf::kPruneBins; ++b) {
        const uint32_t e = pf::prune_edge(b);
        thetas.push_back(e - 1);
        thetas.push_back(e);
        thetas.push_back(e + 1);
    }
    thetas.push_back(pf::kPruneOneBits);
    if (pf::prune_bin(pf::kPruneLowBits) != 0 || pf::prune_bin(pf::kPruneLowBits - 1) != -1 ||
        pf::prune_bin(pf::kPruneOneBits) != pf::kPruneBins - 1 || pf::prune_bin(pf::kPruneOneBits - 1) != pf::kPruneBins - 2 ||
        pf::prune_bin(0x40000000u) != pf::kPruneBins - 1 || pf::prune_edge(pf::kPruneBins - 1) != pf::kPruneOneBits) {
        std::printf("bin mapping wrong\n");
        return 1;
    }
    long cases = 0, tight = 0;
    const int Ts[3] = {0, 1, 48};
    for (int T : Ts) {
        const int nterms = 7 + T;
        for (int u = 0; u <= nterms; ++u) {
            if (pf::prune_need(0u, u, nterms) != 0.0 || pf::prune_dead(0.0, 0.0, pf::prune_need(0u, u, nterms))) {
                std::printf("theta 0 must drop nothing (u=%d)\n", u);
                return 1;
            }
            for (uint32_t tb : thetas) {
                const float theta = pf::prune_float(tb);
                const double need = pf::prune_need(tb, u, nterms);
                if (std::isinf(need)) {
                    ++cases;
                    if (!(ref_score((double)u, u, nterms) < theta)) {
                        std::printf("T=%d u=%d theta=%a: need = inf but S = 1 scores %a\n", T, u, theta, ref_score(u, u, nterms));
                        return 1;
                    }
                    continue;
                }
                const double lim = need - 1e-9;
                std::vector<double> accs;
                for (int i = 0; i <= 32; ++i) accs.push_back(lim * (double)i / 32.0);
                double x = lim;
                for (int i = 0; i < 8; ++i) {
                    x = std::nextafter(x, -1.0);
                    accs.push_back(x);
                }
                x = lim;
                for (int i = 0; i < 8; ++i) {  // and the doubles at and above it the kernel's own test still drops
                    accs.push_back(x);
                    x = std::nextafter(x, 1e300);
                }
                for (double acc : accs) {
                    if (!(acc >= 0.0) || !(acc < lim || pf::prune_dead(acc, 0.0, need))) continue;
                    ++cases;
                    const float f = ref_score(acc, u, nterms);
                    if (!(f < theta)) {
                        std::printf("T=%d u=%d theta=%a acc=%a need=%a: score %a not below theta\n", T, u, theta, acc, need, f);
                        return 1;
                    }
                }
                // not vacuous: a sum at need[u] scores within 2^-19 of theta
                if (u > 0 && need <= (double)u) {
                    ++tight;
                    if (!(ref_score(need, u, nterms) >= theta * (1.0f - 1.0f / 524288.0f))) {
                        std::printf("T=%d u=%d theta=%a: the bound is loose, need=%a scores %a\n", T, u, theta, need,
                                    ref_score(need, u, nterms));
                        return 1;
                    }
                }
            }
        }
    }
    std::printf("ok %ld cases, %ld tightness checks\n", cases, tight);
    return 0;
}
