// K5's round planning (pf_kernels.hip fas_post_kernel; tools/probe/k5_plan.hip runs both planners
// over the same inputs): the serial planner, and the one that holds a column per lane.
#pragma once
#include "pf_device.h"

namespace pf {

// The next round from (column ci, token jcur): tokens [ja, jb), columns [ca, ce) touched (ce - 1
// is left unfinished when ci_next == ce - 1).  Greedy: whole columns while the round holds <= 64
// tokens and <= kRoundCap entries; a column that does not fit an empty round is split (at least
// one token, whose entries in the block are <= kBlockCands hits).
struct Round {
    int ja, jb, ca, ce;
};
template <int CAP = kRoundCap>
__device__ __forceinline__ Round next_round(const QCol* scol, const uint32_t* gpre, int n_act, int& ci, int& jcur) {
    Round r;
    r.ja = jcur;
    r.jb = jcur;
    r.ca = ci;
    const uint32_t g0 = gpre[r.ja];
    while (ci < n_act) {
        const int j1 = scol[ci].j1;
        if (j1 - r.ja <= kRoundToks && gpre[j1] - g0 <= (uint32_t)CAP) {
            r.jb = j1;
            ++ci;
            continue;
        }
        if (r.jb == r.ja) {
            int jb = r.ja + 1;
            const int lim = min(j1, r.ja + kRoundToks);
            while (jb < lim && gpre[jb + 1] - g0 <= (uint32_t)CAP) ++jb;
            r.jb = jb;
            if (jb == j1) ++ci;
        }
        break;
    }
    jcur = r.jb;
    r.ce = (ci < n_act && scol[ci].j0 < r.jb) ? ci + 1 : ci;
    return r;
}

// The same rounds with lane c holding active column c (n_act <= kPostMaxCols < 64 lanes): the
// serial planner reads scol[ci].j1 and then gpre[j1] per column, two dependent LDS round trips on
// the one wave every other wave of the workgroup waits for; here a round is one compare per lane,
// a ballot and a find-first.  The columns' tokens never change during a launch; K5 still calls
// col_tokens in every block (one LDS read per lane, issued before the prefix scan it waits under)
// because holding them would cost two VGPRs of every wave through the whole block loop.  gpre
// changes with every block (col_ends, one more LDS read per lane).
struct ColPlan {
    int j0, j1;   // the lane's column's tokens (lanes >= n_act: unused)
    uint32_t g1;  // gpre[j1]
};
__device__ __forceinline__ ColPlan col_tokens(const QCol* scol, int n_act, int lane) {
    ColPlan p;
    const QCol c = scol[min(lane, max(n_act, 1) - 1)];
    p.j0 = c.j0;
    p.j1 = c.j1;
    p.g1 = 0u;
    return p;
}
__device__ __forceinline__ void col_ends(ColPlan& p, const uint32_t* gpre, int n_act, int lane) {
    p.g1 = lane < n_act ? gpre[p.j1] : 0u;
}
// wave-uniform like next_round (every lane of the wave calls it with the same ci, jcur)
template <int CAP = kRoundCap>
__device__ __forceinline__ Round plan_round(const ColPlan& p, const uint32_t* gpre, int n_act, int lane, int& ci,
                                            int& jcur) {
    Round r;
    r.ja = jcur;
    r.jb = jcur;
    r.ca = ci;
    const uint32_t g0 = gpre[r.ja];
    // the first column from ci on that does not fit with the ones before it
    const bool fits = p.j1 - r.ja <= kRoundToks && p.g1 - g0 <= (uint32_t)CAP;
    const uint64_t nf = __ballot(lane >= ci && lane < n_act && !fits);
    const int first = nf ? __ffsll((unsigned long long)nf) - 1 : n_act;
    if (first > ci) r.jb = __builtin_amdgcn_readlane(p.j1, first - 1);
    ci = first;
    if (ci < n_act && r.jb == r.ja) {  // it does not fit an empty round: split by tokens (rare)
        const int j1 = __builtin_amdgcn_readlane(p.j1, ci);
        int jb = r.ja + 1;
        const int lim = min(j1, r.ja + kRoundToks);
        while (jb < lim && gpre[jb + 1] - g0 <= (uint32_t)CAP) ++jb;
        r.jb = jb;
        if (jb == j1) ++ci;
    }
    jcur = r.jb;
    r.ce = (ci < n_act && __builtin_amdgcn_readlane(p.j0, min(ci, 63)) < r.jb) ? ci + 1 : ci;
    return r;
}

}  // namespace pf
