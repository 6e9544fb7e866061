// Device check of K5's round planning (pf_plan.h): the serial next_round and the lane-parallel
// plan_round run over the same columns and entry prefixes, one wave per case, and every round tuple
// and the round count must agree.  The host builds inputs and compares the two device results; it
// plans nothing itself.  Prints OK and the sweep's figures, or the first mismatches.
//   hipcc --offload-arch=gfx950 -O3 -I csrc tools/probe/k5_plan.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "pf_plan.h"
using namespace pf;

#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FAIL %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Case {
    int n_act, col0, tok0, out0, cap;  // first column / first gpre word / first output row, rows allowed
};

__global__ void probe(const Case* cases, const QCol* cols, const uint32_t* gpre_all, int4* out_s, int4* out_l, int* nr_s,
                      int* nr_l) {
    const Case c = cases[blockIdx.x];
    const int lane = threadIdx.x & 63;
    const QCol* scol = cols + c.col0;
    const uint32_t* gpre = gpre_all + c.tok0;
    {
        int ci = 0, j = 0, nr = 0;
        while (ci < c.n_act && nr < c.cap) {
            const Round r = next_round(scol, gpre, c.n_act, ci, j);
            if (lane == 0) out_s[c.out0 + nr] = make_int4(r.ja, r.jb, r.ca, r.ce);
            ++nr;
        }
        if (lane == 0) nr_s[blockIdx.x] = nr;
    }
    {
        ColPlan p = col_tokens(scol, c.n_act, lane);
        col_ends(p, gpre, c.n_act, lane);
        int ci = 0, j = 0, nr = 0;
        while (ci < c.n_act && nr < c.cap) {
            const Round r = plan_round(p, gpre, c.n_act, lane, ci, j);
            if (lane == 0) out_l[c.out0 + nr] = make_int4(r.ja, r.jb, r.ca, r.ce);
            ++nr;
        }
        if (lane == 0) nr_l[blockIdx.x] = nr;
    }
}

struct Builder {
    std::vector<Case> cases;
    std::vector<QCol> cols;
    std::vector<uint32_t> gpre;
    int rows = 0;
    // columns of the given token counts (contiguous, ascending), one entry count per token
    void add(const std::vector<int>& col_toks, const std::vector<uint32_t>& len) {
        Case c;
        c.n_act = (int)col_toks.size();
        c.col0 = (int)cols.size();
        c.tok0 = (int)gpre.size();
        c.out0 = rows;
        int j = 0;
        for (int i = 0; i < c.n_act; ++i) {
            cols.push_back(QCol{i, j, j + col_toks[i], 0});
            j += col_toks[i];
        }
        if (c.n_act == 0) cols.push_back(QCol{0, 0, 0, 0});  // (col_tokens reads one column)
        uint32_t g = 0;
        for (int t = 0; t < j; ++t) { gpre.push_back(g); g += len[t]; }
        gpre.push_back(g);
        c.cap = j + c.n_act + 2;  // every round takes a token or finishes a column
        rows += c.cap;
        cases.push_back(c);
    }
};

int main() {
    Builder b;
    std::mt19937 rng(20250);
    const uint32_t CAP = (uint32_t)kRoundCap;
    const int n_acts[5] = {0, 1, 2, 47, 48}, col_lens[5] = {1, 63, 64, 65, 200};
    for (int n_act : n_acts)
        for (int L : col_lens)
            for (int pat = 0; pat < 6; ++pat) {
                std::vector<int> ct(n_act, L);
                const int nt = n_act * L;
                std::vector<uint32_t> len(nt, 1u);
                if (pat == 0) std::fill(len.begin(), len.end(), 0u);  // all-empty lists: F = 0 in every round
                // the first column ends a round exactly at the cap (2), one entry past it (3)
                if ((pat == 2 || pat == 3) && nt > 0) len[0] = CAP - (uint32_t)(L - 1) + (pat == 3 ? 1u : 0u);
                // a single token above the cap: the one-token overflow round
                if (pat == 4 && nt > 0) { std::fill(len.begin(), len.end(), 3u); len[nt / 2] = CAP + 7u; }
                if (pat == 5) for (auto& v : len) v = rng() % (2u * CAP / (uint32_t)L + 1u);
                b.add(ct, len);
            }
    for (int it = 0; it < 3000; ++it) {
        const int n_act = (int)(rng() % 49u);
        std::vector<int> ct(n_act);
        int nt = 0;
        for (auto& c : ct) {
            const uint32_t r = rng() % 16u;
            c = r < 10 ? 1 + (int)(rng() % 6u) : r < 13 ? 62 + (int)(rng() % 5u) : 1 + (int)(rng() % 200u);
            nt += c;
        }
        const uint32_t scales[5] = {1u, 4u, CAP / 64u, CAP / 8u, CAP + CAP / 4u};
        const uint32_t sc = scales[rng() % 5u], zero_in = 1u + rng() % 4u;
        std::vector<uint32_t> len(nt);
        for (auto& v : len) v = rng() % zero_in == 0u ? 0u : rng() % (sc + 1u);
        if (nt > 0 && it % 7 == 0) {  // a prefix that lands on the cap or just past it
            uint32_t s = 0;
            int t = 0;
            for (; t < nt - 1 && s + len[t] < CAP; ++t) s += len[t];
            len[t] = CAP - s + (uint32_t)(it % 3);
        }
        b.add(ct, len);
    }
    const int nc = (int)b.cases.size();
    Case* dc; QCol* dq; uint32_t* dg; int4 *ds, *dl; int *ns, *nl;
    CK(hipMalloc(&dc, nc * sizeof(Case)));
    CK(hipMalloc(&dq, b.cols.size() * sizeof(QCol)));
    CK(hipMalloc(&dg, b.gpre.size() * 4));
    CK(hipMalloc(&ds, (size_t)b.rows * sizeof(int4)));
    CK(hipMalloc(&dl, (size_t)b.rows * sizeof(int4)));
    CK(hipMalloc(&ns, nc * 4));
    CK(hipMalloc(&nl, nc * 4));
    CK(hipMemcpy(dc, b.cases.data(), nc * sizeof(Case), hipMemcpyHostToDevice));
    CK(hipMemcpy(dq, b.cols.data(), b.cols.size() * sizeof(QCol), hipMemcpyHostToDevice));
    CK(hipMemcpy(dg, b.gpre.data(), b.gpre.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(ds, 0xFF, (size_t)b.rows * sizeof(int4)));
    CK(hipMemset(dl, 0xEE, (size_t)b.rows * sizeof(int4)));
    CK(hipMemset(ns, 0xFF, nc * 4));
    CK(hipMemset(nl, 0xEE, nc * 4));
    probe<<<nc, 64>>>(dc, dq, dg, ds, dl, ns, nl);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<int4> hs(b.rows), hl(b.rows);
    std::vector<int> hns(nc), hnl(nc);
    CK(hipMemcpy(hs.data(), ds, (size_t)b.rows * sizeof(int4), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hl.data(), dl, (size_t)b.rows * sizeof(int4), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hns.data(), ns, nc * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hnl.data(), nl, nc * 4, hipMemcpyDeviceToHost));
    int bad = 0, max_rounds = 0, three = 0, splits = 0, empty = 0;
    long rounds = 0;
    for (int i = 0; i < nc; ++i) {
        const Case& c = b.cases[i];
        if (hns[i] != hnl[i] || hns[i] < 0 || hns[i] >= c.cap) {
            if (bad++ < 10) printf("case %d (n_act %d): rounds %d serial, %d lanes, cap %d\n", i, c.n_act, hns[i], hnl[i], c.cap);
            continue;
        }
        for (int r = 0; r < hns[i]; ++r) {
            const int4 s = hs[c.out0 + r], l = hl[c.out0 + r];
            if ((s.x != l.x || s.y != l.y || s.z != l.z || s.w != l.w) && bad++ < 10)
                printf("case %d (n_act %d) round %d: serial %d %d %d %d, lanes %d %d %d %d\n", i, c.n_act, r, s.x, s.y, s.z,
                       s.w, l.x, l.y, l.z, l.w);
            // a column shared by two rounds: this round's columns end past the next one's first
            if (r + 1 < hns[i] && s.w > hs[c.out0 + r + 1].z) ++splits;
        }
        rounds += hns[i];
        three += hns[i] >= 3;
        empty += hns[i] == 0;
        max_rounds = hns[i] > max_rounds ? hns[i] : max_rounds;
    }
    // non-trivial: cases of three or more rounds, split columns, and only the n_act = 0 cases without rounds
    if (three == 0 || splits == 0 || rounds == 0) { printf("trivial sweep\n"); ++bad; }
    printf("cases %d rounds %ld max_rounds %d three_plus %d splits %d no_rounds %d\n", nc, rounds, max_rounds, three, splits, empty);
    printf(bad ? "FAIL %d\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
