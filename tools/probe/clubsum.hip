// Device check of the clubs-by-interest stage (pf_clubsum.hip; links the product's build/pf_clubsum_k.o)
// on synthetic ranked keys and a synthetic club CSR, against the serial loop of the definition:
//     per club: double acc = 0; neighbours in rank order, w = (double)score, skipped when w <= 0;
//               acc += w per occurrence in the neighbour's list; score = (float)acc
//     list: (score desc, club id asc), cut to topk.
// Ids, counts and float bits must be equal.  Built with -ffp-contract=off like the product.
//   clubsum               the cases; one line each, a summary line "S ...", then OK
//   clubsum sweep         the cut-over sweep: wall time of the stage per cut-over on three shapes
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "pf_clubsum.h"
#include "pf_types.h"

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__);  \
            exit(2);                                                                       \
        }                                                                                  \
    } while (0)

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Case {
    std::string name;
    // the corpus: users[i] ascending, clubs[i] = dense indices in profile order
    std::vector<int32_t> users;
    std::vector<std::vector<int32_t>> clubs;
    std::vector<int32_t> club_id;  // dense -> id
    // the neighbours, unranked: (user index, score)
    std::vector<std::pair<int32_t, float>> nb;
    std::vector<int32_t> own;  // dense
    int64_t used = -1;         // -1: all
    int32_t topk = 10;
    int32_t cutover = 0;
};

struct DevCase {
    uint64_t* keys = nullptr;
    int32_t *uid = nullptr, *dense = nullptr, *club_id = nullptr;
    int64_t* off = nullptr;
    std::vector<uint64_t> hkeys;
    std::vector<int64_t> hoff;
    std::vector<int32_t> hdense;
    void free_all() {
        (void)hipFree(keys); (void)hipFree(uid); (void)hipFree(dense); (void)hipFree(club_id); (void)hipFree(off);
    }
};

template <class T>
T* up(const std::vector<T>& v) {
    T* p = nullptr;
    CK(hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)));
    if (!v.empty()) CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

DevCase upload(const Case& c) {
    DevCase d;
    for (auto& p : c.nb) d.hkeys.push_back(pf::score_key(p.second, c.users[(size_t)p.first]));
    std::sort(d.hkeys.begin(), d.hkeys.end());
    d.hoff.assign(c.users.size() + 1, 0);
    for (size_t i = 0; i < c.users.size(); ++i) {
        d.hoff[i + 1] = d.hoff[i] + (int64_t)c.clubs[i].size();
        d.hdense.insert(d.hdense.end(), c.clubs[i].begin(), c.clubs[i].end());
    }
    d.keys = up(d.hkeys);
    d.uid = up(c.users);
    d.dense = up(d.hdense);
    d.club_id = up(c.club_id);
    d.off = up(d.hoff);
    return d;
}

struct Ref {
    std::vector<int32_t> club;
    std::vector<float> score;
    int64_t contributions = 0, clubs = 0, long_runs = 0, max_run = 0, min_run = 0, ties = 0;
};

Ref reference(const Case& c, const DevCase& d, int64_t used, int cutover) {
    const size_t nc = c.club_id.size();
    std::vector<double> acc(nc, 0.0);
    std::vector<int64_t> n(nc, 0);
    std::vector<char> own(nc, 0);
    for (int32_t o : c.own) own[(size_t)o] = 1;
    Ref r;
    for (int64_t k = 0; k < used; ++k) {
        const double w = (double)pf::key_score(d.hkeys[(size_t)k]);
        if (w <= 0.0) continue;
        const int32_t u = pf::key_uid(d.hkeys[(size_t)k]);
        const size_t i = (size_t)(std::lower_bound(c.users.begin(), c.users.end(), u) - c.users.begin());
        for (int32_t x : c.clubs[i]) {
            if (own[(size_t)x]) continue;
            acc[(size_t)x] += w;
            ++n[(size_t)x];
            ++r.contributions;
        }
    }
    std::vector<uint64_t> keys;
    for (size_t x = 0; x < nc; ++x) {
        if (!n[x]) continue;
        ++r.clubs;
        if (n[x] >= cutover) ++r.long_runs;
        r.max_run = std::max(r.max_run, n[x]);
        r.min_run = r.min_run ? std::min(r.min_run, n[x]) : n[x];
        keys.push_back(pf::score_key((float)acc[x], c.club_id[x]));
    }
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i + 1 < keys.size(); ++i) r.ties += (keys[i] >> 32) == (keys[i + 1] >> 32);
    for (size_t i = 0; i < keys.size() && (int64_t)i < c.topk; ++i) {
        r.club.push_back(pf::key_uid(keys[i]));
        r.score.push_back(pf::key_score(keys[i]));
    }
    return r;
}

pf::ClubSumWs g_ws;
struct Totals {
    int64_t cases = 0, long_runs = 0, short_only = 0, ties = 0, own_cases = 0, contributions = 0, order_visible = 0,
            multi_block = 0, at_cut = 0;
} g_t;

pf::ClubSumIn make_in(const Case& c, const DevCase& d, int64_t used) {
    pf::ClubSumIn in{};
    in.keys = d.keys;
    in.used = used;
    in.uid = d.uid;
    in.n_users = (int32_t)c.users.size();
    in.n_club_ids = (int32_t)c.club_id.size();
    in.club_off = d.off;
    in.club_dense = d.dense;
    in.club_id = d.club_id;
    in.own = c.own.data();
    in.n_own = (int32_t)c.own.size();
    in.topk = c.topk;
    in.cutover = c.cutover;
    return in;
}

// runs the case and compares; returns the reference for the caller's own assertions
Ref run(const Case& c) {
    DevCase d = upload(c);
    const int64_t used = c.used < 0 ? (int64_t)d.hkeys.size() : std::min<int64_t>(c.used, (int64_t)d.hkeys.size());
    const int cut = c.cutover > 0 ? c.cutover : pf::kClubSumCutoverDefault;
    const Ref r = reference(c, d, used, cut);
    std::vector<int32_t> oc((size_t)std::max(c.topk, 1), -7);
    std::vector<float> os((size_t)std::max(c.topk, 1), -7.f);
    pf::ClubSumOut out;
    hipError_t err = hipSuccess;
    const auto t0 = std::chrono::steady_clock::now();
    const pf::ClubSumStatus st = pf::clubsum_run(make_in(c, d, used), g_ws, nullptr, oc.data(), os.data(), &out, &err);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    bool ok = st == pf::kClubSumOk && out.count == (int32_t)r.club.size() && out.contributions == r.contributions &&
              out.clubs == r.clubs && out.long_runs == r.long_runs;
    for (size_t i = 0; ok && i < r.club.size(); ++i)
        ok = oc[i] == r.club[i] && std::memcmp(&os[i], &r.score[i], 4) == 0;
    printf("case %s used %lld contributions %lld clubs %lld long %lld max_run %lld count %d ms %.3f %s\n", c.name.c_str(),
           (long long)used, (long long)out.contributions, (long long)out.clubs, (long long)out.long_runs, (long long)r.max_run,
           out.count, ms, ok ? "ok" : "MISMATCH");
    if (!ok) {
        printf("  status %d hip %s; want count %zu contributions %lld clubs %lld long %lld\n", (int)st, hipGetErrorString(err),
               r.club.size(), (long long)r.contributions, (long long)r.clubs, (long long)r.long_runs);
        for (size_t i = 0; i < r.club.size() && i < 8; ++i)
            printf("  [%zu] got %d %a want %d %a\n", i, oc[i], (double)os[i], r.club[i], (double)r.score[i]);
        exit(1);
    }
    ++g_t.cases;
    g_t.long_runs += out.long_runs;
    g_t.short_only += out.long_runs == 0 && out.clubs > 0;
    g_t.ties += r.ties;
    g_t.own_cases += !c.own.empty();
    g_t.contributions += out.contributions;
    g_t.multi_block += used > pf::kClubSumThreads;
    d.free_all();
    return r;
}

// n users with uids 10, 13, 16, ... and an identity club table of nc clubs
Case base(const std::string& name, int n, int nc) {
    Case c;
    c.name = name;
    for (int i = 0; i < n; ++i) c.users.push_back(10 + 3 * i);
    c.clubs.resize((size_t)n);
    for (int x = 0; x < nc; ++x) c.club_id.push_back(100 + x);
    return c;
}

// every user a neighbour with a score from a small set (ties in the club sums), 0..4 clubs of nc, with
// repeats, club-less users and users scoring 0 and -0.25
Case random_case(const std::string& name, int n, int nc, uint64_t seed) {
    Case c = base(name, n, nc);
    Rng g{seed};
    for (int i = 0; i < n; ++i) {
        const int k = (int)g.below(5);
        for (int j = 0; j < k; ++j) c.clubs[(size_t)i].push_back((int32_t)g.below((uint32_t)nc));
        if (k >= 2 && g.below(4) == 0) c.clubs[(size_t)i][1] = c.clubs[(size_t)i][0];  // listed twice
        const uint32_t t = g.below(16);
        const float s = t == 0 ? 0.0f : t == 1 ? -0.25f : 0.125f * (float)(1 + g.below(6));
        c.nb.push_back({i, s});
    }
    return c;
}

void cases() {
    // the stage's edges: nobody, one neighbour
    {
        Case c = random_case("nobody", 50, 20, 1);
        c.used = 0;
        run(c);
        Case e = base("one_neighbour", 3, 5);
        e.clubs[1] = {4, 2, 4};
        e.nb = {{1, 0.5f}};
        const Ref r = run(e);
        if (r.club.size() != 2 || r.club[0] != 104 || r.score[0] != 1.0f) { printf("one_neighbour: wrong reference\n"); exit(1); }
    }
    // contributions one below, at and one above a workgroup's scan width, by neighbours of one club each and by
    // fewer neighbours of several; used one below, at and one above it
    for (int n : {pf::kClubSumThreads - 1, pf::kClubSumThreads, pf::kClubSumThreads + 1}) {
        Case c = base("width_" + std::to_string(n), n, 7);
        for (int i = 0; i < n; ++i) {
            c.clubs[(size_t)i] = {i % 7};
            c.nb.push_back({i, 0.25f + 0.001f * (float)(i % 11)});
        }
        const Ref r = run(c);
        if (r.contributions != n) { printf("width: wrong reference\n"); exit(1); }
        Case m = base("width_sum_" + std::to_string(n), 100, 9);
        int left = n;
        for (int i = 0; i < 100 && left > 0; ++i) {
            const int k = std::min(left, i == 99 ? left : 1 + (i % 5));
            for (int j = 0; j < k; ++j) m.clubs[(size_t)i].push_back((i + 2 * j) % 9);
            left -= k;
            m.nb.push_back({i, 0.5f - 0.003f * (float)i});
        }
        const Ref r2 = run(m);
        if (r2.contributions != n) { printf("width_sum: wrong reference %lld\n", (long long)r2.contributions); exit(1); }
    }
    // several workgroups, every planted category of random_case; the cut applied at odd places
    for (int64_t used : {-1ll, 1ll, 64ll, 65ll, 1000ll}) {
        Case c = random_case("random_used_" + std::to_string(used), 3000, 60, 7);
        c.used = used;
        c.topk = used == 64 ? 100 : 10;  // topk above the clubs there are
        run(c);
    }
    // runs of exactly the cut-over and one either side, at the default and at two other cut-overs
    for (int cut : {0, 2, 64, 65}) {
        const int cv = cut ? cut : pf::kClubSumCutoverDefault;
        Case c = base("cutover_" + std::to_string(cv), 400, 8);
        c.cutover = cut;
        for (int i = 0; i < 400; ++i) {
            if (i < cv - 1) c.clubs[(size_t)i].push_back(0);
            if (i < cv) c.clubs[(size_t)i].push_back(1);
            if (i < cv + 1) c.clubs[(size_t)i].push_back(2);
            if (i % 3 == 0) c.clubs[(size_t)i].push_back(3 + i % 5);
            c.nb.push_back({i, 0.9f - 0.002f * (float)i});
        }
        const Ref r = run(c);
        if (r.long_runs < 2) { printf("cutover: wrong reference\n"); exit(1); }
        ++g_t.at_cut;
    }
    // one run of every neighbour (5,000: 79 wave steps, the last one partial), beside short ones
    {
        Case c = base("one_run", 5000, 40);
        Rng g{11};
        for (int i = 0; i < 5000; ++i) {
            c.clubs[(size_t)i] = {17};
            if (i % 50 == 0) c.clubs[(size_t)i].push_back((int32_t)g.below(40));
            c.nb.push_back({i, 1.0f / (float)(1 + g.below(1000))});
        }
        const Ref r = run(c);
        if (r.max_run < 5000) { printf("one_run: wrong reference\n"); exit(1); }
    }
    // every club distinct
    {
        Case c = base("all_distinct", 3000, 3000);
        for (int i = 0; i < 3000; ++i) {
            c.clubs[(size_t)i] = {2999 - i};
            c.nb.push_back({i, 0.001f * (float)(1 + i % 7)});
        }
        c.topk = 3000;
        const Ref r = run(c);
        if (r.clubs != 3000 || r.max_run != 1) { printf("all_distinct: wrong reference\n"); exit(1); }
    }
    // own lists of 0, 1 and 65,535 entries over 70,000 clubs
    for (int n_own : {0, 1, 65535}) {
        Case c = base("own_" + std::to_string(n_own), 2000, 70000);
        Rng g{5};
        for (int i = 0; i < 2000; ++i) {
            for (int j = 0; j < 6; ++j) c.clubs[(size_t)i].push_back((int32_t)g.below(70000));
            c.clubs[(size_t)i].push_back(69999);  // never own
            c.clubs[(size_t)i].push_back(3);      // own as soon as there is an own list
            c.nb.push_back({i, 0.01f * (float)(1 + g.below(90))});
        }
        for (int x = 0; x < n_own; ++x) c.own.push_back(n_own == 1 ? 3 : x);
        const Ref r = run(c);
        const bool has3 = std::find(r.club.begin(), r.club.end(), 103) != r.club.end();
        if (has3 != (n_own == 0) || r.club.empty() || r.club[0] != (n_own == 0 ? 103 : 100 + 69999)) {
            printf("own: wrong reference\n");
            exit(1);
        }
    }
    // club ids up to 2^30 - 1 whose dense order is not id order
    {
        Case c = random_case("big_ids", 1500, 64, 23);
        for (int x = 0; x < 64; ++x) c.club_id[(size_t)x] = (int32_t)(((1u << 30) - 1u) - 16777259u * (uint32_t)((x * 37) % 64));
        const Ref r = run(c);
        if (*std::max_element(c.club_id.begin(), c.club_id.end()) != (1 << 30) - 1) { printf("big_ids: wrong ids\n"); exit(1); }
        (void)r;
    }
    // the order made visible.  (a) as stated: 1.0f, then 200 neighbours of 2^-60f: in rank order every small add is
    // lost and the double is exactly 1.0.  (b) the same with a neighbour of 2^-24f in second place: in rank order the
    // double stays 1 + 2^-24, which rounds to even, 1.0f; any sum that first gathers the small ones lands above the
    // midpoint and rounds to 1 + 2^-23f.  On both paths: run above and below the cut-over.
    for (int cut : {0, 1000}) {
        for (int mid : {0, 1}) {
            Case c = base(std::string("order_") + (mid ? "b" : "a") + (cut ? "_short" : "_long"), 300, 4);
            c.cutover = cut;
            c.clubs[0] = {2};
            c.nb.push_back({0, 1.0f});
            if (mid) {
                c.clubs[1] = {2};
                c.nb.push_back({1, std::ldexp(1.0f, -24)});
            }
            for (int i = 0; i < 200; ++i) {
                c.clubs[(size_t)(10 + i)] = {2};
                c.nb.push_back({10 + i, std::ldexp(1.0f, -60)});
            }
            const Ref r = run(c);
            double tree = 200.0 * std::ldexp(1.0, -60) + (mid ? std::ldexp(1.0, -24) : 0.0) + 1.0;
            if (r.score.size() != 1 || r.score[0] != 1.0f || !(tree > 1.0) || (mid && (float)tree == 1.0f)) {
                printf("order: wrong reference\n");
                exit(1);
            }
            g_t.order_visible += mid;
        }
    }
    printf("S cases %lld long_runs %lld short_only %lld ties %lld own_cases %lld at_cut %lld multi_block %lld order_visible %lld\n",
           (long long)g_t.cases, (long long)g_t.long_runs, (long long)g_t.short_only, (long long)g_t.ties, (long long)g_t.own_cases,
           (long long)g_t.at_cut, (long long)g_t.multi_block, (long long)g_t.order_visible);
}

// wall time of the stage (its three synchronisations included) per cut-over: the median of 15 after 3 warm-ups
void sweep() {
    struct Shape { const char* name; int n, nc, hot; };
    // hot: every hot-th neighbour also lists club 0 (one long run) on top of 0..4 random clubs
    const Shape shapes[] = {{"n100", 100, 5000, 2}, {"n10000", 10000, 50000, 2}, {"n200000", 200000, 200000, 1}};
    for (const Shape& sh : shapes) {
        Case c = random_case(sh.name, sh.n, sh.nc, 99);
        for (int i = 0; i < sh.n; i += sh.hot) c.clubs[(size_t)i].push_back(0);
        DevCase d = upload(c);
        std::vector<int32_t> oc(10);
        std::vector<float> os(10);
        for (int cut : {4, 8, 16, 32, 64, 128, 256, 1 << 30}) {
            c.cutover = cut;
            std::vector<double> ms;
            pf::ClubSumOut out;
            for (int it = 0; it < 18; ++it) {
                hipError_t err;
                const auto t0 = std::chrono::steady_clock::now();
                if (pf::clubsum_run(make_in(c, d, (int64_t)d.hkeys.size()), g_ws, nullptr, oc.data(), os.data(), &out, &err) !=
                    pf::kClubSumOk) {
                    printf("sweep: stage failed\n");
                    exit(1);
                }
                if (it >= 3) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            printf("sweep %s cutover %d contributions %lld clubs %lld long %lld median_ms %.4f min_ms %.4f max_ms %.4f\n", sh.name, cut,
                   (long long)out.contributions, (long long)out.clubs, (long long)out.long_runs, ms[ms.size() / 2], ms.front(),
                   ms.back());
        }
        d.free_all();
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "sweep") == 0) {
        sweep();
    } else {
        cases();
    }
    printf("OK\n");
    return 0;
}
