// Device check of the job pipeline's kernels (pf_jobs.hip), each as an operation on synthetic plans of
// this probe's own making against a plain serial host loop.  Links the product's own object
// (build/pf_jobs_k.o) and calls its launchers (pf_jobs.h) with plain device pointers:
//   A  K3 gather_kernel, all six kinds: rounds of 2 x 1024 positions, the friend-segment scan's trips
//      of 1024, limits at a round's edge, duplicates, views, hash clusters, the counting-sort path;
//   B  K9 expand_pairs_kernel, order_pairs_kernel and slot_class through it;
//   C  K4' collab_kernel: the double sums bit for bit on inputs whose float result depends on the
//      summation order, and the fused top-k hand-off (and K8 for a job with topk > 64);
//   D  K7 clubs_kernel: every club's sum in the stream order, acc left zero;
//   E  K8 topk_kernel.
// K6 (qimage_kernel) has a probe of its own (qimage.hip); pair_stats_kernel is not here.  Prints one summary line per part and OK;
// at the first HIP error or mismatch it prints FAIL ... and exits 1 without another launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <unordered_set>
#include <vector>

#include "pf_jobs.h"
#include "pf_types.h"
using namespace pf;

#define FAIL(...) do { printf("FAIL "); printf(__VA_ARGS__); printf("\n"); fflush(stdout); exit(1); } while (0)
#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) FAIL("%s: %s", #x, hipGetErrorString(e_)); } while (0)
#define SYNC(x) do { CK(x); CK(hipDeviceSynchronize()); } while (0)

static const int32_t SENT = 0x5A5A5A5A;  // every output buffer starts as bytes of 0x5A
static const uint64_t SENT64 = 0x5A5A5A5A5A5A5A5Aull;
static const uint64_t NONE = ~0ull;
static std::mt19937_64 rng(20261);
static int64_t rnd(int64_t n) { return (int64_t)(rng() % (uint64_t)n); }  // [0, n)
static float frand(float lo, float hi) { return lo + (hi - lo) * (float)((rng() >> 40) + 1) / 16777218.0f; }  // (lo, hi)
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static std::vector<void*> g_dev;
template <class T> static T* dalloc(size_t n, int byte = 0x5A) {
    T* p;
    const size_t b = std::max<size_t>(n, 1) * sizeof(T);
    CK(hipMalloc((void**)&p, b));
    CK(hipMemset(p, byte, b));
    g_dev.push_back(p);
    return p;
}
template <class T> static T* up(const std::vector<T>& v) {
    T* p = dalloc<T>(v.size(), 0);
    if (!v.empty()) CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}
template <class T> static std::vector<T> down(const T* p, size_t n) {
    std::vector<T> v(n);
    if (n) CK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}
static void free_all() {
    for (void* p : g_dev) CK(hipFree(p));
    g_dev.clear();
}

// ================================================================ the synthetic store
// Nodes [0, n) are profiles, [n, M) have none.  g_uid differs from the node number and slot_of is a
// permutation with no fixed structure the kernels could lean on.
static int32_t uid_of(int32_t x) { return 3 * x + 7; }
static int32_t node_of_uid(int32_t id) { return (id - 7) / 3; }

struct Graph {
    int32_t n = 0, M = 0;
    std::vector<std::vector<int32_t>> row;
    std::vector<int32_t> len, uid, slot_of;  // len -1: no row
    std::vector<std::vector<int32_t>> clubs;  // [n] dense club indices
    std::vector<int32_t> club_id;
    void init(int32_t n_, int32_t M_, int32_t nclubs) {
        n = n_;
        M = M_;
        row.assign(M, {});
        len.assign(M, -1);
        uid.resize(M);
        slot_of.resize(n);
        clubs.assign(n, {});
        for (int32_t x = 0; x < M; ++x) uid[x] = uid_of(x);
        for (int32_t i = 0; i < n; ++i) slot_of[i] = (int32_t)(((int64_t)i * 48271 + 12345) % n);
        std::vector<char> hit(n, 0);
        for (int32_t i = 0; i < n; ++i) {
            if (hit[slot_of[i]]) FAIL("slot_of is no permutation");
            hit[slot_of[i]] = 1;
        }
        club_id.resize(nclubs);
        for (int32_t d = 0; d < nclubs; ++d) club_id[d] = 5 * d + 11;
    }
    void set_row(int32_t x, std::vector<int32_t> r) {
        len[x] = (int32_t)r.size();
        row[x] = std::move(r);
    }
    DevJobsStore upload() const {  // the K6 members stay null
        std::vector<int64_t> off(M), coff(n + 1, 0);
        std::vector<int32_t> nbr, cd;
        for (int32_t x = 0; x < M; ++x) {
            off[x] = (int64_t)nbr.size();
            nbr.insert(nbr.end(), row[x].begin(), row[x].end());
        }
        for (int32_t i = 0; i < n; ++i) {
            cd.insert(cd.end(), clubs[i].begin(), clubs[i].end());
            coff[i + 1] = (int64_t)cd.size();
        }
        DevJobsStore s{};
        s.slot_of = up(slot_of);
        s.g_off = up(off);
        s.g_len = up(len);
        s.g_nbr = up(nbr);
        s.g_uid = up(uid);
        s.n = n;
        s.M = M;
        s.club_off = up(coff);
        s.club_dense = up(cd);
        s.club_id = up(club_id);
        s.n_club_ids = (int32_t)club_id.size();
        return s;
    }
};

struct VEntry { int32_t node, ver, len; std::vector<int32_t> row; };
struct View {
    std::vector<VEntry> e;
    DevView upload() {
        std::sort(e.begin(), e.end(), [](const VEntry& a, const VEntry& b) { return a.node != b.node ? a.node < b.node : a.ver > b.ver; });
        std::vector<int32_t> node, ver, len, nbr;
        std::vector<int64_t> off;
        for (const VEntry& x : e) {
            node.push_back(x.node);
            ver.push_back(x.ver);
            len.push_back(x.len);
            off.push_back((int64_t)nbr.size());
            nbr.insert(nbr.end(), x.row.begin(), x.row.end());
        }
        DevView v{};
        v.node = up(node);
        v.ver = up(ver);
        v.off = up(off);
        v.len = up(len);
        v.nbr = up(nbr);
        v.n = (int32_t)e.size();
        return v;
    }
};

// What a job sees of node x's row: its own row, else the newest override with ver <= its version,
// else the base row.  Returns the length (-1: none).
struct JobRows { int32_t version = 0, own = -1, own_len = -1; std::vector<int32_t> own_row; };
static int32_t h_row(const Graph& g, const View& v, const JobRows& j, int32_t x, const int32_t*& p) {
    p = nullptr;
    if (j.own >= 0 && x == j.own) { p = j.own_row.data(); return j.own_len; }
    const VEntry* best = nullptr;
    for (const VEntry& e : v.e)
        if (e.node == x && e.ver <= j.version && (!best || e.ver > best->ver)) best = &e;
    if (best) { p = best->row.data(); return best->len; }
    if (x < 0 || x >= g.M) return -1;
    p = g.row[x].data();
    return g.len[x];
}

// slot_class restated from its comment: classes 0..7 are slots 0..7, then eight classes per power of
// two of the slot, by the three bits under its leading one
static int h_slot_class(int32_t s) {
    if (s < 8) return s;
    int lg = 0;
    while ((s >> (lg + 1)) > 0) ++lg;
    return 8 + 8 * (lg - 3) + ((s >> (lg - 3)) & 7);
}

// ================================================================ A: K3 gather
struct AJob {
    std::string cat;
    int kind;
    int32_t u;
    std::vector<int32_t> F;
    int32_t L;
    JobRows jr;
};
struct ARef {
    std::vector<int32_t> kept;  // nodes, in order
    int64_t total = 0;
    int F1 = 0, rounds = 0;
};
static const int kRound = 2048;  // K3's round: 2 x 1024 positions

static std::vector<int32_t> a_seq(const Graph& g, const View& v, const AJob& j, bool graph) {
    std::vector<int32_t> s;
    for (int32_t f : j.F) {
        const int32_t* p;
        const int32_t l = h_row(g, v, j.jr, f, p);
        if (graph) {
            if (f == j.u) continue;  // the whole segment is skipped
            s.push_back(f);
        }
        for (int32_t k = 0; k < l; ++k) s.push_back(p[k]);
    }
    return s;
}

static ARef a_ref(const Graph& g, const View& v, const AJob& j) {
    const bool graph = j.kind == kDjInterest || j.kind == kDjRawGraph;
    const bool raw = j.kind == kDjRawGraph || j.kind == kDjRawCollab;
    const std::vector<int32_t> s = a_seq(g, v, j, graph);
    ARef r;
    r.total = (int64_t)s.size();
    std::unordered_set<int32_t> seen, excl;
    if (j.kind == kDjInterest) {
        excl.insert(j.F.begin(), j.F.end());
        excl.insert(j.u);
    }
    int cnt = 0;
    bool open = true;  // the kernel still walks rounds
    for (int64_t p = 0; p < r.total; ++p) {
        if (p % kRound == 0) {
            if (cnt >= j.L) open = false;
            if (open) ++r.rounds;
        }
        const int32_t x = s[p];
        if (x == j.u || !seen.insert(x).second) continue;
        if (p < kRound) ++r.F1;
        if (cnt >= j.L) continue;
        ++cnt;  // counts against the limit whether or not it is kept
        if (raw || (x < g.n && !excl.count(x))) r.kept.push_back(x);
    }
    return r;
}

static std::vector<int32_t> distinct_profiles(const Graph& g, const std::vector<int32_t>& F) {
    std::vector<int32_t> fd;
    for (int32_t f : F)
        if (f >= 0 && f < g.n && std::find(fd.begin(), fd.end(), f) == fd.end()) fd.push_back(f);
    return fd;
}

static void part_a() {
    Graph g;
    g.init(100000, 131072, 16);
    View view;
    std::vector<AJob> jobs;
    std::map<std::string, int> cat;
    int32_t next_p = 1000, next_np = g.n + 100;
    auto fresh = [&](bool profile) { return profile ? next_p++ : next_np++; };
    auto target = [&]() { return (int32_t)rnd(g.M); };
    auto limits = [&](int64_t total, int F1) {
        std::set<int32_t> L;
        for (int64_t l : {(int64_t)1, total - 1, total, total + 1, (int64_t)F1 - 1, (int64_t)F1, (int64_t)F1 + 1})
            if (l >= 1) L.insert((int32_t)l);
        return L;
    };
    // a scenario's jobs: every kind of its flavour at the seven limits around its total and F1
    auto add = [&](const std::string& c, int32_t u, const std::vector<int32_t>& F, bool graph, const JobRows& jr = JobRows(),
                   const std::set<int32_t>* only = nullptr) {
        for (int kind : {graph ? (int)kDjRawGraph : (int)kDjRawCollab, graph ? (int)kDjInterest : (int)kDjCollab}) {
            AJob j{c, kind, u, F, INT32_MAX, jr};
            const ARef all = a_ref(g, view, j);
            const std::set<int32_t> Ls = only ? *only : limits(all.total, all.F1);
            for (int32_t L : Ls) {
                j.L = L;
                jobs.push_back(j);
                ++cat[c];
            }
        }
    };
    // friends with rows of the given lengths (-1: no row) over random targets
    auto friends = [&](const std::vector<int32_t>& lens) {
        std::vector<int32_t> F;
        for (size_t i = 0; i < lens.size(); ++i) {
            const int32_t f = fresh(i % 7 != 3);
            F.push_back(f);
            if (lens[i] >= 0) {
                std::vector<int32_t> r(lens[i]);
                for (auto& x : r) x = target();
                g.set_row(f, r);
            }
        }
        return F;
    };
    // nf friends whose sequence has `total` positions in the given flavour
    auto spread = [&](int nf, int64_t total, bool graph) {
        const int64_t S = graph ? total - nf : total;
        if (S < 0) FAIL("scenario: total below nf");
        std::vector<int32_t> lens(nf);
        for (int i = 0; i < nf; ++i) {
            lens[i] = (int32_t)(S / nf + (i < S % nf));
            if (lens[i] == 0 && (i & 1)) lens[i] = -1;
        }
        return friends(lens);
    };
    const std::set<int32_t> three = {1, 1000, 1 << 20};
    for (int graph = 0; graph < 2; ++graph) {
        // the segment scan's trips of 1024 and its carry: rows of one element each
        for (int nf : {0, 1, 2, 1023, 1024, 1025, 2049}) add("nf_sweep", fresh(true), spread(nf, graph ? 2 * nf : nf, graph), graph, JobRows(), &three);
        // the rounds of 2048 positions
        for (int64_t total : {1, 2047, 2048, 2049, 4095, 4096, 4097, 10007})
            add("total_sweep", fresh(true), spread(total < 3 ? 1 : 3, total, graph), graph);
    }
    {  // total 0 in both flavours
        const int32_t u = fresh(true);
        add("total_sweep", u, {u, u}, true);
        add("total_sweep", fresh(true), friends({-1, 0}), false);
    }
    {  // duplicates
        const int32_t a = 70001, b = 70002, c = 70003, d = 70004, e = 70005;
        const int32_t f = fresh(true);
        g.set_row(f, std::vector<int32_t>(5000, a));
        for (int graph = 0; graph < 2; ++graph) add("dups", fresh(true), {f}, graph);
        std::vector<int32_t> E(6000);
        for (size_t i = 0; i < E.size(); ++i) E[i] = 71000 + (int32_t)i;  // otherwise distinct
        E[0] = E[5999] = a;        // position 0 and the last one
        E[100] = E[2148] = b;      // round 0 and round 1
        E[2548] = E[4596] = c;     // round 1 and round 2
        E[10] = E[1034] = d;       // p and p + 1024 of round 0
        E[2055] = E[3079] = e;     // p and p + 1024 of round 1
        std::vector<int32_t> F;
        for (int i = 0; i < 3; ++i) {
            F.push_back(fresh(true));
            g.set_row(F.back(), std::vector<int32_t>(E.begin() + 2000 * i, E.begin() + 2000 * (i + 1)));
        }
        for (int graph = 0; graph < 2; ++graph) add("dups", fresh(true), F, graph);
    }
    {  // the query node and row lengths
        const int32_t u = fresh(true), a = fresh(true), b = fresh(true), c = fresh(false), d = fresh(true), e = fresh(true), h = fresh(true);
        g.set_row(u, {a, 72001, 72002});
        g.set_row(a, {72003, u, 72004, u});
        g.set_row(c, {});         // b has no row, c and e and h have empty ones
        g.set_row(d, {u, 72005, 72003});
        g.set_row(e, {});
        g.set_row(h, {});
        // leading, inner and trailing empty segments: a trailing one is u in the graph flavour, an empty row in the other
        for (int graph = 0; graph < 2; ++graph) {
            add("rowlens", u, {c, a, u, b, c, a, d, e, h, u, u}, graph);
            add("rowlens", u, {c, a, u, b, c, a, d, u, e, h}, graph);
        }
    }
    {  // nodes without a profile: kept in raw lists, dropped but counted elsewhere
        const int32_t f = fresh(true), q = fresh(false), np1 = g.n + 1, np2 = g.n + 2, np3 = g.n + 3;
        g.set_row(f, {np1, np2, 73001, np3, 73002, 73003});
        g.set_row(q, {np3, 73004, np1});  // a node without a profile with a row of its own
        const std::set<int32_t> Ls = {2, 3, 4, 5, 100};
        for (int graph = 0; graph < 2; ++graph) add("noprofile", fresh(true), {f, q}, graph, JobRows(), &Ls);
    }
    {  // interest: members of row(u) and u are dropped but counted; then every candidate excluded
        const int32_t u = fresh(true), f = fresh(true), e1 = fresh(true);
        g.set_row(f, {e1, 74001, u, e1, 74002, 74003});
        const std::set<int32_t> Ls = {1, 2, 3, 4, 5, 100};
        add("interest_excl", u, {f, e1}, true, JobRows(), &Ls);
        const int32_t v = fresh(true), a = fresh(true), b = fresh(true), c = fresh(true);
        g.set_row(a, {b, c, v});
        g.set_row(b, {a, c});
        g.set_row(c, {a, b, v, v});
        add("interest_excl", v, {a, b, c}, true, JobRows(), &Ls);
    }
    {  // views
        const int32_t X = fresh(true), Y = fresh(true), Z = fresh(true), W = fresh(true), Q = fresh(true);
        auto r = [&](int n0) { std::vector<int32_t> v(n0); for (auto& x : v) x = target(); return v; };
        g.set_row(X, r(5));
        g.set_row(Y, r(6));
        g.set_row(Z, r(7));
        g.set_row(W, r(8));
        g.set_row(Q, r(9));
        view.e.push_back(VEntry{Y, 5, 11, r(11)});
        view.e.push_back(VEntry{X, INT32_MIN, 3, r(3)});  // visible to all
        view.e.push_back(VEntry{Y, 9, 13, r(13)});        // two versions of Y
        view.e.push_back(VEntry{Z, INT32_MIN, -1, {}});   // erased
        const std::vector<int32_t> F = {X, Y, Z, W, Q};
        for (int32_t ver : {0, 4, 5, 7, 9, 100}) {
            JobRows jr;
            jr.version = ver;
            for (int graph = 0; graph < 2; ++graph) add("views", fresh(true), F, graph, jr);
        }
        JobRows own;
        own.version = 7;
        own.own = W;
        own.own_row = r(17);
        own.own_len = 17;
        for (int graph = 0; graph < 2; ++graph) add("views", fresh(true), F, graph, own);
        own.own_row.clear();
        own.own_len = -1;  // the own row erased
        for (int graph = 0; graph < 2; ++graph) add("views", fresh(true), F, graph, own);
        own.own = X;  // the own row wins over the override
        own.own_row = r(4);
        own.own_len = 4;
        for (int graph = 0; graph < 2; ++graph) add("views", fresh(true), F, graph, own);
    }
    int clusters = 0, wrap = 0;
    {  // hash placement: nodes sharing one home slot, and a cluster at the table's last slot
        const int lg = gather_ht_lg(false, 3, 64);
        const uint32_t mask = (1u << lg) - 1u;
        auto home = [&](int32_t x) { return (((uint32_t)x * 0x9E3779B1u) >> 7) & mask; };
        std::vector<std::vector<int32_t>> by(mask + 1);
        for (int32_t x = 0; x < g.M; ++x)  // by brute force, over nodes without a row that no later scenario takes
            if (g.len[x] < 0 && (x < next_p || x >= next_p + 100) && (x < next_np || x >= next_np + 100)) by[home(x)].push_back(x);
        uint32_t h0 = 1;
        for (uint32_t h = 1; h < mask; ++h)
            if (by[h].size() > by[h0].size()) h0 = h;
        auto take = [&](uint32_t h, size_t first, size_t k) {
            if (by[h].size() < first + k) FAIL("hash: home slot %u has %zu nodes, %zu wanted", h, by[h].size(), first + k);
            return std::vector<int32_t>(by[h].begin() + first, by[h].begin() + first + k);
        };
        std::vector<int32_t> row;
        for (uint32_t h : {h0, mask}) {  // at least 8 members each
            const std::vector<int32_t> c = take(h, 0, 8);
            row.insert(row.end(), c.begin(), c.end());
            ++clusters;
            wrap += h == mask;
        }
        for (uint32_t h : {0u, 1u}) {  // where the wrapped probes land
            const std::vector<int32_t> c = take(h, 0, 2);
            row.insert(row.end(), c.begin(), c.end());
        }
        std::shuffle(row.begin(), row.end(), rng);
        const std::vector<int32_t> last = take(mask, 8, 2);
        const int32_t f = fresh(true);
        g.set_row(f, row);
        const std::vector<int32_t> F = {f, last[0], last[1]};  // exclusions claimed in the cluster first
        const std::set<int32_t> Ls = {1 << 20};
        const size_t j0 = jobs.size();
        for (int graph = 0; graph < 2; ++graph) add("hash", fresh(true), F, graph, JobRows(), &Ls);
        for (size_t i = j0; i < jobs.size(); ++i) {
            const ARef r = a_ref(g, view, jobs[i]);
            if (gather_ht_lg(false, (int64_t)jobs[i].F.size(), std::min<int64_t>(jobs[i].L, r.total)) != lg) FAIL("hash: the clusters were built for another table size");
        }
    }
    // the counting-sort path: nk at 64, 65 and 2048
    for (int nk : {64, 65, 2048}) {
        const int32_t f = fresh(true);
        std::vector<int32_t> r(nk);
        for (int i = 0; i < nk; ++i) r[i] = 40000 + 13 * i + nk;
        std::shuffle(r.begin(), r.end(), rng);
        g.set_row(f, r);
        const std::set<int32_t> Ls = {1 << 20};
        for (int graph = 0; graph < 2; ++graph) add("nk", fresh(true), {f}, graph, JobRows(), &Ls);
    }
    // every candidate: no exclusions, a three-friend row, a longer row with the user and a node without a profile
    for (int nf : {0, 3, 40}) {
        const int32_t u = 500 + nf;
        std::vector<int32_t> F;
        for (int i = 0; i < nf; ++i) F.push_back(i == 7 ? u : i == 9 ? g.n + 5 : (int32_t)rnd(g.n));
        jobs.push_back(AJob{"all", kDjAll, u, F, 1, JobRows()});
        ++cat["all"];
    }
    {  // clubs: the sim slots and the sreg regions
        const int32_t u = fresh(true), a = fresh(true), b = fresh(true), c = fresh(true);
        g.set_row(a, {u, 75001, g.n + 9, 75002, u});
        g.set_row(b, {});
        for (int i = 0; i < 1500; ++i) g.row[c].push_back(target());
        g.len[c] = 1500;
        std::vector<int32_t> F = {a, g.n + 7, b, c, a, fresh(true)};
        for (const VEntry& e : view.e)
            if (e.len < 0) F.push_back(e.node);  // an erased row
        jobs.push_back(AJob{"clubs", kDjClubs, u, F, 1, JobRows()});
        jobs.push_back(AJob{"clubs", kDjClubs, fresh(true), {}, 1, JobRows()});
        cat["clubs"] += 2;
    }

    // ---- lay the jobs out the way the planner does
    const int nj = (int)jobs.size();
    std::vector<DevJob> dj(nj);
    std::vector<ARef> ref(nj);
    std::vector<int32_t> pool(1, 0);
    std::vector<int64_t> pool64(1, 0);
    int64_t HT = 0, SEQ = 0, E = 0;
    int multi_round = 0, edge_limit = 0, sort_path = 0;
    std::vector<std::vector<int32_t>> fds(nj);
    for (int i = 0; i < nj; ++i) {
        const AJob& j = jobs[i];
        DevJob& d = dj[i];
        memset(&d, 0, sizeof d);
        d.kind = j.kind;
        d.u = j.u;
        d.L = j.L;
        d.version = j.jr.version;
        d.own = j.jr.own;
        d.own_len = j.jr.own_len;
        d.own_off = (int64_t)pool.size();
        pool.insert(pool.end(), j.jr.own_row.begin(), j.jr.own_row.end());
        d.f_off = (int64_t)pool.size();
        pool.insert(pool.end(), j.F.begin(), j.F.end());
        d.nf = (int32_t)j.F.size();
        for (int32_t f : j.F)
            if (f < 0 || f >= g.M) FAIL("A job %d: friend outside the graph", i);
        if (j.kind == kDjCollab || j.kind == kDjClubs) {
            fds[i] = distinct_profiles(g, j.F);
            d.nfd = (int32_t)fds[i].size();
            d.fd_off = (int64_t)pool.size();
            pool.insert(pool.end(), fds[i].begin(), fds[i].end());
            d.sim_off = E;
            E += d.nfd;
        }
        if (j.kind == kDjClubs) {
            d.sreg_off = (int64_t)pool64.size();
            for (int32_t f : fds[i]) {
                const int32_t* p;
                const int32_t l = h_row(g, view, j.jr, f, p);
                pool64.push_back(E);
                E += std::max(l, 0);
            }
            continue;
        }
        if (j.kind == kDjAll) {
            d.cap = g.n;
            d.ht_lg = gather_ht_lg(true, d.nf, d.cap);
        } else {
            ref[i] = a_ref(g, view, j);
            d.cap = (int32_t)std::min<int64_t>(j.L, ref[i].total);
            d.ht_lg = gather_ht_lg(false, d.nf, d.cap);
            multi_round += ref[i].rounds > 1;
            edge_limit += ref[i].total > kRound && j.L >= ref[i].F1 - 1 && j.L <= ref[i].F1 + 1;
            if ((int64_t)ref[i].kept.size() > d.cap) FAIL("A job %d: the reference keeps more than cap", i);
        }
        d.ht_off = HT;
        HT += 3ll << d.ht_lg;
        d.seg_off = SEQ;
        SEQ += d.nf + 1;
        d.cand_off = E;
        E += d.cap;
    }
    // ---- what the kernel must leave
    std::vector<int32_t> xs(E, SENT), xi(E, SENT), xn(nj, SENT);
    for (int i = 0; i < nj; ++i) {
        const AJob& j = jobs[i];
        const DevJob& d = dj[i];
        for (int r = 0; r < d.nfd; ++r) xs[d.sim_off + r] = g.slot_of[fds[i][r]];
        if (j.kind == kDjClubs) {
            for (int r = 0; r < d.nfd; ++r) {
                const int32_t* p;
                const int32_t l = h_row(g, view, j.jr, fds[i][r], p);
                for (int k = 0; k < l; ++k) xs[pool64[d.sreg_off + r] + k] = (p[k] != j.u && p[k] >= 0 && p[k] < g.n) ? g.slot_of[p[k]] : -1;
            }
            continue;
        }
        if (j.kind == kDjAll) {
            std::unordered_set<int32_t> ex(j.F.begin(), j.F.end());
            ex.insert(j.u);
            for (int32_t c = 0; c < d.cap; ++c) {
                xs[d.cand_off + c] = ex.count(c) ? -1 : g.slot_of[c];
                xi[d.cand_off + c] = ex.count(c) ? -1 : g.uid[c];
            }
            xn[i] = d.cap;
            continue;
        }
        const bool raw = j.kind == kDjRawGraph || j.kind == kDjRawCollab;
        const int nk = (int)ref[i].kept.size();
        for (int c = 0; c < d.cap; ++c) {
            xs[d.cand_off + c] = c < nk ? (raw ? 0 : g.slot_of[ref[i].kept[c]]) : -1;
            xi[d.cand_off + c] = c < nk ? g.uid[ref[i].kept[c]] : -1;
        }
        xn[i] = nk;
    }
    // ---- run
    const DevJobsStore ds = g.upload();
    const DevView dv = view.upload();
    DevJob* d_jobs = up(dj);
    int32_t* d_pool = up(pool);
    int64_t* d_pool64 = up(pool64);
    int32_t* d_ht = dalloc<int32_t>(HT);
    int32_t* d_seq = dalloc<int32_t>(SEQ);
    int32_t* d_slot = dalloc<int32_t>(E);
    int32_t* d_id = dalloc<int32_t>(E);
    int32_t* d_ncand = dalloc<int32_t>(nj);
    const DevStore st{};
    const CandFilter filt{};
    SYNC(launch_gather(ds, dv, d_jobs, nj, d_pool, d_pool64, d_ht, d_seq, d_slot, d_id, d_ncand, st, filt, nullptr));
    std::vector<int32_t> gs = down(d_slot, E), gi = down(d_id, E);
    const std::vector<int32_t> gn = down(d_ncand, nj);
    for (int i = 0; i < nj; ++i) {
        const AJob& j = jobs[i];
        const DevJob& d = dj[i];
        if (gn[i] != xn[i]) FAIL("A %s job %d kind %d L %d: ncand %d want %d", j.cat.c_str(), i, j.kind, j.L, gn[i], xn[i]);
        if ((j.kind == kDjInterest || j.kind == kDjCollab) && xn[i] > 64) {
            // the order is free: the same pairs, grouped by class, every pair still matched
            ++sort_path;
            std::vector<std::pair<int32_t, int32_t>> got, want;
            for (int c = 0; c < xn[i]; ++c) {
                const int32_t s = gs[d.cand_off + c], id = gi[d.cand_off + c];
                got.emplace_back(s, id);
                want.emplace_back(xs[d.cand_off + c], xi[d.cand_off + c]);
                const int32_t x = node_of_uid(id);
                if (id < 7 || (id - 7) % 3 || x >= g.n || s != g.slot_of[x]) FAIL("A %s job %d: pair (%d, %d) at %d is not a slot and its id", j.cat.c_str(), i, s, id, c);
                if (c && h_slot_class(gs[d.cand_off + c - 1]) > h_slot_class(s)) FAIL("A %s job %d: slot class falls at %d", j.cat.c_str(), i, c);
            }
            std::sort(got.begin(), got.end());
            std::sort(want.begin(), want.end());
            if (got != want) FAIL("A %s job %d kind %d L %d: the sorted list holds other pairs", j.cat.c_str(), i, j.kind, j.L);
            for (int c = 0; c < xn[i]; ++c) {
                gs[d.cand_off + c] = xs[d.cand_off + c];
                gi[d.cand_off + c] = xi[d.cand_off + c];
            }
        }
    }
    for (int64_t e = 0; e < E; ++e)
        if (gs[e] != xs[e] || gi[e] != xi[e]) {
            int at = -1;
            for (int i = 0; i < nj; ++i)
                if (jobs[i].kind != kDjClubs && e >= dj[i].cand_off && e < dj[i].cand_off + dj[i].cap) at = i;
            if (at >= 0)
                FAIL("A %s job %d kind %d L %d nf %d total %lld: entry %lld of %d is (%d, %d) want (%d, %d)", jobs[at].cat.c_str(), at, jobs[at].kind,
                     jobs[at].L, dj[at].nf, (long long)ref[at].total, (long long)(e - dj[at].cand_off), dj[at].cap, gs[e], gi[e], xs[e], xi[e]);
            FAIL("A: word %lld (a sim slot or an sreg region) is (%d, %d) want (%d, %d)", (long long)e, gs[e], gi[e], xs[e], xi[e]);
        }
    printf("A jobs %d nf_sweep %d total_sweep %d dups %d rowlens %d noprofile %d interest_excl %d views %d hash %d nk %d all %d clubs %d "
           "multi_round %d edge_limit %d clusters %d wrap %d sort_path %d\n",
           nj, cat["nf_sweep"], cat["total_sweep"], cat["dups"], cat["rowlens"], cat["noprofile"], cat["interest_excl"], cat["views"], cat["hash"],
           cat["nk"], cat["all"], cat["clubs"], multi_round, edge_limit, clusters, wrap, sort_path);
    free_all();
}

// ================================================================ B: K9 and the dispatch order
static void check_order(const std::vector<int32_t>& first_slot, const char* what) {
    const int nb = (int)first_slot.size();
    // every block starts at its own word of the slot array, in a shuffled place
    std::vector<int32_t> where(nb), slots(nb);
    for (int b = 0; b < nb; ++b) where[b] = b;
    std::shuffle(where.begin(), where.end(), rng);
    std::vector<PairBlock> blocks(nb);
    for (int b = 0; b < nb; ++b) {
        blocks[b] = PairBlock{b, where[b], 1, b};
        slots[where[b]] = first_slot[b];
    }
    PairBlock* d_b = up(blocks);
    int32_t* d_s = up(slots);
    int32_t* d_o = dalloc<int32_t>(nb);
    SYNC(launch_order_pairs(d_b, nb, d_s, nb, d_o, nullptr));
    const std::vector<int32_t> order = down(d_o, nb);
    std::vector<char> seen(nb, 0);
    int prev = -1;
    for (int i = 0; i < nb; ++i) {
        const int32_t b = order[i];
        if (b < 0 || b >= nb || seen[b]) FAIL("B order %s nblocks %d: position %d holds %d, no permutation", what, nb, i, b);
        seen[b] = 1;
        const int key = first_slot[b] < 0 ? 256 : h_slot_class(first_slot[b]);
        if (key < prev) FAIL("B order %s nblocks %d: key falls from %d to %d at position %d", what, nb, prev, key, i);
        prev = key;
    }
    free_all();
}

static void part_b() {
    // ---- expand_pairs_kernel against PairGen's formula
    long blocks_checked = 0, run_edges = 0;
    for (int ngens : {1, 2, 1000}) {
        std::vector<PairGen> gens(ngens);
        std::vector<int2> pool;
        int nblocks = 0;
        const int caps[6] = {1, 511, 513, 1000, 1537, 2049};
        for (int i = 0; i < ngens; ++i) {
            PairGen& G = gens[i];
            G.nf = (i & 1) ? 7 : 1;
            G.cap = ngens <= 2 ? caps[3 + i] : (i < 6 ? caps[i] : 1 + (int)rnd(1600));
            G.nch = (G.cap + kPairThreads - 1) / kPairThreads;
            G.cand = (int)rnd(1 << 20);
            G.fl = (int)pool.size();
            G.stride = G.cap + (int)rnd(9);
            G.out = (int)rnd(1 << 20);
            G.first = nblocks;
            for (int f = 0; f < G.nf; ++f) pool.push_back(make_int2((int)rnd(5000), (int)rnd(64)));
            nblocks += G.nf * G.nch;
        }
        PairGen* d_g = up(gens);
        int2* d_p = up(pool);
        PairBlock* d_b = dalloc<PairBlock>(nblocks);
        SYNC(launch_expand_pairs(d_g, ngens, d_p, nblocks, d_b, nullptr));
        const std::vector<PairBlock> got = down(d_b, nblocks);
        for (const PairGen& G : gens)
            for (int x = 0; x < G.nch; ++x)
                for (int f = 0; f < G.nf; ++f) {
                    const int b = G.first + x * G.nf + f;
                    const int2 e = pool[G.fl + f];
                    const PairBlock w{e.x, G.cand + x * kPairThreads, std::min(kPairThreads, G.cap - x * kPairThreads), G.out + e.y * G.stride + x * kPairThreads};
                    const PairBlock& h = got[b];
                    if (h.qimg != w.qimg || h.begin != w.begin || h.count != w.count || h.out != w.out)
                        FAIL("B expand ngens %d block %d: (%d %d %d %d) want (%d %d %d %d)", ngens, b, h.qimg, h.begin, h.count, h.out, w.qimg, w.begin, w.count, w.out);
                    ++blocks_checked;
                    run_edges += (x == 0 && f == 0) || (x == G.nch - 1 && f == G.nf - 1);
                }
        free_all();
    }
    // ---- slot_class on the host: monotone and below 232
    std::vector<int32_t> probe_slots;
    for (int32_t s = 0; s <= 40; ++s) probe_slots.push_back(s);
    for (int k = 1; k <= 30; ++k)
        for (int d = -1; d <= 1; ++d) probe_slots.push_back((int32_t)((1ll << k) + d));
    probe_slots.push_back(INT32_MAX);
    std::sort(probe_slots.begin(), probe_slots.end());
    for (size_t i = 0; i < probe_slots.size(); ++i) {
        const int c = h_slot_class(probe_slots[i]);
        if (c < 0 || c >= 232) FAIL("B slot_class(%d) = %d", probe_slots[i], c);
        if (i && c < h_slot_class(probe_slots[i - 1])) FAIL("B slot_class falls at %d", probe_slots[i]);
    }
    // ---- and on the device, through the order it gives blocks that start at those slots
    std::vector<int32_t> fs;
    for (int rep = 0; rep < 3; ++rep) fs.insert(fs.end(), probe_slots.begin(), probe_slots.end());
    fs.push_back(-1);
    std::shuffle(fs.begin(), fs.end(), rng);
    check_order(fs, "slot_class");
    // ---- order_pairs_kernel around its 8 x 1024 kept keys
    int below = 0, above = 0;
    for (int nb : {1, 1023, 1024, 1025, 8191, 8192, 8193, 20000}) {
        std::vector<int32_t> f(nb);
        for (auto& s : f) {
            const int kind = (int)rnd(10);
            s = kind == 0 ? -1 - (int32_t)rnd(5) : kind < 4 ? (int32_t)rnd(64) : (int32_t)rnd(1ll << (3 + rnd(28)));
        }
        check_order(f, "sizes");
        (nb <= 8192 ? below : above) += 1;
    }
    printf("B expand_blocks %ld run_edges %ld slot_values %zu order_below_8192 %d order_above_8192 %d\n", blocks_checked, run_edges, probe_slots.size(), below, above);
}

// ================================================================ C: K4' sums and the fused top-k
struct CJob {
    int nf = 0, cap = 0, nfd = 0, topk = 0, launch = 0;
    bool planted = false;
    std::vector<int32_t> fpos, slot, id;
    std::vector<float> sim, M, ref;
    std::vector<char> has_plant;
    int64_t fpos_off = 0, sim_off = 0, m_off = 0, off = 0;
};

static float c_sum(const CJob& j, int c, bool reverse) {
    double s = 0.0;
    for (int q = 0; q < j.nf; ++q) {
        const int p = reverse ? j.nf - 1 - q : q;
        const int r = j.fpos[p];
        if (r < 0) continue;
        s += (double)j.sim[r] * (double)j.M[(size_t)r * j.cap + c];
    }
    return (float)s;
}

static std::vector<uint64_t> c_topk(const CJob& j, int k) {
    std::vector<uint64_t> keys;
    for (int c = 0; c < j.cap; ++c)
        if (j.slot[c] >= 0) keys.push_back(score_key(j.ref[c], j.id[c]));
    std::sort(keys.begin(), keys.end());
    keys.resize(k, NONE);
    return keys;
}

static long g_same_tile = 0, g_cross_tile = 0;
static CJob make_cjob(int nf, int cap, bool plant, bool ties) {
    CJob j;
    j.nf = nf;
    j.cap = cap;
    j.planted = plant;
    std::vector<int> uses;
    for (int p = 0; p < nf; ++p) {
        const int kind = nf == 1 ? 2 : (int)rnd(10);
        if (kind == 0) j.fpos.push_back(-1);
        else if (kind == 1 && j.nfd > 0) { const int r = (int)rnd(j.nfd); j.fpos.push_back(r); ++uses[r]; }  // a repeated friend
        else { j.fpos.push_back(j.nfd++); uses.push_back(1); }
    }
    const float big = ldexpf(1.0f, 40), tiny = ldexpf(1.0f, -40);
    std::vector<char> isbig(j.nfd, 0);
    j.sim.resize(j.nfd);
    for (int r = 0; r < j.nfd; ++r) {
        isbig[r] = plant && uses[r] == 1 && rnd(2);
        j.sim[r] = isbig[r] ? big : frand(0.1f, 1.0f);
    }
    j.M.resize((size_t)j.nfd * cap);
    for (int r = 0; r < j.nfd; ++r)
        for (int c = 0; c < cap; ++c) j.M[(size_t)r * cap + c] = frand(0.1f, 1.0f) * (isbig[r] ? tiny : 1.0f);  // every product in (0.01, 1)
    std::vector<int> bigpos;
    for (int p = 0; p < nf; ++p)
        if (j.fpos[p] >= 0 && isbig[j.fpos[p]]) bigpos.push_back(p);
    j.has_plant.assign(cap, 0);
    if (bigpos.size() >= 2)
        for (int c = 0; c < cap; ++c) {
            int a, b;
            if (c & 1) {  // neighbours: mostly within one 64-tile
                a = (int)rnd((int64_t)bigpos.size() - 1);
                b = a + 1;
            } else {
                a = (int)rnd((int64_t)bigpos.size());
                b = (int)rnd((int64_t)bigpos.size() - 1);
                if (b >= a) ++b;
                if (a > b) std::swap(a, b);
            }
            const int p1 = bigpos[a], p2 = bigpos[b];
            j.M[(size_t)j.fpos[p1] * cap + c] = big;    // + 2^80 at p1
            j.M[(size_t)j.fpos[p2] * cap + c] = -big;   // - 2^80 at p2 > p1
            j.has_plant[c] = 1;
            (p1 / 64 == p2 / 64 ? g_same_tile : g_cross_tile) += 1;
        }
    if (ties)  // equal scores that differ in id
        for (int c = 1; c < cap; c += 2) {
            for (int r = 0; r < j.nfd; ++r) j.M[(size_t)r * cap + c] = j.M[(size_t)r * cap + c - 1];
            j.has_plant[c] = j.has_plant[c - 1];
        }
    j.slot.resize(cap);
    j.id.resize(cap);
    for (int c = 0; c < cap; ++c) {
        j.slot[c] = rnd(8) == 0 ? -1 - (int32_t)rnd(3) : (int32_t)rnd(1 << 20);
        j.id[c] = 100 + 7 * c;
    }
    std::shuffle(j.id.begin(), j.id.end(), rng);
    j.ref.resize(cap);
    for (int c = 0; c < cap; ++c) j.ref[c] = c_sum(j, c, false);
    return j;
}

static void part_c() {
    const int ks[4] = {1, 10, 63, 64};
    std::vector<CJob> jobs;
    int combo = 0;
    for (int nf : {1, 63, 64, 65, 127, 128, 129, 1000})
        for (int cap : {1, 63, 64, 65, 128, 129, 1000}) {
            jobs.push_back(make_cjob(nf, cap, nf > 1 && combo % 3 != 2, combo % 5 == 0));
            jobs.back().launch = combo % 4;
            jobs.back().topk = ks[combo % 4];
            ++combo;
        }
    for (int l = 0; l < 4; ++l) {
        CJob z = make_cjob(65, 0, false, false);  // cap 0: its key row stays as it was
        z.launch = l;
        z.topk = ks[l];
        jobs.insert(jobs.begin() + 5 + 9 * l, z);
        CJob w = make_cjob(129, l & 1 ? 1000 : 129, true, true);  // topk 65: ranked by K8
        w.launch = l;
        w.topk = 65;
        jobs.push_back(w);
    }
    const int nj = (int)jobs.size();
    // the inputs tell summation orders apart: on the host reference alone, before any launch
    long planted = 0, differ = 0, planted_jobs = 0;
    for (const CJob& j : jobs) {
        planted_jobs += j.planted;
        for (int c = 0; c < j.cap; ++c)
            if (j.has_plant[c]) {
                ++planted;
                differ += bits_of(c_sum(j, c, true)) != bits_of(j.ref[c]);
            }
    }
    if (planted == 0 || differ * 100 < planted * 95) FAIL("C: reversing the sum changes %ld of %ld planted candidates, below 95 %%", differ, planted);
    if (planted_jobs * 2 < nj) FAIL("C: %ld of %d jobs planted", planted_jobs, nj);
    // ---- layout
    std::vector<DevJob> dj(nj);
    std::vector<int32_t> pool(1, 0), slots, ids;
    std::vector<float> pout;
    for (int i = 0; i < nj; ++i) {
        CJob& j = jobs[i];
        DevJob& d = dj[i];
        memset(&d, 0, sizeof d);
        d.kind = kDjCollab;
        d.nf = j.nf;
        d.cap = j.cap;
        d.nfd = j.nfd;
        d.topk = j.topk;
        d.fpos_off = (int64_t)pool.size();
        pool.insert(pool.end(), j.fpos.begin(), j.fpos.end());
        d.sim_off = (int64_t)pout.size();
        pout.insert(pout.end(), j.sim.begin(), j.sim.end());
        d.m_off = (int64_t)pout.size();
        pout.insert(pout.end(), j.M.begin(), j.M.end());
        j.off = d.cand_off = d.out_off = (int64_t)slots.size();
        slots.insert(slots.end(), j.slot.begin(), j.slot.end());
        ids.insert(ids.end(), j.id.begin(), j.id.end());
    }
    const size_t E = slots.size();
    DevJob* d_jobs = up(dj);
    int32_t* d_pool = up(pool);
    float* d_pout = up(pout);
    int32_t* d_slot = up(slots);
    int32_t* d_id = up(ids);
    float* d_score = dalloc<float>(E);
    int32_t* d_ncand = dalloc<int32_t>(nj, 0);
    std::vector<uint32_t> want_score(E, (uint32_t)SENT);
    long live = 0, dead = 0, fused[3] = {0, 0, 0}, untouched = 0, k8_rows = 0, tie_pairs = 0;
    for (int l = 0; l < 4; ++l) {
        const int k = ks[l];
        std::vector<int32_t> jix;
        int max_cap = 0;
        for (int i = 0; i < nj; ++i)
            if (jobs[i].launch == l) { jix.push_back(i); max_cap = std::max(max_cap, jobs[i].cap); }
        std::reverse(jix.begin(), jix.end());
        std::swap(jix[1], jix[jix.size() / 2]);  // neither the identity nor complete; the cap-0 job stays between two others
        const int nl = (int)jix.size(), gx = (max_cap + 63) / 64;
        int32_t* d_jix = up(jix);
        uint64_t* d_parts = dalloc<uint64_t>((size_t)nl * gx * k);
        unsigned int* d_tickets = dalloc<unsigned int>(nl, 0);
        uint64_t* d_out = dalloc<uint64_t>((size_t)nj * k);
        SYNC(launch_collab(d_jobs, d_jix, nl, max_cap, d_pool, d_pout, d_slot, d_score, d_id, d_parts, d_tickets, d_out, k, nullptr));
        for (int i : jix)
            for (int c = 0; c < jobs[i].cap; ++c)
                if (jobs[i].slot[c] >= 0) { want_score[jobs[i].off + c] = bits_of(jobs[i].ref[c]); ++live; } else ++dead;
        const std::vector<float> sc = down(d_score, E);
        for (size_t e = 0; e < E; ++e)
            if (bits_of(sc[e]) != want_score[e]) {
                int at = 0;
                for (int i = 0; i < nj; ++i)
                    if ((int64_t)e >= jobs[i].off && (int64_t)e < jobs[i].off + jobs[i].cap) at = i;
                FAIL("C k %d job %d (nf %d cap %d planted %d) candidate %lld: score bits %08x want %08x", k, at, jobs[at].nf, jobs[at].cap, (int)jobs[at].planted,
                     (long long)((int64_t)e - jobs[at].off), bits_of(sc[e]), want_score[e]);
            }
        std::vector<uint64_t> want_out((size_t)nj * k, SENT64);
        std::vector<int32_t> to_k8;
        for (int i : jix) {
            const CJob& j = jobs[i];
            if (j.topk > kMaxTopK) { to_k8.push_back(i); ++untouched; continue; }
            if (j.cap == 0) { ++untouched; continue; }
            const std::vector<uint64_t> w = c_topk(j, k);
            std::copy(w.begin(), w.end(), want_out.begin() + (size_t)i * k);
            const int nb = (j.cap + 63) / 64;
            ++fused[nb == 1 ? 0 : nb == 2 ? 1 : 2];
            for (int q = 1; q < k; ++q) tie_pairs += w[q] != NONE && (w[q] >> 32) == (w[q - 1] >> 32);
        }
        std::vector<uint64_t> out = down(d_out, (size_t)nj * k);
        for (size_t e = 0; e < out.size(); ++e)
            if (out[e] != want_out[e]) FAIL("C k %d job %d (cap %d topk %d) key %zu: %016llx want %016llx", k, (int)(e / k), jobs[e / k].cap, jobs[e / k].topk, e % k,
                                            (unsigned long long)out[e], (unsigned long long)want_out[e]);
        // the jobs beyond the fused bound: K8 fills their rows, and only theirs
        int32_t* d_jix8 = up(to_k8);
        SYNC(launch_job_topk(d_jobs, d_jix8, (int)to_k8.size(), d_score, d_id, d_slot, d_ncand, d_out, k, nullptr));
        for (int i : to_k8) {
            const std::vector<uint64_t> w = c_topk(jobs[i], k);
            std::copy(w.begin(), w.end(), want_out.begin() + (size_t)i * k);
            ++k8_rows;
        }
        out = down(d_out, (size_t)nj * k);
        for (size_t e = 0; e < out.size(); ++e)
            if (out[e] != want_out[e]) FAIL("C K8 k %d job %d key %zu: %016llx want %016llx", k, (int)(e / k), e % k, (unsigned long long)out[e], (unsigned long long)want_out[e]);
    }
    printf("C jobs %d planted_jobs %ld planted %ld order_sensitive %ld share %.4f same_tile %ld cross_tile %ld live %ld dead %ld fused_1 %ld fused_2 %ld fused_16 %ld "
           "untouched %ld k8_rows %ld tie_pairs %ld\n",
           nj, planted_jobs, planted, differ, (double)differ / (double)planted, g_same_tile, g_cross_tile, live, dead, fused[0], fused[1], fused[2], untouched, k8_rows, tie_pairs);
    free_all();
}

// ================================================================ D: K7 clubs
struct DJob {
    std::string name;
    int32_t u = 0;
    std::vector<int32_t> F, fpos, fdnode;
    std::vector<float> sim;
    std::vector<std::vector<float>> S;  // per distinct friend r, one value per element of its row
    int cap = 0;
    int64_t out_off = 0;
    std::map<int32_t, std::vector<double>> seqs;  // the reference: every club's contributions in stream order
    std::map<int32_t, double> sum;
};

static const int kNClubs = 8192;
struct DWorld {
    Graph g;
    int32_t next = 100;
    int32_t node(std::vector<int32_t> clubs) {
        const int32_t x = next++;
        if (x >= g.n) FAIL("D: out of nodes");
        g.clubs[x] = std::move(clubs);
        return x;
    }
    std::vector<int32_t> rclubs(int k) {  // k distinct clubs outside the designated ones [0, 1000)
        std::set<int32_t> s;
        while ((int)s.size() < k) s.insert(1000 + (int32_t)rnd(kNClubs - 1000));
        std::vector<int32_t> v(s.begin(), s.end());
        std::shuffle(v.begin(), v.end(), rng);
        return v;
    }
    // a friend (a new distinct one) with its clubs, its row (nullptr: none) and the row's S values
    int add_friend(DJob& j, float sim, std::vector<int32_t> clubs, const std::vector<int32_t>* row, std::vector<float> S) {
        const int32_t f = node(std::move(clubs));
        if (row) g.set_row(f, *row);
        if (S.size() != (row ? row->size() : 0)) FAIL("D: S and the row differ in length");
        j.F.push_back(f);
        j.fpos.push_back((int32_t)j.sim.size());
        j.fdnode.push_back(f);
        j.sim.push_back(sim);
        j.S.push_back(std::move(S));
        return (int)j.sim.size() - 1;
    }
    void add_repeat(DJob& j, int r) { j.F.push_back(j.fdnode[r]); j.fpos.push_back(r); }
    void add_skip(DJob& j, int32_t x) { j.F.push_back(x); j.fpos.push_back(-1); }
};

static long g_multi_round_items = 0, g_nan_clubs = 0;
static std::set<int> g_chunk_totals;
static void d_ref(const Graph& g, DJob& j) {
    const std::set<int32_t> own(g.clubs[j.u].begin(), g.clubs[j.u].end());
    auto give = [&](int32_t x, double v) {
        g_multi_round_items += g.clubs[x].size() > 512;
        for (int32_t d : g.clubs[x])
            if (!own.count(d)) { j.seqs[d].push_back(v); j.sum[d] += v; }
    };
    const int nf = (int)j.F.size();
    int total1 = 0, total2 = 0, items2 = 0;
    for (int p = 0; p < nf; ++p) {  // phase 1: friends in order, then each friend's clubs
        const int r = j.fpos[p];
        if (r < 0) continue;
        const double w = (double)j.sim[r];
        if (w <= 0.0) continue;
        give(j.F[p], w);
        total1 += (int)g.clubs[j.F[p]].size();
    }
    for (int p = 0; p < nf; ++p) {  // phase 2: friends in order, their rows, each friend-of-friend's clubs
        const int r = j.fpos[p];
        if (r < 0) continue;
        const int32_t f = j.F[p];
        if (g.len[f] < 0) continue;
        const double w = (double)j.sim[r];
        if (w <= 0.0) continue;
        for (int k = 0; k < g.len[f]; ++k) {
            ++items2;
            const int32_t x = g.row[f][k];
            if (x == j.u || x < 0 || x >= g.n) continue;
            const double sx = (double)j.S[r][k];
            if (sx <= 0.0) continue;
            give(x, w * sx);
            total2 += (int)g.clubs[x].size();
        }
    }
    if (nf <= 64) g_chunk_totals.insert(total1);   // one phase-1 chunk
    if (nf <= 64 && items2 <= 64) g_chunk_totals.insert(total2);  // one phase-2 chunk
    j.cap = (int)j.sum.size() + 4;
}

static void part_d() {
    DWorld W;
    W.g.init(20000, 20100, kNClubs);
    Graph& g = W.g;
    std::vector<DJob> jobs;
    auto begin = [&](const char* name, std::vector<int32_t> own = {}) {
        jobs.emplace_back();
        jobs.back().name = name;
        jobs.back().u = W.node(std::move(own));
        return &jobs.back();
    };
    auto split = [&](int T, int parts) {  // T distinct random clubs in `parts` lists
        const std::vector<int32_t> all = W.rclubs(T);
        std::vector<std::vector<int32_t>> v(parts);
        for (int i = 0; i < T; ++i) v[i % parts].push_back(all[i]);
        return v;
    };
    // the stream total of one chunk on both sides of a round of 512
    for (int T : {511, 512, 513, 1024, 1025}) {
        DJob* j = begin("totals");
        std::vector<int32_t> row;
        std::vector<float> S;
        for (auto& c : split(T, 64)) { row.push_back(W.node(c)); S.push_back(frand(0.1f, 1.0f)); }
        const auto fc = split(T, 8);
        for (int i = 0; i < 8; ++i) {
            if (i == 0) W.add_friend(*j, frand(0.1f, 1.0f), fc[i], &row, S);
            else if (i & 1) W.add_friend(*j, frand(0.1f, 1.0f), fc[i], nullptr, {});
            else { const std::vector<int32_t> none; W.add_friend(*j, frand(0.1f, 1.0f), fc[i], &none, {}); }
        }
    }
    {  // a single item spans rounds: 600 clubs in phase 1 and in phase 2
        DJob* j = begin("span");
        const std::vector<int32_t> row = {W.node(W.rclubs(600)), W.node(W.rclubs(5))};
        W.add_friend(*j, 0.5f, W.rclubs(3), &row, {0.25f, 0.75f});
        W.add_friend(*j, 0.3f, W.rclubs(600), nullptr, {});
        W.add_friend(*j, 0.7f, W.rclubs(40), nullptr, {});
    }
    {  // club 1 twice in one round and again in the next
        DJob* j = begin("twice");
        for (int n0 : {256, 256, 10}) {
            std::vector<int32_t> c = W.rclubs(n0 - 1);
            c.insert(c.begin(), 1);
            W.add_friend(*j, frand(0.1f, 1.0f), c, nullptr, {});
        }
    }
    {  // owner lanes: 65 clubs equal mod 64, 64 all different
        DJob* j = begin("lanes");
        std::vector<int32_t> a, b;
        for (int i = 0; i < 65; ++i) a.push_back(7 + 64 * i);
        for (int i = 0; i < 64; ++i) b.push_back(6400 + i);
        std::shuffle(a.begin(), a.end(), rng);
        const std::vector<int32_t> row = {W.node(a), W.node(b)};
        W.add_friend(*j, 0.9f, a, &row, {0.5f, 0.6f});
        W.add_friend(*j, 0.8f, b, nullptr, {});
    }
    {  // the query's own clubs
        DJob* j = begin("own", {20, 21, 22, 23, 24});
        const std::vector<int32_t> row = {W.node({21, 31}), W.node({20, 24})};
        W.add_friend(*j, 0.9f, {20, 21, 22, 23, 24}, nullptr, {});  // all of them the query's own
        W.add_friend(*j, 0.8f, {20, 30}, &row, {0.5f, 0.6f});
    }
    for (int nf : {0, 1, 64, 65}) {  // friends per phase-1 and phase-2 group of 64
        DJob* j = begin("nf");
        for (int i = 0; i < nf; ++i) {
            if (i % 9 == 4) { W.add_skip(*j, i % 2 ? g.n + 3 : 5); continue; }
            if (i % 9 == 7 && !j->sim.empty()) { W.add_repeat(*j, (int)rnd((int64_t)j->sim.size())); continue; }
            std::vector<int32_t> row;
            std::vector<float> S;
            const int len = (int)rnd(6);
            for (int k = 0; k < len; ++k) { row.push_back(W.node(W.rclubs((int)rnd(5)))); S.push_back(frand(0.1f, 1.0f)); }
            W.add_friend(*j, frand(0.1f, 1.0f), W.rclubs(3), i % 5 == 1 ? nullptr : &row, i % 5 == 1 ? std::vector<float>() : S);
        }
    }
    {  // one friend whose sim is NaN
        DJob* j = begin("nan");
        const std::vector<int32_t> row = {W.node({42, 43})};
        W.add_friend(*j, 0.5f, {40, 44}, nullptr, {});
        W.add_friend(*j, nanf(""), {40, 41}, &row, {0.5f});
        W.add_friend(*j, 0.25f, {40, 43, 45}, nullptr, {});
    }
    {  // what is skipped: w <= 0, sx <= 0, the user, nodes without a profile, friends without a row
        DJob* j = begin("skips");
        const int32_t x1 = W.node({50, 51}), x2 = W.node({51, 52});
        const std::vector<int32_t> row = {x1, j->u, g.n + 4, x2, x1, x2};
        W.add_friend(*j, 0.5f, {50, 53}, &row, {0.5f, 0.9f, 0.9f, 0.0f, -0.5f, 0.25f});
        W.add_friend(*j, 0.0f, {50, 54}, &row, {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f});
        W.add_friend(*j, -0.5f, {50, 55}, &row, {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f});
        W.add_skip(*j, g.n + 5);
        W.add_repeat(*j, 0);
        const std::vector<int32_t> none;
        W.add_friend(*j, 0.75f, {56}, &none, {});
    }
    // sums whose float depends on the order: 1.0, 2^-24, then 2^-54 four times, as w * sx with w = 1
    const float seq6[6] = {1.0f, ldexpf(1.0f, -24), ldexpf(1.0f, -54), ldexpf(1.0f, -54), ldexpf(1.0f, -54), ldexpf(1.0f, -54)};
    std::vector<std::pair<size_t, int32_t>> order_clubs;  // (job, club)
    {  // phase 1 alone
        DJob* j = begin("order_p1");
        for (int i = 0; i < 6; ++i) W.add_friend(*j, seq6[i], {100, 101}, nullptr, {});
        order_clubs.push_back({jobs.size() - 1, 100});
        order_clubs.push_back({jobs.size() - 1, 101});
    }
    {  // phase 1, then phase 2
        DJob* j = begin("order_p1p2");
        std::vector<int32_t> row;
        for (int i = 0; i < 4; ++i) row.push_back(W.node({102, 103}));
        W.add_friend(*j, seq6[0], {102, 103}, nullptr, {});
        W.add_friend(*j, seq6[1], {103, 102}, nullptr, {});
        W.add_friend(*j, 1.0f, {104}, &row, {seq6[2], seq6[3], seq6[4], seq6[5]});
        order_clubs.push_back({jobs.size() - 1, 102});
        order_clubs.push_back({jobs.size() - 1, 103});
    }
    {  // phase 2 within a round
        DJob* j = begin("order_p2");
        std::vector<int32_t> row;
        for (int i = 0; i < 6; ++i) row.push_back(W.node({105, 106}));
        W.add_friend(*j, 1.0f, {107}, &row, std::vector<float>(seq6, seq6 + 6));
        order_clubs.push_back({jobs.size() - 1, 105});
        order_clubs.push_back({jobs.size() - 1, 106});
    }
    {  // phase 2 across a round's edge: 510 contributions first
        DJob* j = begin("order_p2_edge");
        std::vector<int32_t> row = {W.node(W.rclubs(510))};
        std::vector<float> S = {0.5f};
        for (int i = 0; i < 6; ++i) { row.push_back(W.node({108, 109})); S.push_back(seq6[i]); }
        W.add_friend(*j, 1.0f, {110}, &row, S);
        order_clubs.push_back({jobs.size() - 1, 108});
        order_clubs.push_back({jobs.size() - 1, 109});
    }
    {  // phase 1 across a round's edge: 511 contributions first
        DJob* j = begin("order_p1_edge");
        W.add_friend(*j, 0.5f, W.rclubs(511), nullptr, {});
        for (int i = 0; i < 6; ++i) W.add_friend(*j, seq6[i], {111, 112}, nullptr, {});
        order_clubs.push_back({jobs.size() - 1, 111});
        order_clubs.push_back({jobs.size() - 1, 112});
    }
    const int nj = (int)jobs.size();
    for (DJob& j : jobs) d_ref(g, j);
    for (int T : {511, 512, 513, 1024, 1025})
        if (!g_chunk_totals.count(T)) FAIL("D: no chunk with a stream total of %d", T);
    for (auto& oc : order_clubs) {
        const std::vector<double>& s = jobs[oc.first].seqs[oc.second];
        double f = 0.0, r = 0.0;
        for (size_t i = 0; i < s.size(); ++i) { f += s[i]; r += s[s.size() - 1 - i]; }
        if (s.size() != 6 || bits_of((float)f) != 0x3f800000u || bits_of((float)r) != 0x3f800001u)
            FAIL("D %s club %d: %zu terms, %08x in order, %08x reversed", jobs[oc.first].name.c_str(), oc.second, s.size(), bits_of((float)f), bits_of((float)r));
    }
    // ---- layout
    std::vector<DevJob> dj(nj);
    std::vector<int32_t> pool(1, 0);
    std::vector<int64_t> pool64(1, 0);
    std::vector<float> pout(1, 0.0f);
    int64_t E = 0;
    for (int i = 0; i < nj; ++i) {
        DJob& j = jobs[i];
        DevJob& d = dj[i];
        memset(&d, 0, sizeof d);
        d.kind = kDjClubs;
        d.u = j.u;
        d.own = -1;
        d.own_len = -1;
        d.nf = (int32_t)j.F.size();
        d.nfd = (int32_t)j.sim.size();
        d.f_off = (int64_t)pool.size();
        pool.insert(pool.end(), j.F.begin(), j.F.end());
        d.fpos_off = (int64_t)pool.size();
        pool.insert(pool.end(), j.fpos.begin(), j.fpos.end());
        d.sim_off = (int64_t)pout.size();
        pout.insert(pout.end(), j.sim.begin(), j.sim.end());
        d.sreg_off = (int64_t)pool64.size();
        for (int r = 0; r < d.nfd; ++r) {
            pool64.push_back((int64_t)pout.size());
            pout.insert(pout.end(), j.S[r].begin(), j.S[r].end());
        }
        d.cap = j.cap;
        j.out_off = d.out_off = d.cand_off = E;
        E += j.cap;
        for (size_t p = 0; p < j.F.size(); ++p)
            if (j.fpos[p] >= 0 && (j.F[p] < 0 || j.F[p] >= g.n)) FAIL("D: a counted friend without a profile");
    }
    const DevJobsStore ds = g.upload();
    View none;
    const DevView dv = none.upload();
    DevJob* d_jobs = up(dj);
    int32_t* d_pool = up(pool);
    int64_t* d_pool64 = up(pool64);
    float* d_pout = up(pout);
    double* d_acc = dalloc<double>((size_t)nj * kNClubs, 0);
    float* d_score = dalloc<float>(E);
    int32_t* d_ids = dalloc<int32_t>(E);
    int32_t* d_ncand = dalloc<int32_t>(nj);
    long clubs_checked = 0, acc_zero = 0, order_ok = 0;
    for (int pass = 0; pass < 2; ++pass) {  // back to back over the same acc slots, jobs in other slots
        std::vector<int32_t> jix(nj);
        for (int i = 0; i < nj; ++i) jix[i] = pass ? (i * 7 + 3) % nj : nj - 1 - i;
        if (std::set<int32_t>(jix.begin(), jix.end()).size() != (size_t)nj) FAIL("D: jix is no permutation");
        int32_t* d_jix = up(jix);
        CK(hipMemset(d_score, 0x5A, std::max<int64_t>(E, 1) * 4));
        CK(hipMemset(d_ids, 0x5A, std::max<int64_t>(E, 1) * 4));
        CK(hipMemset(d_ncand, 0x5A, nj * 4));
        SYNC(launch_clubs(ds, dv, d_jobs, d_jix, nj, d_pool, d_pool64, d_pout, d_acc, d_score, d_ids, d_ncand, kNClubs, nullptr));
        const std::vector<float> sc = down(d_score, E);
        const std::vector<int32_t> id = down(d_ids, E), nc = down(d_ncand, nj);
        for (int i = 0; i < nj; ++i) {
            const DJob& j = jobs[i];
            if (nc[i] != (int)j.sum.size()) FAIL("D %s job %d pass %d: ncand %d want %zu", j.name.c_str(), i, pass, nc[i], j.sum.size());
            std::map<int32_t, float> got;
            for (int e = 0; e < nc[i]; ++e) got[id[j.out_off + e]] = sc[j.out_off + e];
            if (got.size() != j.sum.size()) FAIL("D %s job %d pass %d: a club listed twice", j.name.c_str(), i, pass);
            for (auto& kv : j.sum) {
                auto it = got.find(g.club_id[kv.first]);
                if (it == got.end()) FAIL("D %s job %d pass %d: club %d missing", j.name.c_str(), i, pass, kv.first);
                const float want = (float)kv.second;
                if (std::isnan(want) ? !std::isnan(it->second) : bits_of(it->second) != bits_of(want))
                    FAIL("D %s job %d pass %d club %d (%zu terms): %08x want %08x", j.name.c_str(), i, pass, kv.first, j.seqs.at(kv.first).size(), bits_of(it->second), bits_of(want));
                ++clubs_checked;
                if (pass == 0) g_nan_clubs += std::isnan(want);
            }
            for (int e = nc[i]; e < j.cap; ++e)
                if (bits_of(sc[j.out_off + e]) != (uint32_t)SENT || id[j.out_off + e] != SENT) FAIL("D %s job %d pass %d: entry %d past ncand written", j.name.c_str(), i, pass, e);
        }
        const std::vector<double> acc = down(d_acc, (size_t)nj * kNClubs);
        for (size_t e = 0; e < acc.size(); ++e) {
            uint64_t b;
            memcpy(&b, &acc[e], 8);
            if (b != 0) FAIL("D pass %d: acc slot %zu club %zu is not zero after the launch", pass, e / kNClubs, e % kNClubs);
        }
        acc_zero += (long)acc.size();
        order_ok += (long)order_clubs.size();
    }
    if (g_nan_clubs == 0) FAIL("D: no club with a NaN score");
    printf("D jobs %d clubs_checked %ld order_clubs %zu order_checked %ld multi_round_items %ld nan_clubs %ld chunk_totals %zu acc_zero %ld launches 2\n", nj, clubs_checked,
           order_clubs.size(), order_ok, g_multi_round_items, g_nan_clubs, g_chunk_totals.size(), acc_zero);
    free_all();
}

// ================================================================ E: K8
static void part_e() {
    long rows = 0, short_rows = 0, tie_pairs = 0, club_rows = 0;
    for (int k : {1, 10, 64}) {
        struct EJob { int cap, kind, ncand; int64_t off; };
        std::vector<EJob> jobs;
        std::vector<DevJob> dj;
        std::vector<float> score;
        std::vector<int32_t> ids, slots, ncand;
        const float levels[5] = {0.0f, 0.125f, 0.5f, 0.75f, 1.5f};  // few scores: long ties, broken by id
        for (int kind : {(int)kDjCollab, (int)kDjClubs, (int)kDjInterest})
            for (int cap : {0, 1, 63, 64, 65, 255, 256, 257, 1000}) {
                EJob j{cap, kind, kind == kDjClubs ? cap - cap / 3 : 12345, (int64_t)score.size()};
                for (int c = 0; c < cap; ++c) {
                    score.push_back(rnd(3) ? levels[rnd(5)] : frand(-1.0f, 2.0f));
                    ids.push_back(3 + 1009 * c + (int32_t)rnd(1000));  // distinct within a job
                    // club jobs ignore the slots (all < 0 here); user jobs skip a slot < 0
                    slots.push_back(kind == kDjClubs ? -1 : rnd(4) == 0 ? -1 : (int32_t)rnd(1000));
                }
                DevJob d;
                memset(&d, 0, sizeof d);
                d.kind = kind;
                d.cap = cap;
                d.cand_off = d.out_off = j.off;
                d.topk = k;
                dj.push_back(d);
                jobs.push_back(j);
                ncand.push_back(j.ncand);
            }
        const int nj = (int)jobs.size();
        std::vector<int32_t> jix;
        for (int i = nj - 1; i >= 0; --i)
            if (i % 5 != 2) jix.push_back(i);  // neither the identity nor complete
        DevJob* d_jobs = up(dj);
        int32_t* d_jix = up(jix);
        float* d_score = up(score);
        int32_t* d_ids = up(ids);
        int32_t* d_slots = up(slots);
        int32_t* d_ncand = up(ncand);
        uint64_t* d_out = dalloc<uint64_t>((size_t)nj * k);
        SYNC(launch_job_topk(d_jobs, d_jix, (int)jix.size(), d_score, d_ids, d_slots, d_ncand, d_out, k, nullptr));
        const std::vector<uint64_t> out = down(d_out, (size_t)nj * k);
        std::vector<uint64_t> want((size_t)nj * k, SENT64);
        for (int i : jix) {
            const EJob& j = jobs[i];
            std::vector<uint64_t> keys;
            const int lim = j.kind == kDjClubs ? j.ncand : j.cap;
            for (int c = 0; c < lim; ++c)
                if (j.kind == kDjClubs || slots[j.off + c] >= 0) keys.push_back(score_key(score[j.off + c], ids[j.off + c]));
            std::sort(keys.begin(), keys.end());
            short_rows += (int)keys.size() < k;
            keys.resize(k, NONE);
            std::copy(keys.begin(), keys.end(), want.begin() + (size_t)i * k);
            for (int q = 1; q < k; ++q) tie_pairs += keys[q] != NONE && (keys[q] >> 32) == (keys[q - 1] >> 32);
            ++rows;
            club_rows += j.kind == kDjClubs;
        }
        for (size_t e = 0; e < out.size(); ++e)
            if (out[e] != want[e]) FAIL("E k %d job %d (kind %d cap %d) key %zu: %016llx want %016llx", k, (int)(e / k), jobs[e / k].kind, jobs[e / k].cap, e % k,
                                        (unsigned long long)out[e], (unsigned long long)want[e]);
        free_all();
    }
    printf("E rows %ld club_rows %ld short_rows %ld tie_pairs %ld\n", rows, club_rows, short_rows, tie_pairs);
}

int main() {
    part_a();
    part_b();
    part_c();
    part_d();
    part_e();
    printf("OK\n");
    return 0;
}
