// Device check of the query-image builder K6 (qimage_kernel, pf_jobs.hip) on synthetic users of this
// probe's own making.  Links the product's own objects (build/pf_jobs_k.o, pf_store.o, pf_idf_k.o): the
// corpus goes through build_host_corpus and build_store, K6's tables and image sizes come from the
// planner's own rule (pf_jobs.h build_img_tables / build_img_plan / img_batch), and launch_qimages runs
// once per corpus and once more with every ImgJob::rows forced to the device bisection.  One packed
// corpus (P) and one wide one (W).  Every image is checked exactly against host expectations:
//   QConst   byte-equal to build_query's, hmul aside;
//   values   bit-equal to {(double)tf * (double)idf, (double)idf} by a plain loop over the corpus rows;
//   table    as a multiset: the distinct clubs, distinct friends and tokens of the raw rows (std::set),
//            each once, each at cuckoo_h1 or cuckoo_h2 of its key under the image's hmul, the exclusion
//            table empty, hmul one of the 16 multipliers, and the same entry set as build_query's;
//   *fail    0; the pool bytes between and around the images and the scratch guard untouched.
// Prints one summary line per corpus and OK.  A HIP error ends the probe at once; mismatches are
// listed (FAIL ...) after the corpus's launches and the probe exits 1 without another launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <set>
#include <string>
#include <vector>

#include "pf_jobs.h"
#include "pf_store.h"
#include "pf_types.h"
using namespace pf;

#define DIE(...) do { printf("FAIL "); printf(__VA_ARGS__); printf("\n"); fflush(stdout); exit(1); } while (0)
#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) DIE("%s: %s", #x, hipGetErrorString(e_)); } while (0)

static int g_bad = 0;
#define BAD(...) do { if (++g_bad <= 60) { printf("FAIL "); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const uint8_t FILL = 0xA5;  // the pool and the scratch start as bytes of this
static const size_t GUARD = 4096, GAP = 32;
static const int T = 5, NO_IDF_COL = 2;

template <class V> static void* up(const V& v) {
    void* p;
    const size_t b = std::max<size_t>(v.size() * sizeof(typename V::value_type), 16);
    CK(hipMalloc(&p, b));
    CK(hipMemset(p, 0, b));
    if (v.size()) CK(hipMemcpy(p, v.data(), v.size() * sizeof(typename V::value_type), hipMemcpyHostToDevice));
    return p;
}

// ================================================================ the users
struct User {
    std::string cat;
    int32_t pub = 1, gen = 0, comp = 0, age = 0, reg[3] = {-1, -1, -1};
    std::vector<uint32_t> clubs, friends;
    std::vector<std::pair<int32_t, int32_t>> col[T];  // (token id, tf)
    int64_t ntok() const { int64_t s = 0; for (int t = 0; t < T; ++t) s += (int64_t)col[t].size(); return s; }
};

static int32_t tf_of(int64_t j) { return 1 + (int32_t)((j * 7 + 3) % 200); }
// n tokens over the columns round-robin, distinct ids per column
static void add_tokens(User& u, int64_t n, int32_t base = 0) {
    for (int64_t j = 0; j < n; ++j) u.col[j % T].emplace_back(base + (int32_t)(j / T) * 3 + (int32_t)(j % T), tf_of(j));
}
static void add_ids(std::vector<uint32_t>& v, int64_t n, uint32_t base, uint32_t step) {
    for (int64_t j = 0; j < n; ++j) v.push_back(base + (uint32_t)j * step);
}
static float idf_val(int t, int32_t tid) { return 0.25f + (float)((tid * 37 + t * 11) % 997) / 64.0f; }

// the build class the planner gives a user of nc distinct clubs, nf distinct friends, nt tokens
static int class_of(bool packed, int64_t nc, int64_t nf, int64_t nt) {
    ImgPlan p;
    p.packed = packed;
    p.lge = lg_for(0);
    const int lg = packed ? lg_for((size_t)(nc + nf + nt)) : std::max({lg_for((size_t)nc), lg_for((size_t)nf), lg_for((size_t)nt)});
    p.lg.assign(1, (uint8_t)lg);
    p.nset.assign(1, (int32_t)(nc + nf));
    p.ntok.assign(1, (int32_t)nt);
    p.rows.assign(1, 0u);
    return img_build_class(p, 0);
}

// restated from qimage_kernel's step 3 (packed format): the set's key of a word and its first slot
static uint32_t set_key_packed(bool club, uint32_t id) { return (id + 1u) | (club ? 0u : 0x80000000u); }
static uint32_t set_home(uint32_t key, uint32_t dmask) { return ((key * 0x9E3779B1u) >> 5) & dmask; }

struct Edge { size_t lo, hi; };  // users on the two sides of a class boundary

struct Plant {
    std::vector<User> u;
    std::vector<Edge> edges;
    std::vector<size_t> retry, wrap_users;
    int wrap_words = 0;
    size_t add(const std::string& cat) {
        User x;
        x.cat = cat;
        const size_t i = u.size();
        // as many distinct completion values as ages, at other table rows but for the first and the last
        static const int32_t vals[] = {0, 1, 128, 129, 32767, 50, 77, 2}, ages[] = {0, 1, 128, 129, 32767, 18, 33, 64};
        x.comp = vals[i % 8];
        x.age = ages[(i / 2 + 3) % 8];
        x.pub = i % 5 == 0 ? -1 : (int32_t)(i % 2);
        x.gen = i % 3 == 0 ? -1 : (int32_t)(i % 3) - 1;
        const int rc = (int)(i % 4);
        for (int k = 0; k < rc; ++k) x.reg[k] = (int32_t)(3 + (i + k) % 4);
        if (i % 8 == 5) { x.reg[0] = -1; x.reg[1] = 6; x.reg[2] = -1; }  // one part, not the first
        u.push_back(x);
        return i;
    }
};

static void plant(bool packed, Plant& P) {
    // class boundaries, reached through tokens and through friends (the set's share of the LDS)
    for (int kind = 0; kind < 2; ++kind) {
        int found = 0;
        for (int64_t n = 1; n < 6000; ++n) {
            const int a = kind ? class_of(packed, 0, n, 0) : class_of(packed, 0, 0, n);
            const int b = kind ? class_of(packed, 0, n + 1, 0) : class_of(packed, 0, 0, n + 1);
            if (a == b) continue;
            ++found;
            Edge e;
            for (int side = 0; side < 2; ++side) {
                const size_t i = P.add(std::string(kind ? "edge_friends_" : "edge_tokens_") + std::to_string(n + side));
                if (kind) add_ids(P.u[i].friends, n + side, 1000, 3);
                else add_tokens(P.u[i], n + side);
                (side ? e.hi : e.lo) = i;
            }
            P.edges.push_back(e);
        }
        if (found != 2) DIE("expected two class boundaries, found %d (%s, kind %d)", found, packed ? "packed" : "wide", kind);
    }
    P.add("empty");
    add_ids(P.u[P.add("only_clubs")].clubs, 5, 40, 7);
    add_ids(P.u[P.add("only_friends")].friends, 5, 41, 7);
    add_tokens(P.u[P.add("only_tokens")], 5);
    for (int v : {1, 255, 256, 257, 513}) {  // the strides of 256 threads
        const size_t i = P.add("stride_" + std::to_string(v));
        add_ids(P.u[i].clubs, v / 2, 9, 5);
        add_ids(P.u[i].friends, v - v / 2, 9, 5);  // the same ids as the clubs: both kinds of most
        add_tokens(P.u[i], v, 100);
    }
    {
        const size_t i = P.add("repeats");
        P.u[i].clubs.assign(256, 77u);
        P.u[i].clubs.push_back(78u);
        P.u[i].friends = {5u, 5u, 9u};
    }
    {
        const size_t i = P.add("club_and_friend");
        P.u[i].clubs = {123u};
        P.u[i].friends = {123u};
    }
    {
        const size_t i = P.add("id_range");
        P.u[i].clubs = {0u, kIdLimit - 1u};
        P.u[i].friends = {kIdLimit - 1u, 0u};
    }
    for (int v : {7, 8, 511, 512}) {  // the set at its fullest: 2 nset + 2 on both sides of a power of two
        const size_t i = P.add("set_full_" + std::to_string(v));
        add_ids(P.u[i].clubs, v / 2, 1u << 20, 11);
        add_ids(P.u[i].friends, v - v / 2, 1u << 21, 13);
    }
    if (packed) {  // words whose probe sequences cluster on the set's last slots and wrap past its end
        const size_t i = P.add("set_wrap");
        const int nc = 6, nf = 6;
        const uint32_t dmask = (1u << pow2_lg(2 * (nc + nf) + 2)) - 1u;
        for (uint32_t id = 0; (int)P.u[i].clubs.size() < nc; ++id)
            if (set_home(set_key_packed(true, id), dmask) >= dmask - 1u) P.u[i].clubs.push_back(id);
        for (uint32_t id = 0; (int)P.u[i].friends.size() < nf; ++id)
            if (set_home(set_key_packed(false, id), dmask) == dmask) P.u[i].friends.push_back(id);
        P.wrap_users.push_back(i);
        P.wrap_words = nc + nf - 2;  // 12 distinct keys whose first slots are the last two: ten at least move past the end
    }
    {
        const size_t i = P.add("cols_all");
        for (int t = 0; t < T; ++t)
            for (int j = 0; j < 3; ++j) P.u[i].col[t].emplace_back(7 + 2 * j + t, 2 + j);
    }
    P.u[P.add("cols_last")].col[T - 1] = {{4, 9}, {11, 1}};
    {
        const size_t i = P.add("tf_edges");
        P.u[i].col[0] = {{1, 0}, {2, 255}};
        P.u[i].col[NO_IDF_COL] = {{3, 17}, {5, 1}};
        P.u[i].col[1] = {{3, 4}, {10, 6}};  // id 3 has no idf entry (1.0), id 10 has one
        if (!packed) P.u[i].col[3] = {{1, -5}, {2, (1 << 23) - 1}, {6, 300}, {7, -(1 << 23)}};
    }
    {  // three clubs with one {h1, h2} slot pair at lg 4 under the first multiplier: attempt 0 cannot place them
        const size_t i = P.add("retry");
        const uint32_t tag = packed ? kTagClub : 0u;
        bool done = false;
        for (int pair = 0; pair < 256 && !done; ++pair) {
            std::vector<uint32_t> ids;
            for (uint32_t id = 1; id < (1u << 16) && ids.size() < 3; ++id) {
                const uint32_t x = cuckoo_x(id | tag, kHashMul), a = cuckoo_h1(x, 4), b = cuckoo_h2(x, 4);
                if (a != b && (int)(std::min(a, b) * 16 + std::max(a, b)) == pair) ids.push_back(id);
            }
            if (ids.size() == 3) { P.u[i].clubs = ids; done = true; }
        }
        if (!done) DIE("no retry ids found");
        P.retry.push_back(i);
    }
    {  // one item whose two slots coincide
        const size_t i = P.add("h1_eq_h2");
        const uint32_t tag = packed ? kTagClub : 0u;
        for (uint32_t id = 1; P.u[i].clubs.empty(); ++id) {
            const uint32_t x = cuckoo_x(id | tag, kHashMul);
            if (cuckoo_h1(x, 4) == cuckoo_h2(x, 4)) P.u[i].clubs.push_back(id);
        }
        P.u[i].clubs.push_back(3u);
        P.u[i].friends = {4u};
    }
    if (!packed) {  // ids only the wide format takes
        size_t i = P.add("wide_club_2p31_friend_0");
        P.u[i].clubs = {0x80000000u};
        P.u[i].friends = {0u};
        i = P.add("wide_club_C5_friend_45");
        P.u[i].clubs = {0xC0000005u};
        P.u[i].friends = {0x40000005u};
        i = P.add("wide_club_ones");
        P.u[i].clubs = {0xFFFFFFFFu};
        i = P.add("wide_club_ones_x3");
        P.u[i].clubs = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        i = P.add("wide_friend_ones");
        P.u[i].friends = {0xFFFFFFFFu};
        i = P.add("wide_7F_both");
        P.u[i].friends = {0x7FFFFFFFu};
        P.u[i].clubs = {0x7FFFFFFFu};
    }
}

// ================================================================ one corpus
struct Counters {
    int images = 0, cls[3] = {0, 0, 0}, retries = 0, dup_words = 0, wrap = 0, bisect = 0, edges = 0, scr_nonzero = 0;
    int tokens = 0, entries = 0, wide_ids = 0;
};

struct Entry {
    uint64_t e;
    uint32_t slot;
};

static std::vector<uint64_t> aos_of(const uint32_t* w, uint32_t ntab, int lg, int lge) {  // the SoA layout undone
    const uint32_t excl = ntab << lg, total = excl + (1u << lge);
    std::vector<uint64_t> a(total);
    for (uint32_t i = 0; i < total; ++i) {
        uint32_t kw, vw;
        soa_words(i, excl, lg, lge, kw, vw);
        a[i] = (uint64_t)w[kw] | ((uint64_t)w[vw] << 32);
    }
    return a;
}

struct Run {
    bool packed;
    Plant P;
    HostCorpus hc;
    HostStore hs;
    ImgTables it;
    ImgPlan ip;
    std::vector<int64_t> off;  // per idx: its image's byte offset in the pool
    size_t pool_bytes = 0;
    std::vector<size_t> user_of_idx;
    DevStore ds{};
    DevJobsStore js{};
    Counters cn;
};

static void check_pool(Run& R, const std::vector<uint8_t>& pool, const char* pass) {
    const HostCorpus& hc = R.hc;
    const bool packed = R.packed;
    const uint32_t ntab = packed ? 1u : 3u;
    const uint64_t empty = packed ? kEmptyEntryPacked : kEmptyEntry;
    std::vector<uint8_t> owned(pool.size(), 0);
    for (int32_t idx = 0; idx < hc.n; ++idx) {
        const User& U = R.P.u[R.user_of_idx[idx]];
        const char* cat = U.cat.c_str();
        const ImgJob m = img_job(R.ip, idx, (uint32_t)R.off[idx]);
        const uint8_t* base = pool.data() + GUARD;
        const size_t nkeys = img_nkeys(R.ip, idx);
        const int64_t ntok = R.ip.ntok[idx];
        std::fill(owned.begin() + GUARD + m.const_off, owned.begin() + GUARD + m.const_off + sizeof(QConst), 1);
        std::fill(owned.begin() + GUARD + m.keys_off, owned.begin() + GUARD + m.keys_off + nkeys * 8, 1);
        std::fill(owned.begin() + GUARD + m.vals_off, owned.begin() + GUARD + m.vals_off + ntok * sizeof(QVal), 1);
        // ---- QConst against the host builder's
        QImageHost qh;
        if (!build_query(hc, packed, idx, nullptr, qh)) DIE("%s %s: build_query failed", pass, cat);
        if (qh.c.lg != R.ip.lg[idx]) DIE("%s %s: precondition: the host builder grew its table (lg %d, planner %d)", pass, cat, qh.c.lg, R.ip.lg[idx]);
        QConst got, want = qh.c;
        memcpy(&got, base + m.const_off, sizeof got);
        const uint32_t hmul = got.hmul;
        got.hmul = want.hmul = 0;
        if (memcmp(&got, &want, sizeof got) != 0) {
            const uint8_t *g = (const uint8_t*)&got, *w = (const uint8_t*)&want;
            size_t at = 0;
            while (g[at] == w[at]) ++at;
            BAD("%s %s: QConst differs from build_query's at byte %zu (lg %d/%d n_vals %d/%d)", pass, cat, at, got.lg, want.lg, got.n_vals, want.n_vals);
        }
        bool known = false;
        for (uint32_t s = 0; s < 16; ++s) known |= hmul == kHashMul + 2u * s * 0x6A09E667u;
        if (!known) BAD("%s %s: hmul %08x is none of the 16 multipliers", pass, cat, hmul);
        // ---- the expected values and entries, by plain loops over the corpus rows
        std::vector<uint64_t> exp[3];
        {
            std::set<uint32_t> sc(hc.clubs.begin() + hc.club_off[idx], hc.clubs.begin() + hc.club_off[idx + 1]);
            std::set<uint32_t> sf(hc.friends.begin() + hc.friend_off[idx], hc.friends.begin() + hc.friend_off[idx + 1]);
            for (uint32_t x : sc) exp[0].push_back(packed ? make_entry(x | kTagClub, 1u) : make_entry(x, 0u));
            for (uint32_t x : sf) exp[packed ? 0 : 1].push_back(packed ? make_entry(x, 0x10000u) : make_entry(x, 0u));
            R.cn.dup_words += (int)(R.ip.nset[idx] - (int64_t)sc.size() - (int64_t)sf.size());
        }
        const QVal* vals = reinterpret_cast<const QVal*>(base + m.vals_off);
        uint32_t vi = 0;
        for (int t = 0; t < hc.T; ++t)
            for (int64_t k = hc.tok_off[(size_t)idx * hc.T + t]; k < hc.tok_off[(size_t)idx * hc.T + t + 1]; ++k, ++vi) {
                const double idf = hc.has_idf[t] ? (double)hc.idf[t][hc.tid[k]] : 1.0;
                const QVal w{(double)hc.tf[k] * idf, idf};
                if (memcmp(&vals[vi], &w, sizeof w) != 0)
                    BAD("%s %s: vals[%u] = {%a, %a}, expected {%a, %a} (col %d tf %d)", pass, cat, vi, vals[vi].wq, vals[vi].idf, w.wq, w.idf, t, hc.tf[k]);
                exp[packed ? 0 : 2].push_back(packed ? make_entry(kTagTok | ((uint32_t)t << kTidBits) | (uint32_t)hc.tid[k], kTokVal | vi | ((uint32_t)t << kTidBits))
                                                     : make_entry((uint32_t)hc.tid[k] | ((uint32_t)t << kWideTidBits), (uint32_t)t | (vi << 8)));
                ++R.cn.tokens;
            }
        if ((int64_t)vi != ntok) DIE("%s %s: token count", pass, cat);
        // ---- the tables as multisets
        const int lg = m.lg;
        const std::vector<uint64_t> dev = aos_of(reinterpret_cast<const uint32_t*>(base + m.keys_off), ntab, lg, m.lge);
        const std::vector<uint64_t> host = aos_of(reinterpret_cast<const uint32_t*>(qh.keys.data()), ntab, lg, qh.c.lg_excl);
        if (qh.c.lg_excl != m.lge || host.size() != dev.size()) DIE("%s %s: exclusion table sizes", pass, cat);
        for (uint32_t k = 0; k < ntab; ++k) {
            std::vector<uint64_t> gotv, hostv;
            int misplaced = 0;
            for (uint32_t s = 0; s < (1u << lg); ++s) {
                const uint64_t e = dev[((size_t)k << lg) + s];
                if (host[((size_t)k << lg) + s] != empty) hostv.push_back(host[((size_t)k << lg) + s]);
                if (e == empty) continue;
                gotv.push_back(e);
                const uint32_t x = cuckoo_x((uint32_t)e, hmul);
                if (s != cuckoo_h1(x, lg) && s != cuckoo_h2(x, lg) && misplaced++ == 0)
                    BAD("%s %s: table %u entry %016llx sits at slot %u, not at its h1 %u or h2 %u", pass, cat, k, (unsigned long long)e, s, cuckoo_h1(x, lg), cuckoo_h2(x, lg));
            }
            if (misplaced > 1) BAD("%s %s: table %u: %d entries in all sit at neither of their slots", pass, cat, k, misplaced);
            std::sort(gotv.begin(), gotv.end());
            std::sort(hostv.begin(), hostv.end());
            std::sort(exp[k].begin(), exp[k].end());
            if (hostv != exp[k]) DIE("%s %s: table %u: build_query's entries differ from the rows' (%zu vs %zu)", pass, cat, k, hostv.size(), exp[k].size());
            if (gotv != exp[k]) {
                std::vector<uint64_t> miss, extra;
                std::set_difference(exp[k].begin(), exp[k].end(), gotv.begin(), gotv.end(), std::back_inserter(miss));
                std::set_difference(gotv.begin(), gotv.end(), exp[k].begin(), exp[k].end(), std::back_inserter(extra));
                BAD("%s %s: table %u holds %zu entries, expected %zu; missing %zu (first %016llx) extra or repeated %zu (first %016llx)", pass, cat, k,
                    gotv.size(), exp[k].size(), miss.size(), (unsigned long long)(miss.empty() ? 0 : miss[0]), extra.size(),
                    (unsigned long long)(extra.empty() ? 0 : extra[0]));
            }
            R.cn.entries += (int)gotv.size();
        }
        int excl_used = 0;
        for (uint32_t s = 0; s < (1u << m.lge); ++s) excl_used += dev[((size_t)ntab << lg) + s] != empty;
        if (excl_used) BAD("%s %s: %d exclusion slots are not empty", pass, cat, excl_used);
        if (hmul != kHashMul) ++R.cn.retries;
    }
    size_t stray = 0, first = 0;
    for (size_t b = 0; b < pool.size(); ++b)
        if (!owned[b] && pool[b] != FILL && stray++ == 0) first = b;
    if (stray) BAD("%s: %zu pool bytes outside the images were written (first at %zd from the pool's start)", pass, stray, (ssize_t)first - (ssize_t)GUARD);
}

static void run_corpus(bool packed, const char* name) {
    Run R;
    R.packed = packed;
    plant(packed, R.P);
    std::vector<User>& U = R.P.u;
    const int32_t n = (int32_t)U.size();
    // ---- pf_corpus_desc
    std::vector<int32_t> uid(n), pub(n), comp(n), gen(n), age(n), reg(3 * n), tid, tf;
    std::vector<int64_t> coff(n + 1, 0), foff(n + 1, 0), toff((size_t)n * T + 1, 0);
    std::vector<uint32_t> clubs, friends;
    for (int32_t i = 0; i < n; ++i) {
        uid[i] = 10 + 3 * i;
        pub[i] = U[i].pub; gen[i] = U[i].gen; comp[i] = U[i].comp; age[i] = U[i].age;
        for (int k = 0; k < 3; ++k) reg[3 * i + k] = U[i].reg[k];
        clubs.insert(clubs.end(), U[i].clubs.begin(), U[i].clubs.end());
        friends.insert(friends.end(), U[i].friends.begin(), U[i].friends.end());
        coff[i + 1] = (int64_t)clubs.size();
        foff[i + 1] = (int64_t)friends.size();
        for (int t = 0; t < T; ++t) {
            for (auto& kv : U[i].col[t]) { tid.push_back(kv.first); tf.push_back(kv.second); }
            toff[(size_t)i * T + t + 1] = (int64_t)tid.size();
        }
    }
    if (clubs.empty()) clubs.push_back(0);
    std::vector<uint8_t> has_idf(T, 1), npres(kNumFixed + T, 0);
    has_idf[NO_IDF_COL] = 0;
    std::vector<int64_t> ioff(T + 1, 0);
    std::vector<int32_t> itid;
    std::vector<float> ival;
    for (int t = 0; t < T; ++t) {
        if (has_idf[t])
            for (int32_t k = 0; k < 4000; ++k)
                if (k % 7 != 3) { itid.push_back(k); ival.push_back(idf_val(t, k)); }
        ioff[t + 1] = (int64_t)itid.size();
    }
    std::vector<float> nmean(kNumFixed + T, 0.f), nsd(kNumFixed + T, 0.f);
    for (int k = 0; k < kNumFixed + T; k += 2) { npres[k] = 1; nmean[k] = 0.1f + 0.01f * k; nsd[k] = 0.2f + 0.02f * k; }
    pf_corpus_desc d{};
    d.n_users = n; d.n_cols = T;
    d.user_id = uid.data(); d.public_flag = pub.data(); d.completion = comp.data(); d.gender = gen.data(); d.age = age.data();
    d.region = reg.data();
    d.club_off = coff.data(); d.club_ids = clubs.data(); d.friend_off = foff.data(); d.friend_ids = friends.data();
    d.tok_off = toff.data(); d.tok_tid = tid.data(); d.tok_tf = tf.data();
    d.idf_mode = PF_IDF_EXPLICIT;
    d.col_has_idf = has_idf.data(); d.idf_off = ioff.data(); d.idf_tid = itid.data(); d.idf_val = ival.data();
    d.norm_present = npres.data(); d.norm_mean = nmean.data(); d.norm_sd = nsd.data();
    std::string err;
    if (build_host_corpus(&d, R.hc, err) != PF_OK) DIE("%s: build_host_corpus: %s", name, err.c_str());
    if (build_store(R.hc, R.hs, err) != PF_OK) DIE("%s: build_store: %s", name, err.c_str());
    if (R.hs.packed != packed) DIE("%s: the store is %s", name, R.hs.packed ? "packed" : "wide");
    R.user_of_idx.resize(n);
    for (int32_t i = 0; i < n; ++i) R.user_of_idx[R.hc.idx_of(uid[i])] = (size_t)i;  // uids ascend: the identity
    // ---- the planner's tables and sizes
    build_img_tables(R.hc, packed, R.it);
    build_img_plan(R.hc, R.hs, R.it, R.ip);
    for (int32_t i = 0; i < n; ++i)
        if (!R.ip.lg[i]) DIE("%s %s: outside the device limits", name, U[i].cat.c_str());
    for (const Edge& e : R.P.edges) {
        const int a = img_build_class(R.ip, R.hc.idx_of(uid[e.lo])), b = img_build_class(R.ip, R.hc.idx_of(uid[e.hi]));
        if (b != a + 1) DIE("%s: %s / %s are in classes %d / %d", name, U[e.lo].cat.c_str(), U[e.hi].cat.c_str(), a, b);
        ++R.cn.edges;
    }
    for (size_t w : R.P.wrap_users) {  // the wrap ids were searched for this set size
        const int32_t idx = R.hc.idx_of(uid[w]);
        if (!packed || img_dlg(R.ip, idx) != pow2_lg(2 * (int64_t)R.ip.nset[idx] + 2)) DIE("%s: the wrap ids were built for another set size", name);
        R.cn.wrap += R.P.wrap_words;
    }
    // ---- device inputs: the five DevStore members K6 reads and the K6 part of DevJobsStore
    R.ds.hdr0 = (const uint4*)up(R.hs.hdr0);
    R.ds.hdr1 = (const uint4*)up(R.hs.hdr1);
    R.ds.hdr2 = (const uint4*)up(R.hs.hdr2);
    R.ds.rows = (const uint4*)up(R.hs.rows);
    R.ds.row_off = (const uint64_t*)up(R.hs.row_off);
    R.ds.n_slots = n;
    R.ds.packed = packed ? 1 : 0;
    R.ds.n_cols = T;
    std::vector<QConst> tv(1, R.it.tmpl);
    R.js.tmpl = (const QConst*)up(tv);
    R.js.sig_reg = (const double*)up(R.it.sig_reg);
    R.js.comp_vals = (const int32_t*)up(R.it.comp_vals);
    R.js.comp_rows = (const double*)up(R.it.comp_rows);
    R.js.age_vals = (const int32_t*)up(R.it.age_vals);
    R.js.age_rows = (const double*)up(R.it.age_rows);
    R.js.n_comp = (int32_t)R.it.comp_vals.size();
    R.js.n_age = (int32_t)R.it.age_vals.size();
    R.js.idf_dense_off = (const int64_t*)up(R.it.dense_off);
    R.js.idf_dense_len = (const int32_t*)up(R.it.dense_len);
    R.js.idf_dense = (const float*)up(R.it.dense);
    R.js.slot_of = (const int32_t*)up(R.hs.slot_of_idx);
    R.js.n = n;
    // ---- the images, GAP filler bytes apart, ordered as build_resident_images orders them
    R.off.assign(n, 0);
    std::vector<ImgJob> ij;
    size_t at = 0;
    for (int32_t idx = 0; idx < n; ++idx) {
        R.off[idx] = (int64_t)at;
        ij.push_back(img_job(R.ip, idx, (uint32_t)at));
        at += img_bytes(R.ip, idx) + GAP;
    }
    R.pool_bytes = at;
    ImgBatch B;
    img_batch(R.ip, ij, B);
    for (int k = 0; k < 3; ++k) R.cn.cls[k] = B.nc[k];
    R.cn.images = n;
    for (int x = B.nc[0] + B.nc[1]; x < (int)B.ij.size(); ++x) R.cn.scr_nonzero += B.ij[x].scr_off != 0;
    if (B.nc[2] < 2) DIE("%s: fewer than two global builds", name);
    // bounds of everything the launch may write, before it runs
    for (size_t x = 0; x < B.ij.size(); ++x) {
        const ImgJob& m = B.ij[x];
        const bool glob = (int)x >= B.nc[0] + B.nc[1];
        if ((size_t)m.const_off + img_bytes(R.ip, m.idx) > R.pool_bytes || m.const_off % 16 != 0) DIE("%s: image out of the pool", name);
        if (glob && m.scr_off + img_scratch_words(R.ip, m.idx) > B.scr) DIE("%s: scratch out of bounds", name);
        if (!glob && qimage_lds(m.lg, m.lge, m.dlg, (uint32_t)(R.ip.nset[m.idx] + R.ip.ntok[m.idx]), packed) == 0) DIE("%s: LDS build too large", name);
    }
    uint8_t* d_pool;
    uint32_t* d_scr;
    int32_t* d_fail;
    const size_t scr_bytes = (size_t)B.scr * 4 + GUARD;
    CK(hipMalloc((void**)&d_pool, R.pool_bytes + 2 * GUARD));
    CK(hipMalloc((void**)&d_scr, scr_bytes));
    CK(hipMalloc((void**)&d_fail, 16));
    std::vector<uint8_t> first;
    for (int pass = 0; pass < 2; ++pass) {  // pass 1: the completion / age rows by device bisection
        std::vector<ImgJob> jobs = B.ij;
        if (pass)
            for (ImgJob& m : jobs) m.rows = 0xFFFFFFFFu;
        const ImgJob* d_ij = (const ImgJob*)up(jobs);
        CK(hipMemset(d_pool, FILL, R.pool_bytes + 2 * GUARD));
        CK(hipMemset(d_scr, FILL, scr_bytes));
        CK(hipMemset(d_fail, 0, 16));
        CK(launch_qimages(R.ds, R.js, d_ij, B.nc[0], B.nc[1], B.nc[2], d_pool + GUARD, d_scr, d_fail, nullptr));
        CK(hipDeviceSynchronize());
        int32_t failed = -1;
        CK(hipMemcpy(&failed, d_fail, 4, hipMemcpyDeviceToHost));
        std::vector<uint8_t> pool(R.pool_bytes + 2 * GUARD), sg(GUARD);
        CK(hipMemcpy(pool.data(), d_pool, pool.size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(sg.data(), (uint8_t*)d_scr + (size_t)B.scr * 4, GUARD, hipMemcpyDeviceToHost));
        const std::string label = std::string(name) + (pass ? " bisect" : "");
        if (failed != 0) BAD("%s: *fail = %d after the launch", label.c_str(), failed);
        for (uint8_t b : sg)
            if (b != FILL) { BAD("%s: the scratch guard was written", label.c_str()); break; }
        const Counters keep = R.cn;
        check_pool(R, pool, label.c_str());
        if (pass) {  // identical to the first launch's images but for the tables' placement
            R.cn = keep;  // counted once
            R.cn.bisect = n;
            for (int32_t idx = 0; idx < n; ++idx) {
                const ImgJob m = img_job(R.ip, idx, (uint32_t)R.off[idx]);
                QConst a, b;
                memcpy(&a, pool.data() + GUARD + m.const_off, sizeof a);
                memcpy(&b, first.data() + GUARD + m.const_off, sizeof b);
                a.hmul = b.hmul = 0;
                if (memcmp(&a, &b, sizeof a) != 0 ||
                    memcmp(pool.data() + GUARD + m.vals_off, first.data() + GUARD + m.vals_off, (size_t)R.ip.ntok[idx] * sizeof(QVal)) != 0)
                    BAD("%s %s: the image differs from the first launch's", label.c_str(), U[R.user_of_idx[idx]].cat.c_str());
            }
        } else {
            first = pool;
        }
    }
    for (size_t r : R.P.retry) {
        QConst c;
        memcpy(&c, first.data() + GUARD + R.off[R.hc.idx_of(uid[r])], sizeof c);
        if (c.hmul == kHashMul) BAD("%s retry: the table was placed under the first multiplier", name);
    }
    if (!packed)
        for (const User& x : U) R.cn.wide_ids += x.cat.compare(0, 5, "wide_") == 0;
    const Counters& c = R.cn;
    printf("%s images %d small %d big %d global %d scr_nonzero %d edges %d retries %d dup_words %d tokens %d entries %d bisect %d", name, c.images,
           c.cls[0], c.cls[1], c.cls[2], c.scr_nonzero, c.edges, c.retries, c.dup_words, c.tokens, c.entries, c.bisect);
    if (packed) printf(" wrap %d\n", c.wrap);
    else printf(" wide_ids %d\n", c.wide_ids);
    fflush(stdout);
    if (g_bad) {
        printf("FAIL %s: %d mismatches\n", name, g_bad);
        exit(1);
    }
}

// --edges: the class boundaries the planner's rule gives (no device work), for the test that puts users
// of these sizes through the public calls: per format and kind, the last size of the lower class
static void print_edges() {
    for (int packed = 1; packed >= 0; --packed) {
        printf("edges %s", packed ? "P" : "W");
        for (int kind = 0; kind < 2; ++kind) {
            printf(" %s", kind ? "friends" : "tokens");
            for (int64_t n = 1; n < 6000; ++n)
                if ((kind ? class_of(packed, 0, n, 0) : class_of(packed, 0, 0, n)) != (kind ? class_of(packed, 0, n + 1, 0) : class_of(packed, 0, 0, n + 1)))
                    printf(" %lld", (long long)n);
        }
        printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "--edges") == 0) {
        print_edges();
        return 0;
    }
    CK(hipSetDevice(0));
    run_corpus(true, "P");
    run_corpus(false, "W");
    printf("OK\n");
    return 0;
}
