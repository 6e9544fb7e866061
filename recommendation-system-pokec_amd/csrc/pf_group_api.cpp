// pf_group_api.cpp — the host part of the group query (pokec_fas.h "Group query"): seed resolution, the
// exclusion union, the pass plan and the launches of fas_group_kernel (pf_group.h), and
// pf_group_scores through the pair kernel (image staging and the pair runner: pf_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <unordered_set>
#include <vector>

#include "pf_debug.h"
#include "pf_group.h"
#include "pf_host.h"

namespace pf {

namespace {

// PF_DEBUG group_tile=N caps the images of a pass; group_lds=BYTES sets a pass's LDS budget
int group_tile() {
    static const int n = (int)std::max(0L, pf::debug_long("group_tile", 0));
    return n;
}
uint32_t group_budget() {
    static const uint32_t b = (uint32_t)std::min<long>(160L * 1024L, std::max(0L, pf::debug_long("group_lds", pf::kGroupLdsBudgetDefault)));
    return b;
}

// the aggregate of G per-seed scores s[g * stride], in seed order (pokec_fas.h "Aggregate")
float group_aggregate(int agg, const float* s, size_t G, size_t stride) {
    if (agg == PF_GROUP_MEAN) {
        double acc = 0.0;
        for (size_t g = 0; g < G; ++g) acc += (double)s[g * stride];
        return (float)(acc / (double)G);
    }
    float m = s[0];
    for (size_t g = 1; g < G; ++g) {
        const float x = s[g * stride];
        if (agg == PF_GROUP_MIN ? x < m : x > m) m = x;
    }
    return m;
}

}  // namespace

int group_args(pf_ctx* c, const pf_group_query* g) {
    if (g->n_seeds < 0 || g->n_exclude < 0) return c->fail(PF_EINVAL, "group query: negative count");
    if (g->n_seeds > PF_GROUP_MAX_SEEDS) return c->fail(PF_EINVAL, "group query: more than PF_GROUP_MAX_SEEDS seeds");
    if (g->agg != PF_GROUP_MEAN && g->agg != PF_GROUP_MIN && g->agg != PF_GROUP_MAX)
        return c->fail(PF_EINVAL, "group query: unknown aggregate");
    if (g->flags & ~PF_GROUP_EXCLUDE_ADJ) return c->fail(PF_EINVAL, "group query: unknown flag bits");
    if ((g->n_seeds && !g->seed_uid) || (g->n_exclude && !g->exclude_uid))
        return c->fail(PF_EINVAL, "group query: null array with a positive count");
    return PF_OK;
}

// the kept seeds, as corpus indices in the caller's order
std::vector<int32_t> group_seeds(const pf_ctx* c, const pf_group_query& g) {
    std::vector<int32_t> idx;
    std::unordered_set<int32_t> seen;
    for (int32_t i = 0; i < g.n_seeds; ++i) {
        const int32_t x = c->hc.idx_of(g.seed_uid[i]);
        if (x >= 0 && seen.insert(x).second) idx.push_back(x);
    }
    return idx;
}

namespace {

// What one group launches: the images (the last one carries the exclusion union), their carve
// offsets and the passes.
struct GroupPlan {
    std::vector<int32_t> idx;
    Images im;
    std::vector<uint32_t> img_lds, off;
    std::vector<pf::GroupPass> passes;
    uint32_t hit_bytes = 0;
    int n_global = 0;
};

int group_plan(pf_ctx* c, const pf_group_query& g, GroupPlan& P) {
    P.idx = group_seeds(c, g);
    const size_t G = P.idx.size();
    if (G == 0) return PF_OK;
    std::vector<int32_t> excl;
    for (int32_t i : P.idx) excl.push_back(c->hc.uid[i]);
    for (int32_t i = 0; i < g.n_exclude; ++i)
        if (c->hc.idx_of(g.exclude_uid[i]) >= 0) excl.push_back(g.exclude_uid[i]);
    if (g.flags & PF_GROUP_EXCLUDE_ADJ)
        for (int32_t i : P.idx) {
            auto it = c->hc.adj.find(c->hc.uid[i]);
            if (it != c->hc.adj.end()) excl.insert(excl.end(), it->second.begin(), it->second.end());
        }
    std::sort(excl.begin(), excl.end());
    excl.erase(std::unique(excl.begin(), excl.end()), excl.end());
    if (excl.size() > (size_t)PF_GROUP_MAX_EXCLUDE)
        return c->fail(PF_EUNSUPP, "group query: exclusion union above PF_GROUP_MAX_EXCLUDE uids");
    std::vector<pf::QImageHost> qi(G);
    std::vector<uint8_t> ok(G, 1);
    par_jobs(G, [&](size_t i) { ok[i] = pf::build_query(c->hc, c->hs.packed, P.idx[i], i + 1 == G ? &excl : nullptr, qi[i]) ? 1 : 0; });
    std::vector<uint8_t> glob(G, 0);
    for (size_t i = 0; i < G; ++i) {
        if (!ok[i]) return c->fail(PF_EUNSUPP, "query hash table too large");
        add_image(P.im, qi[i]);
        P.hit_bytes = std::max(P.hit_bytes, qi[i].c.n_hits_max);
        glob[i] = P.im.refs[i].lds_bytes == 0;
        P.n_global += glob[i];
        P.img_lds.push_back((uint32_t)sizeof(pf::QConst) + P.im.refs[i].lds_bytes);
    }
    P.passes = pf::group_pack(P.img_lds, glob, P.hit_bytes, group_budget(), group_tile(), P.off);
    return PF_OK;
}

// One group's passes on the context's stream, its k keys into d_keys, with x the call's options for
// this group (its own count word).  One pinned staging buffer [refs | offsets | sync | image pool] goes
// up in a single copy, as in scan_stream_images.
int group_scan(pf_ctx* c, const pf::ScanExtras& x, const GroupPlan& P, int agg, int k, uint64_t* d_keys, bool timed) {
    const size_t G = P.idx.size();
    const int tiles = c->tile_end - c->tile_begin;
    const StageLayout<4> L = stage_group_layout(G, sizeof(pf::QImageRef), sizeof(pf::ScanSync), P.im.pool.size());
    const StagePiece pool{P.im.pool.data(), P.im.pool.size()};
    uint8_t* base = nullptr;
    int rc = stage_send(c, L, {P.im.refs.data(), P.off.data(), nullptr}, &pool, 1, c->d_pool, c->stream, base);
    if (rc != PF_OK) return rc;
    if (P.passes.size() > 1) HIPCHK(c, c->d_scores.ensure((size_t)std::max(1, c->ds.n_slots) * sizeof(double)));
    std::vector<int> blocks(P.passes.size());
    for (size_t p = 0; p < P.passes.size(); ++p) {
        const int per_cu = pf::group_blocks_per_cu(c->hs.packed, P.passes[p].gtab, P.passes[p].lds);
        blocks[p] = std::max(1, std::min((tiles + 3) / 4, c->num_cus * per_cu));
    }
    HIPCHK(c, c->d_part.ensure((size_t)(blocks.back() + 8) * k * sizeof(uint64_t)));
    hipEvent_t e0, e1;
    if ((rc = timed_begin(c, timed, e0, e1, c->stream)) != PF_OK) return rc;
    for (size_t p = 0; p < P.passes.size(); ++p)
        HIPCHK(c, pf::launch_group({.st = c->ds, .pool = base + L.off[3],
                                    .refs_dev = reinterpret_cast<const pf::QImageRef*>(base),
                                    .off_dev = reinterpret_cast<const uint32_t*>(base + L.off[1]), .pass = P.passes[p],
                                    .hit_bytes = P.hit_bytes, .first = p == 0, .last = p + 1 == P.passes.size(),
                                    .agg = agg, .n_seeds = (int)G, .excl_img = (int)G - 1, .tile_begin = c->tile_begin,
                                    .tile_end = c->tile_end, .k = k, .blocks = blocks[p], .acc = c->d_scores.as<double>(),
                                    .parts = c->d_part.as<uint64_t>(), .out = d_keys,
                                    .sync = reinterpret_cast<pf::ScanSync*>(base + L.off[2]), .s = c->stream,
                                    .x = x}));
    return timed_end(c, timed, e0, e1, c->stream);
}

}  // namespace

// pf_recommend_group's scans: group i's keys through row 0 of d_out, its count in word i (0 for G = 0);
// last_scan_ms is the last scanned group's
int recommend_groups(pf_ctx* c, SyncScan& S, const pf_group_query* g, int32_t ng, int32_t topk, int32_t* ou, float* os,
                     int32_t* oc) {
    int rc = S.begin(ng, 1, topk, false);
    if (rc != PF_OK) return rc;
    for (int32_t i = 0; i < ng; ++i) {
        GroupPlan P;
        if ((rc = group_plan(c, g[i], P)) != PF_OK) return rc;
        if (P.idx.empty()) continue;
        if ((rc = group_scan(c, S.call.group(i), P, g[i].agg, topk, c->d_out.as<uint64_t>(), true)) != PF_OK) return rc;
        if ((rc = S.keys(1, topk, true, ou + (size_t)i * topk, os + (size_t)i * topk, &oc[i])) != PF_OK) return rc;
    }
    return S.finish();
}

}  // namespace pf

extern "C" {

int pf_recommend_group(pf_ctx* c, const pf_group_query* g, int32_t ng, int32_t topk, int32_t* ou, float* os, int32_t* oc) {
    if (!c) return PF_EINVAL;
    if (ng < 0 || topk < 0) return c->fail(PF_EINVAL, "group query: negative ng / topk");
    if (ng && (!g || !oc || (topk && (!ou || !os)))) return c->fail(PF_EINVAL, "group query: null argument with ng > 0");
    for (int32_t i = 0; i < ng; ++i) {
        const int rc = pf::group_args(c, &g[i]);
        if (rc != PF_OK) return rc;
    }
    if (topk > pf::kMaxTopK) return c->fail(PF_EUNSUPP, "group query: topk above the scan kernels' bound (64)");
    (void)hipSetDevice(c->device);
    for (int32_t i = 0; i < ng; ++i) oc[i] = 0;
    if (topk == 0) return PF_OK;
    pf::SyncScan S(c);
    return pf::recommend_groups(c, S, g, ng, topk, ou, os, oc);
}

int pf_group_scores(pf_ctx* c, const pf_group_query* g, const int32_t* b, int64_t n, const pf_field_select* s, float* out) {
    if (!c) return PF_EINVAL;
    if (!g || n < 0 || (n && (!b || !out))) return c->fail(PF_EINVAL, "group scores: null argument");
    int rc = pf::group_args(c, g);
    if (rc != PF_OK) return rc;
    pf::FieldSel sel;
    if (pf::make_select(c, s, sel) != PF_OK) return c->fail(PF_EINVAL, "group scores: unknown bits in fixed / flags");
    (void)hipSetDevice(c->device);
    const std::vector<int32_t> idx = pf::group_seeds(c, *g);
    const size_t G = idx.size();
    for (int64_t i = 0; i < n; ++i) out[i] = NAN;
    if (G == 0 || n == 0) return PF_OK;
    // G x chunk pairs per launch of the pair kernel: every seed one group over the same candidates
    const int64_t chunk = std::max<int64_t>(1, ((int64_t)4 << 20) / (int64_t)G);
    for (int64_t b0 = 0; b0 < n; b0 += chunk) {
        const int64_t b1 = std::min(n, b0 + chunk);
        pf::PairGroups pg;  // one group: the candidates every seed shares
        pf::group_pairs(c, nullptr, b, b0, b1, pg);
        if (pg.slots.empty()) continue;
        const std::vector<int32_t>& slots = pg.slots[0];
        const std::vector<int64_t>& where = pg.dest[0];
        const std::vector<std::vector<int32_t>> gs(G, slots);
        std::vector<std::vector<float>> res;
        if ((rc = pf::run_pairs(c, idx, gs, res, nullptr, nullptr, sel)) != PF_OK) return rc;
        std::vector<float> col(G);
        for (size_t j = 0; j < slots.size(); ++j) {
            for (size_t q = 0; q < G; ++q) col[q] = res[q][j];
            out[where[j]] = pf::group_aggregate(g->agg, col.data(), G, 1);
        }
    }
    return PF_OK;
}

int pf_group_plan_of(pf_ctx* c, const pf_group_query* g, pf_group_plan* out) {
    if (!c) return PF_EINVAL;
    if (!g || !out) return c->fail(PF_EINVAL, "group plan: null argument");
    int rc = pf::group_args(c, g);
    if (rc != PF_OK) return rc;
    pf::GroupPlan P;
    if ((rc = pf::group_plan(c, *g, P)) != PF_OK) return rc;
    out->n_seeds = (int32_t)P.idx.size();
    out->n_passes = (int32_t)P.passes.size();
    out->n_global = P.n_global;
    out->pad = 0;
    out->stream_bytes = (int64_t)P.passes.size() * pf::k1_pass_bytes(c);
    return PF_OK;
}

int pf_group_image_lds(pf_ctx* c, const pf_group_query* g, int32_t* out, int32_t cap) {
    if (!c) return PF_EINVAL;
    if (!g || !out) return c->fail(PF_EINVAL, "group image lds: null argument");
    int rc = pf::group_args(c, g);
    if (rc != PF_OK) return rc;
    pf::GroupPlan P;
    if ((rc = pf::group_plan(c, *g, P)) != PF_OK) return rc;
    const size_t G = P.idx.size();
    if ((size_t)cap < G + 2) return c->fail(PF_EINVAL, "group image lds: out too small");
    for (size_t i = 0; i < G; ++i) out[i] = (int32_t)P.img_lds[i];
    out[G] = (int32_t)(P.hit_bytes * (uint32_t)pf::kScanThreads + pf::kGroupTailLds);
    out[G + 1] = (int32_t)pf::group_budget();
    return PF_OK;
}

}  // extern "C"
