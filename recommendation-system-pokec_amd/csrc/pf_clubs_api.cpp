// pf_clubs_api.cpp — the host part of clubs by interest (pokec_fas.h "Clubs by interest"): the three
// calls run the scan underneath with options of their own (the query's window and cap, the context's
// filter and selection; SyncScan with nothing stored in the context) and hand the ranked keys it
// left on the device (d_coll_sorted) to the stage (pf_clubsum.h).  The synchronous scans, the window
// check and the group call's seed resolution: pf_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "pf_clubsum.h"
#include "pf_debug.h"
#include "pf_host.h"

namespace {

int clubs_args(pf_ctx* c, const pf_clubs_query* q, int32_t topk, const int32_t* oclub, const float* oscore, const int32_t* oc) {
    if (!c) return PF_EINVAL;
    if (!q || !oc) return c->fail(PF_EINVAL, "clubs by interest: null query or out_count");
    if (topk < 0) return c->fail(PF_EINVAL, "clubs by interest: negative topk");
    if (topk && (!oclub || !oscore)) return c->fail(PF_EINVAL, "clubs by interest: null output with topk > 0");
    if (q->cap <= 0 || q->cap > (int64_t)INT32_MAX) return c->fail(PF_EINVAL, "clubs by interest: cap below 1 or above INT32_MAX");
    if (q->neighbours < 0) return c->fail(PF_EINVAL, "clubs by interest: negative neighbours");
    if (q->flags & ~PF_CLUBS_KEEP_OWN) return c->fail(PF_EINVAL, "clubs by interest: unknown flag bits");
    if (c->n_shards > 1)
        return c->fail(PF_EUNSUPP, "clubs by interest: a sharded context (partial sums of shards cannot be merged in rank order)");
    if (!c->jb.ok) return c->fail(PF_EUNSUPP, "clubs by interest: the job pipeline's club tables are unavailable: " + c->jb.why);
    return PF_OK;
}

// club ids -> the dense indices of those the corpus knows (a club nobody holds has no neighbour's add)
void own_dense(const pf_ctx* c, const uint32_t* ids, int64_t n, std::vector<int32_t>& out) {
    const std::vector<int32_t>& tab = c->jb.club_id;
    for (int64_t i = 0; i < n; ++i) {
        const auto it = std::lower_bound(tab.begin(), tab.end(), (int32_t)ids[i]);
        if (it != tab.end() && *it == (int32_t)ids[i]) out.push_back((int32_t)(it - tab.begin()));
    }
}
void own_of_idx(const pf_ctx* c, int32_t idx, std::vector<int32_t>& out) {
    own_dense(c, c->hc.clubs.data() + c->hc.club_off[(size_t)idx], c->hc.club_off[(size_t)idx + 1] - c->hc.club_off[(size_t)idx], out);
}

// scan(S): the collecting scan underneath, with the window and collector of this call as its options
template <class Scan>
int clubs_run(pf_ctx* c, const pf_clubs_query* q, int32_t topk, const std::vector<int32_t>& own, Scan scan, int32_t* oclub,
              float* oscore, int32_t* oc, pf_clubs_info* info) {
    *oc = 0;
    if (info) *info = pf_clubs_info{0, 0, 0, 0};
    if (topk == 0) return PF_OK;
    (void)hipSetDevice(c->device);
    pf_scan_window given{}, w;
    if (q->window) {
        given = *q->window;
        given.fields &= ~PF_WIN_COUNT;  // the collecting scan counts for itself and stores no totals
    }
    int rc = pf::make_window(c, &given, w);
    if (rc != PF_OK) return rc;
    if ((rc = pf::collect_reserve(c, q->cap)) != PF_OK) return rc;
    pf::SyncScan S(c, w, q->cap);
    if ((rc = scan(S)) != PF_OK) return rc;
    const int64_t total = S.total;
    if (info) info->total = total;
    if (total == 0 || total > q->cap) return PF_OK;
    const int64_t used = q->neighbours > 0 ? std::min<int64_t>(q->neighbours, total) : total;
    pf::ClubSumIn in{};
    in.keys = c->d_coll_sorted.as<uint64_t>();
    in.used = used;
    in.uid = c->jb.js.g_uid;  // the first n nodes are the profiles, in idx (= uid) order
    in.n_users = c->hc.n;
    in.n_club_ids = c->jb.js.n_club_ids;
    in.club_off = c->jb.js.club_off;
    in.club_dense = c->jb.js.club_dense;
    in.club_id = c->jb.js.club_id;
    const bool keep_own = (q->flags & PF_CLUBS_KEEP_OWN) != 0u;
    in.own = keep_own ? nullptr : own.data();
    in.n_own = keep_own ? 0 : (int32_t)own.size();
    in.topk = topk;
    in.cutover = (int32_t)pf::debug_long("clubs_cutover", 0);
    pf::ClubSumOut out;
    hipError_t err = hipSuccess;
    switch (pf::clubsum_run(in, c->clubs_ws, c->stream, oclub, oscore, &out, &err)) {
        case pf::kClubSumOk: break;
        case pf::kClubSumTooMany: return c->fail(PF_EUNSUPP, "clubs by interest: more than INT32_MAX contributions (lower neighbours)");
        case pf::kClubSumNoMem: return c->fail(PF_ENOMEM, "clubs by interest: no device memory for the stage's buffers");
        default: return c->hip_fail(err, "clubs by interest");
    }
    *oc = out.count;
    if (info) {
        info->used = used;
        info->contributions = out.contributions;
        info->clubs = out.clubs;
    }
    return PF_OK;
}

}  // namespace

extern "C" {

int pf_recommend_clubs_interest(pf_ctx* c, int32_t uid, const pf_clubs_query* q, int32_t topk, int32_t* oclub, float* oscore,
                                int32_t* oc, pf_clubs_info* info) {
    const int rc = clubs_args(c, q, topk, oclub, oscore, oc);
    if (rc != PF_OK) return rc;
    std::vector<int32_t> own;
    const int32_t idx = c->hc.idx_of(uid);
    if (idx >= 0) own_of_idx(c, idx, own);
    return clubs_run(c, q, topk, own, [&](pf::SyncScan& S) {
        int32_t u = 0, n = 0;
        float s = 0.f;
        return pf::recommend_uids(c, S, &uid, 1, 1, &u, &s, &n);
    }, oclub, oscore, oc, info);
}

int pf_recommend_clubs_profile(pf_ctx* c, const pf_query_profile* p, const pf_clubs_query* q, int32_t topk, int32_t* oclub,
                               float* oscore, int32_t* oc, pf_clubs_info* info) {
    const int rc = clubs_args(c, q, topk, oclub, oscore, oc);
    if (rc != PF_OK) return rc;
    if (!p) return c->fail(PF_EINVAL, "clubs by interest: null profile");
    std::vector<int32_t> own;
    if (p->n_clubs > 0 && p->club_ids) own_dense(c, p->club_ids, p->n_clubs, own);
    return clubs_run(c, q, topk, own, [&](pf::SyncScan& S) {
        int32_t u = 0, n = 0;
        float s = 0.f;
        std::vector<pf::ProfileOwned> ps;
        const int prc = pf::resolve_profiles(c, p, 1, ps);
        return prc != PF_OK ? prc : pf::recommend_profiles(c, S, ps, 1, &u, &s, &n);
    }, oclub, oscore, oc, info);
}

int pf_recommend_clubs_group(pf_ctx* c, const pf_group_query* g, const pf_clubs_query* q, int32_t topk, int32_t* oclub,
                             float* oscore, int32_t* oc, pf_clubs_info* info) {
    int rc = clubs_args(c, q, topk, oclub, oscore, oc);
    if (rc != PF_OK) return rc;
    if (!g) return c->fail(PF_EINVAL, "clubs by interest: null group");
    if ((rc = pf::group_args(c, g)) != PF_OK) return rc;
    std::vector<int32_t> own;
    for (int32_t idx : pf::group_seeds(c, *g)) own_of_idx(c, idx, own);
    return clubs_run(c, q, topk, own, [&](pf::SyncScan& S) {
        int32_t u = 0, n = 0;
        float s = 0.f;
        return pf::recommend_groups(c, S, g, 1, 1, &u, &s, &n);
    }, oclub, oscore, oc, info);
}

}  // extern "C"
