// pf_diverse_api.cpp — the host part of diverse top-k (pokec_fas.h "Diverse top-k"): the three scan
// calls run the collecting scan underneath as the clubs calls do (pf_clubs_api.cpp: the query's window
// and cap, the context's filter and selection, SyncScan with nothing stored in the context), take the
// first M ranked keys it left on the device (d_coll_sorted) as the pool, score the pool's M x M pairs
// in one run_pairs whose matrix stays on the device, and hand both to the stage (pf_diverse.h).
// pf_diverse_rerank does the same for a list the caller holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <unordered_set>
#include <vector>

#include "pf_diverse.h"
#include "pf_host.h"

namespace {

const pf_diverse_info kNoInfo{0, 0, 0, 0};

bool lambda_ok(float l) { return l >= 0.f && l <= 1.f; }  // false for NaN

int diverse_args(pf_ctx* c, const pf_diverse_query* q, int32_t topk, const int32_t* ou, const float* os, const int32_t* oc) {
    if (!c) return PF_EINVAL;
    if (!q || !oc) return c->fail(PF_EINVAL, "diverse top-k: null query or out_count");
    if (topk < 0) return c->fail(PF_EINVAL, "diverse top-k: negative topk");
    if (topk && (!ou || !os)) return c->fail(PF_EINVAL, "diverse top-k: null output with topk > 0");
    if (q->cap <= 0 || q->cap > (int64_t)INT32_MAX) return c->fail(PF_EINVAL, "diverse top-k: cap below 1 or above INT32_MAX");
    if (q->pool < 1) return c->fail(PF_EINVAL, "diverse top-k: pool below 1");
    if (!lambda_ok(q->lambda)) return c->fail(PF_EINVAL, "diverse top-k: lambda outside [0, 1]");
    if (q->pool > PF_DIVERSE_MAX_POOL) return c->fail(PF_EUNSUPP, "diverse top-k: pool above PF_DIVERSE_MAX_POOL");
    if (c->n_shards > 1) return c->fail(PF_EUNSUPP, "diverse top-k: a sharded context (a shard's pool is not the ranking's)");
    return PF_OK;
}

// a device buffer that cannot be had is reported, not fatal: the sticky error is cleared
bool grow(pf::DBuf& b, size_t bytes) {
    if (b.ensure(std::max<size_t>(bytes, 16)) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// The pool's matrix, sim[s * M + i] = FAS(A = idx[s], B = idx[i]) under sel, left in diverse_ws.sim:
// M groups of M slots in one run_pairs (one chunk: M <= 4096 queries, M * M <= 8M pairs).
int pool_matrix(pf_ctx* c, const std::vector<int32_t>& idx, const pf::FieldSel& sel) {
    const size_t M = idx.size();
    if (!grow(c->diverse_ws.sim, M * M * sizeof(float))) return c->fail(PF_ENOMEM, "diverse top-k: no device memory for the pair matrix");
    std::vector<int32_t> row(M);
    for (size_t i = 0; i < M; ++i) row[i] = c->hs.slot_of_idx[(size_t)idx[i]];
    const std::vector<std::vector<int32_t>> slots(M, row);
    std::vector<std::vector<float>> res;
    std::vector<int64_t> goff;
    return pf::run_pairs(c, idx, slots, res, &c->diverse_ws.sim, &goff, sel);  // goff[g] = g * M
}

int run_stage(pf_ctx* c, const pf::DiverseIn& in, int32_t* ou, float* os, float* open_, double* oval, int32_t* oc) {
    hipError_t err = hipSuccess;
    switch (pf::diverse_run(in, c->diverse_ws, c->stream, ou, os, open_, oval, nullptr, oc, &err)) {
        case pf::kDiverseOk: return PF_OK;
        case pf::kDiverseNoMem: return c->fail(PF_ENOMEM, "diverse top-k: no device memory for the stage's picks");
        default: return c->hip_fail(err, "diverse top-k");
    }
}

// scan(S): the collecting scan underneath, with the window and collector of this call as its options
template <class Scan>
int diverse_scan(pf_ctx* c, const pf_diverse_query* q, int32_t topk, Scan scan, int32_t* ou, float* os, float* open_,
                 double* oval, int32_t* oc, pf_diverse_info* info) {
    *oc = 0;
    if (info) *info = kNoInfo;
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
    const size_t M = (size_t)std::min<int64_t>(q->pool, total);
    // the pool's keys, for grouping: its users' indices are the matrix's rows and columns
    std::vector<uint64_t> keys(M);
    HIPCHK(c, hipMemcpyAsync(keys.data(), c->d_coll_sorted.p, M * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> idx(M);
    for (size_t i = 0; i < M; ++i) {
        idx[i] = c->hc.idx_of(pf::key_uid(keys[i]));
        if (idx[i] < 0) return c->fail(PF_EINVAL, "diverse top-k: a ranked uid has no profile");  // cannot happen
    }
    if ((rc = pool_matrix(c, idx, c->sel)) != PF_OK) return rc;  // run_pairs touches no d_coll_* buffer
    pf::DiverseIn in{};
    in.keys = c->d_coll_sorted.as<uint64_t>();
    in.m = (int32_t)M;
    in.sim = c->diverse_ws.sim.as<float>();
    in.stride = (int64_t)M;
    in.lambda = q->lambda;
    in.topk = topk;
    if ((rc = run_stage(c, in, ou, os, open_, oval, oc)) != PF_OK) return rc;
    if (info) {
        info->pool = (int64_t)M;
        info->pairs = (int64_t)(M * M);
        info->picked = *oc;
    }
    return PF_OK;
}

}  // namespace

extern "C" {

int pf_diverse_rerank(pf_ctx* c, const int32_t* uid, const float* score, int64_t n, float lambda, int32_t topk,
                      const pf_field_select* select, int32_t* ou, float* os, float* open_, double* oval, int32_t* oc) {
    if (!c) return PF_EINVAL;
    if (!oc) return c->fail(PF_EINVAL, "diverse rerank: null out_count");
    *oc = 0;
    if (n < 0 || (n && (!uid || !score))) return c->fail(PF_EINVAL, "diverse rerank: negative n or a null list");
    if (topk < 0) return c->fail(PF_EINVAL, "diverse rerank: negative topk");
    if (topk && (!ou || !os)) return c->fail(PF_EINVAL, "diverse rerank: null output with topk > 0");
    if (!lambda_ok(lambda)) return c->fail(PF_EINVAL, "diverse rerank: lambda outside [0, 1]");
    pf::FieldSel sel;
    if (pf::make_select(c, select, sel) != PF_OK) return c->fail(PF_EINVAL, "diverse rerank: unknown bits in fixed / flags");
    // the pool: the known uids in the caller's order, the first occurrence of each
    std::vector<int32_t> idx, pu;
    std::vector<float> pr;
    std::unordered_set<int32_t> seen;
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(score[i])) return c->fail(PF_EINVAL, "diverse rerank: a NaN or infinite relevance");  // 0 * inf: a NaN value
        const int32_t x = c->hc.idx_of(uid[i]);
        if (x < 0 || !seen.insert(x).second) continue;
        idx.push_back(x);
        pu.push_back(uid[i]);
        pr.push_back(score[i]);
    }
    const size_t M = idx.size();
    if (M > (size_t)PF_DIVERSE_MAX_POOL) return c->fail(PF_EUNSUPP, "diverse rerank: more than PF_DIVERSE_MAX_POOL known, distinct entries");
    if (topk == 0 || M == 0) return PF_OK;
    (void)hipSetDevice(c->device);
    int rc = pool_matrix(c, idx, sel);
    if (rc != PF_OK) return rc;
    pf::DBuf& pool = c->diverse_ws.pool;
    if (!grow(pool, 2 * (size_t)PF_DIVERSE_MAX_POOL * 4)) return c->fail(PF_ENOMEM, "diverse rerank: no device memory for the pool");
    int32_t* d_uid = pool.as<int32_t>();
    float* d_rel = reinterpret_cast<float*>(d_uid + PF_DIVERSE_MAX_POOL);
    // pageable sources: both copies have left pu / pr when the calls return
    HIPCHK(c, hipMemcpyAsync(d_uid, pu.data(), M * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_rel, pr.data(), M * sizeof(float), hipMemcpyHostToDevice, c->stream));
    pf::DiverseIn in{};
    in.uid = d_uid;
    in.rel = d_rel;
    in.m = (int32_t)M;
    in.sim = c->diverse_ws.sim.as<float>();
    in.stride = (int64_t)M;
    in.lambda = lambda;
    in.topk = topk;
    return run_stage(c, in, ou, os, open_, oval, oc);
}

int pf_recommend_diverse_interest(pf_ctx* c, int32_t uid, const pf_diverse_query* q, int32_t topk, int32_t* ou, float* os,
                                  float* open_, double* oval, int32_t* oc, pf_diverse_info* info) {
    const int rc = diverse_args(c, q, topk, ou, os, oc);
    if (rc != PF_OK) return rc;
    return diverse_scan(c, q, topk, [&](pf::SyncScan& S) {
        int32_t u = 0, n = 0;
        float s = 0.f;
        return pf::recommend_uids(c, S, &uid, 1, 1, &u, &s, &n);
    }, ou, os, open_, oval, oc, info);
}

int pf_recommend_diverse_profile(pf_ctx* c, const pf_query_profile* p, const pf_diverse_query* q, int32_t topk, int32_t* ou,
                                 float* os, float* open_, double* oval, int32_t* oc, pf_diverse_info* info) {
    const int rc = diverse_args(c, q, topk, ou, os, oc);
    if (rc != PF_OK) return rc;
    if (!p) return c->fail(PF_EINVAL, "diverse top-k: null profile");
    return diverse_scan(c, q, topk, [&](pf::SyncScan& S) {
        int32_t u = 0, n = 0;
        float s = 0.f;
        std::vector<pf::ProfileOwned> ps;
        const int prc = pf::resolve_profiles(c, p, 1, ps);
        return prc != PF_OK ? prc : pf::recommend_profiles(c, S, ps, 1, &u, &s, &n);
    }, ou, os, open_, oval, oc, info);
}

int pf_recommend_diverse_group(pf_ctx* c, const pf_group_query* g, const pf_diverse_query* q, int32_t topk, int32_t* ou,
                               float* os, float* open_, double* oval, int32_t* oc, pf_diverse_info* info) {
    int rc = diverse_args(c, q, topk, ou, os, oc);
    if (rc != PF_OK) return rc;
    if (!g) return c->fail(PF_EINVAL, "diverse top-k: null group");
    if ((rc = pf::group_args(c, g)) != PF_OK) return rc;
    return diverse_scan(c, q, topk, [&](pf::SyncScan& S) {
        int32_t u = 0, n = 0;
        float s = 0.f;
        return pf::recommend_groups(c, S, g, 1, 1, &u, &s, &n);
    }, ou, os, open_, oval, oc, info);
}

}  // extern "C"
