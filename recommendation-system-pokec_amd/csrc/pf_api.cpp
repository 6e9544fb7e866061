// pf_api.cpp — the C ABI (include/pokec_fas.h): context lifetime and device upload, the setters
// with their validation, argument checks, and the entry points over the host orchestration of the
// reference's recommenders (recommender_graph.cpp:10-237, recommender_clubs.cpp:10-73): the scans
// in pf_scan_host.cpp, the pairs in pf_pairs_host.cpp, the job pipeline in pf_jobs_plan.cpp (the
// group and clubs entry points: pf_group_api.cpp, pf_clubs_api.cpp).  The FAS arithmetic itself runs
// only on the GPU; there is no CPU path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "pf_batch.h"
#include "pf_ctx.h"
#include "pf_debug.h"
#include "pf_host.h"
#include "pf_kernels.h"
#include "pf_store.h"
#include "pokec_fas.h"

namespace {

thread_local std::string g_open_error;

}  // namespace

namespace pf {

void set_open_error(const std::string& m) { g_open_error = m; }

const std::unordered_map<int32_t, std::vector<int32_t>>& base_adj(const pf_ctx* c) { return c->hc.adj; }

void emit(const std::vector<std::pair<int32_t, float>>& r, int i, int topk, int32_t* ou, float* os, int32_t* oc) {
    const int n = std::min<int>((int)r.size(), topk);
    for (int k = 0; k < n; ++k) {
        ou[(int64_t)i * topk + k] = r[k].first;
        os[(int64_t)i * topk + k] = r[k].second;
    }
    oc[i] = n;
}

HostProf::HostProf() {
    on = debug_long("host_prof", 0) != 0;
    for (auto& x : ns) x = 0;
}
HostProf::~HostProf() {
    if (!on) return;
    static const char* nm[kHpStages] = {"workspaces", "prep", "layout", "staging", "wait", "decode", "launch-b",
                                        "launch-a", "finish", "scan-image", "scan-launch", "scan-calls(n)", "scan-stage-wait"};
    fprintf(stderr, "pokec_fas host stages (s):");
    for (int i = 0; i < kHpStages; ++i) fprintf(stderr, " %s=%.3f", nm[i], (double)ns[i].load() * 1e-9);
    fprintf(stderr, "\n");
}
HostProf& host_prof() {
    static HostProf h;
    return h;
}

// The device form of a public selection: PF_EINVAL for unknown bits; NULL, or one that leaves out
// nothing of this engine's T columns, is no selection (on == 0).
int make_select(const pf_ctx* c, const pf_field_select* s, pf::FieldSel& d) {
    d = pf::FieldSel{};
    if (!s) return PF_OK;
    if ((s->fixed & ~pf::kSelFixedAll) || s->flags != 0u) return PF_EINVAL;
    if (pf::select_is_all(s->fixed, s->cols, c->hc.T)) return PF_OK;
    d.fixed = s->fixed;
    d.on = 1u;
    d.cols = s->cols & pf::select_low(c->hc.T);
    return PF_OK;
}

// a caller's window as a call's options take it (null or fields == 0: none), or PF_EINVAL with the reason
int make_window(pf_ctx* c, const pf_scan_window* w, pf_scan_window& d) {
    d = pf_scan_window{};
    if (!w || w->fields == 0u) return PF_OK;
    if ((w->fields & ~pf::kWinAllFields) || w->flags != 0u) return c->fail(PF_EINVAL, "scan window: unknown bits in fields / flags");
    if ((w->fields & PF_WIN_MIN) && std::isnan(w->min_score)) return c->fail(PF_EINVAL, "scan window: min_score is NaN");
    if ((w->fields & PF_WIN_AFTER) && std::isnan(w->after_score)) return c->fail(PF_EINVAL, "scan window: after_score is NaN");
    d = *w;
    return PF_OK;
}

}  // namespace pf

namespace {

// PF_DEBUG host_prof=1: pf_open stage clocks on stderr
struct OpenClock {
    const bool prof = pf::host_prof().on;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        const auto t1 = std::chrono::steady_clock::now();
        if (prof) fprintf(stderr, "[pf_open] %s %.3f s\n", what, std::chrono::duration<double>(t1 - t0).count());
        t0 = t1;
    }
};

// pf_open's stages, in the order they run; a failing one leaves its reason in c->err
int open_device(pf_ctx* c, int device) {
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { c->err = "hipSetDevice failed"; return PF_ENODEV; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        c->num_cus = prop.multiProcessorCount;
        if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
            c->err = std::string("device is ") + prop.gcnArchName + ", the kernels are built for gfx950";
            return PF_ENODEV;
        }
    }
    return PF_OK;
}

int open_host_builds(pf_ctx* c, const pf_corpus_desc* desc, OpenClock& stage) {
    int rc = pf::build_host_corpus(desc, c->hc, c->err);
    if (rc != PF_OK) return rc;
    stage("host corpus (sorted rows, idf, norms)");
    rc = pf::build_store(c->hc, c->hs, c->err);
    if (rc != PF_OK) return rc;
    stage("tile store");
    pf::build_postings(c->hc, c->hp);  // hp.ok = false: the stream scan serves every query
    stage("postings store");
    // PF_DEBUG scan=stream|postings sets the context's initial scan kernel (tests force variants
    // per process with it); pf_set_scan_kernel changes it later
    if (const char* sk = pf::debug_str("scan")) {
        if (!strcmp(sk, "stream")) c->scan_kind = PF_SCAN_STREAM;
        else if (!strcmp(sk, "postings") && c->hp.ok) c->scan_kind = PF_SCAN_POSTINGS;
    }
    return PF_OK;
}

int open_streams(pf_ctx* c) {
    // the job pipeline's two aux streams are created here with the context's own, so the three
    // take consecutive hardware queues whatever streams the host process creates later (created
    // at the first job call, after a torch stream pool, they ran the cfg-3 sub-record of the
    // default bench line at 0.466 vs 0.415 ms per step, r5l)
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->jb.aux, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->jb.aux2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        c->err = "stream/event creation failed";
        return PF_ENODEV;
    }
    for (int l = 3; l < pf::scan_lanes(); ++l)  // lanes past the context's and the aux streams
        if (hipStreamCreateWithFlags(&c->lane_st[l], hipStreamNonBlocking) != hipSuccess) {
            c->err = "stream creation failed";
            return PF_ENODEV;
        }
    return PF_OK;
}

int upload_stores(pf_ctx* c) {
    auto& hs = c->hs;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = upload(c, c->d_stream, hs.stream);
    if (e == hipSuccess) e = upload(c, c->d_tile_off, hs.tile_off);
    if (e == hipSuccess) e = upload(c, c->d_tile_steps, hs.tile_steps);
    if (e == hipSuccess) e = upload(c, c->d_tile_slot0, hs.tile_slot0);
    if (e == hipSuccess) e = upload(c, c->d_tile_lgk, hs.tile_lgk);
    if (e == hipSuccess) e = upload(c, c->d_slot_tile, hs.slot_tile);
    if (e == hipSuccess) e = upload(c, c->d_norms, hs.norms);
    if (e == hipSuccess) e = upload(c, c->d_norm_off, hs.norm_off);
    if (e == hipSuccess) e = upload(c, c->d_hdr0, hs.hdr0);
    if (e == hipSuccess) e = upload(c, c->d_hdr1, hs.hdr1);
    if (e == hipSuccess) e = upload(c, c->d_hdr2, hs.hdr2);
    if (e == hipSuccess) e = upload(c, c->d_rowstore, hs.rows);
    if (e == hipSuccess) e = upload(c, c->d_rowstore_off, hs.row_off);
    if (c->hp.ok) {
        auto& hp = c->hp;
        if (e == hipSuccess) e = upload(c, c->d_phdr, hp.hdr);
        if (e == hipSuccess) e = upload(c, c->d_post, hp.post);
        if (e == hipSuccess) e = upload(c, c->d_pnorm, hp.pnorm);
        if (e == hipSuccess) e = upload(c, c->d_cells, hp.cells);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) return PF_OK;
    c->hip_fail(e, "corpus upload");
    return e == hipErrorOutOfMemory ? PF_ENOMEM : PF_ENODEV;
}

// the device views of the stores (c->ds, c->ps), the byte figures and the whole-corpus shard
void bind_stores(pf_ctx* c) {
    auto& hs = c->hs;
    c->stream_bytes = (int64_t)hs.stream.size() * 16;
    c->norm_bytes = (int64_t)hs.norms.size() * 8;
    c->ds.row_pad = c->d_rowstore.as<uint4>() + hs.row_off[c->hc.n];  // build_store's trailing padding line
    c->ds.stream = c->d_stream.as<uint4>();
    c->ds.tile_off = c->d_tile_off.as<uint64_t>();
    c->ds.tile_steps = c->d_tile_steps.as<uint32_t>();
    c->ds.tile_slot0 = c->d_tile_slot0.as<uint32_t>();
    c->ds.tile_lgk = c->d_tile_lgk.as<uint8_t>();
    c->ds.slot_tile = c->d_slot_tile.as<uint32_t>();
    c->ds.norms = c->d_norms.as<double>();
    c->ds.norm_off = c->d_norm_off.as<uint64_t>();
    c->ds.hdr0 = c->d_hdr0.as<uint4>();
    c->ds.hdr1 = c->d_hdr1.as<uint4>();
    c->ds.hdr2 = c->d_hdr2.as<uint4>();
    c->ds.rows = c->d_rowstore.as<uint4>();
    c->ds.row_off = c->d_rowstore_off.as<uint64_t>();
    c->ds.n_slots = c->hc.n;
    c->ds.n_tiles = (int32_t)hs.tile_steps.size();
    c->ds.packed = hs.packed ? 1 : 0;
    c->ds.n_cols = c->hc.T;
    c->tile_begin = 0;
    c->tile_end = c->ds.n_tiles;
    if (!c->hp.ok) return;
    auto& hp = c->hp;
    c->post_bytes = (int64_t)hp.hdr.size() * 16 + (int64_t)hp.post.size() * 4 + (int64_t)hp.pnorm.size() * 8 +
                    (int64_t)hp.cells.size() * 4;
    c->ps.n_post = (uint32_t)hp.post.size();
    c->ps.n_tok_entries = (uint32_t)hp.pnorm.size();
    c->ps.n_cells = (uint32_t)hp.cells.size();
    c->ps.hdr = c->d_phdr.as<uint4>();
    c->ps.post = c->d_post.as<uint32_t>();
    c->ps.pnorm = c->d_pnorm.as<double>();
    c->ps.cells = c->d_cells.as<uint32_t>();
    c->ps.n = c->hc.n;
    // block size: the LDS capacity.  Sizing blocks to fill whole waves of resident
    // workgroups (798 at 1.6M) measured slower (258 vs 244 us): per-block costs dominate
    // the half-empty last wave.  PF_DEBUG k5_block overrides it (tests).
    const int64_t b = pf::debug_long("k5_block", pf::kBlockCands);
    c->ps.bsize = (int32_t)std::max<int64_t>(64, std::min<int64_t>(pf::kBlockCands, b));
    c->ps.n_blocks = (c->hc.n + c->ps.bsize - 1) / c->ps.bsize;
    c->wb_begin = 0;
    c->wb_end = c->ps.n_blocks;
}

// The host copies of the device stores (~5 GB at 1.63M users) are returned to the system on a
// detached thread: unmapping them takes ~0.6 s that pf_open need not wait for.  hp.cells stays on
// the host: pf_scan_bytes reads the lists' cell ranges.
void release_host_stores(pf_ctx* c) {
    auto& hs = c->hs;
    try {
        std::thread([a = std::move(hs.stream), b = std::move(hs.norms), r = std::move(hs.rows),
                     p = std::move(c->hp.post), q = std::move(c->hp.pnorm)]() mutable {}).detach();
    } catch (...) {  // no thread to be had: free them here (no exception crosses the C ABI)
        hs.stream.clear(); hs.norms.clear(); hs.rows.clear(); c->hp.post.clear(); c->hp.pnorm.clear();
    }
    std::vector<uint64_t>().swap(hs.row_off);
    std::vector<uint4>().swap(c->hp.hdr);
}

pf::AdjView plain_view(const pf_ctx* c) {
    pf::AdjView v;
    v.base = &c->hc.adj;
    return v;
}

// nq calls of one recommender, one per uid of q, under the engine's own adjacency
std::vector<pf::Job> make_jobs(const pf_ctx* c, int kind, const int32_t* q, int32_t nq, int32_t topk, int32_t limit,
                               bool all_candidates) {
    std::vector<pf::Job> jobs((size_t)nq);
    for (int32_t i = 0; i < nq; ++i) {
        jobs[i].kind = kind;
        jobs[i].uid = q[i];
        jobs[i].topk = topk;
        jobs[i].limit = limit;
        jobs[i].all_candidates = all_candidates;
        jobs[i].view = plain_view(c);
    }
    return jobs;
}

int emit_jobs(pf_ctx* c, std::vector<pf::Job> jobs, int topk, int32_t* ou, float* os, int32_t* oc) {
    for (size_t i = 0; i < jobs.size(); ++i) oc[i] = 0;
    if (topk == 0 || jobs.empty()) return PF_OK;
    const int rc = pf::run_jobs(c, jobs);
    if (rc != PF_OK) return rc;
    for (size_t i = 0; i < jobs.size(); ++i) pf::emit(jobs[i].out, (int)i, topk, ou, os, oc);
    return PF_OK;
}

// FAS of the pairs (a[i], b[i]) (a == nullptr: of the profile pv with every b[i]); an unknown uid's is NaN
int scored_pairs(pf_ctx* c, const int32_t* a, const int32_t* b, int64_t n, float* out, const pf::FieldSel& sel,
                 const pf::ProfileView* pv) {
    pf::PairGroups pg(true);  // one float per pair: where[i] = (group, position), no per-group destinations
    pf::group_pairs(c, a, b, 0, n, pg);
    for (int64_t i = 0; i < n; ++i) out[i] = NAN;
    std::vector<std::vector<float>> res;
    const int rc = pf::run_pairs(c, pg.qidx, pg.slots, res, nullptr, nullptr, sel, pv);
    if (rc != PF_OK) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (pg.where[(size_t)i].first >= 0) out[i] = res[pg.where[(size_t)i].first][pg.where[(size_t)i].second];
    return PF_OK;
}

// an unknown uid's breakdown: NaN, nothing present, the row all 0.0 (W doubles)
void blank_terms(pf_pair_terms_head* head, double* terms, int64_t n, size_t W) {
    for (int64_t i = 0; i < n; ++i) head[i] = pf_pair_terms_head{NAN, 0u, 0ull};
    std::fill(terms, terms + (size_t)n * W, 0.0);
}

}  // namespace

extern "C" {

int pf_abi_version(void) { return PF_ABI_VERSION; }

int pf_open(const pf_corpus_desc* desc, int device, pf_ctx** out) {
    if (!out) { g_open_error = "null out"; return PF_EINVAL; }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_open_error = "no HIP device (the FAS engine has no CPU fallback)";
        return PF_ENODEV;
    }
    if (device < 0 || device >= ndev) { g_open_error = "bad device ordinal"; return PF_EINVAL; }
    pf_ctx* c = new pf_ctx();
    auto bail = [&](int rc) {
        g_open_error = c->err;
        delete c;
        return rc;
    };
    int rc = open_device(c, device);
    if (rc != PF_OK) return bail(rc);
    OpenClock stage;
    if ((rc = open_host_builds(c, desc, stage)) != PF_OK) return bail(rc);
    if ((rc = open_streams(c)) != PF_OK) return bail(rc);
    rc = upload_stores(c);
    stage("upload");
    if (rc != PF_OK) return bail(rc);
    bind_stores(c);
    release_host_stores(c);
    rc = pf::jobs_open(c);  // device graph + image-builder tables (the recommenders' pipeline)
    if (rc != PF_OK) return bail(rc);
    stage("job pipeline (graph, image tables)");
    rc = pf::build_resident_post(c);  // every user's K5 image part (the one-query scans' resident images)
    if (rc != PF_OK) return bail(rc);
    stage(c->rp.on ? ("resident postings images, " + std::to_string(c->rp.d_pool.cap >> 20) + " MiB").c_str()
                   : "resident postings images (off)");
    *out = c;
    return PF_OK;
}

void pf_close(pf_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    c->jb.pending.clear();  // calls never waited for: their outputs are not written
    c->jb.carry = pf::JobsState::Carry{};
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->jb.aux2) (void)hipStreamSynchronize(c->jb.aux2);
    for (auto& e : c->prof_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& ln : c->lane) {  // (their streams are the context's, the aux streams and lane_st)
        if (ln.st) (void)hipStreamSynchronize(ln.st);
        if (ln.done) (void)hipEventDestroy(ln.done);
        for (hipEvent_t e : ln.freed)
            if (e) (void)hipEventDestroy(e);
    }
    for (hipStream_t st : c->lane_st)
        if (st) (void)hipStreamDestroy(st);
    for (auto& st : c->stage) {
        if (st.done) (void)hipEventDestroy(st.done);
        if (st.p) (void)hipHostFree(st.p);
    }
    if (c->jb.aux) {
        (void)hipStreamSynchronize(c->jb.aux);
        (void)hipStreamDestroy(c->jb.aux);
    }
    if (c->jb.aux2) {
        (void)hipStreamSynchronize(c->jb.aux2);
        (void)hipStreamDestroy(c->jb.aux2);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* pf_last_error(const pf_ctx* c) { return c ? c->err.c_str() : g_open_error.c_str(); }
int32_t pf_num_users(const pf_ctx* c) { return c ? c->hc.n : 0; }
float pf_idf(const pf_ctx* c, int32_t col, int32_t tid) {
    if (!c || col < 0 || col >= c->hc.T) return NAN;
    return c->hc.idf_of_tid(col, tid);
}

static_assert(PF_SEL_FIXED_ALL == pf::kSelFixedAll && (1u << PF_F_PUBLIC) == pf::kSelPublic &&
                  (1u << PF_F_GENDER) == pf::kSelGender && (1u << PF_F_COMPLETION) == pf::kSelCompletion &&
                  (1u << PF_F_AGE) == pf::kSelAge && (1u << PF_F_REGION) == pf::kSelRegion &&
                  (1u << PF_F_CLUBS) == pf::kSelClubs && (1u << PF_F_FRIENDS) == pf::kSelFriends,
              "pf_select.h restates the public field bits");
static_assert(sizeof(pf_field_select) == 16 && sizeof(pf_field_select) == sizeof(pf::FieldSel), "pf_field_select is 16 B");

int pf_set_scan_select(pf_ctx* c, const pf_field_select* s) {
    if (!c) return PF_EINVAL;
    pf::FieldSel d;
    if (pf::make_select(c, s, d) != PF_OK) return c->fail(PF_EINVAL, "scan select: unknown bits in fixed / flags");
    c->sel = d;
    return PF_OK;
}

int pf_fas_pairs(pf_ctx* c, const int32_t* a, const int32_t* b, int64_t n, float* out) {
    if (!c || n < 0 || (n && (!a || !b || !out))) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    return scored_pairs(c, a, b, n, out, pf::FieldSel{}, nullptr);
}

int pf_fas_pairs_select(pf_ctx* c, const int32_t* a, const int32_t* b, int64_t n, const pf_field_select* s, float* out) {
    if (!c || n < 0 || (n && (!a || !b || !out))) return PF_EINVAL;
    pf::FieldSel d;
    if (pf::make_select(c, s, d) != PF_OK) return c->fail(PF_EINVAL, "pairs select: unknown bits in fixed / flags");
    (void)hipSetDevice(c->device);
    return scored_pairs(c, a, b, n, out, d, nullptr);
}

static_assert(sizeof(pf_pair_terms_head) == 16, "pf_pair_terms_head is 16 B");

int32_t pf_num_cols(const pf_ctx* c) { return c ? c->hc.T : 0; }

int pf_fas_pairs_terms(pf_ctx* c, const int32_t* a, const int32_t* b, int64_t n, const pf_field_select* s,
                       pf_pair_terms_head* head, double* terms) {
    if (!c || n < 0 || (n && (!a || !b || !head || !terms))) return PF_EINVAL;
    pf::FieldSel d;
    if (pf::make_select(c, s, d) != PF_OK) return c->fail(PF_EINVAL, "pairs terms: unknown bits in fixed / flags");
    (void)hipSetDevice(c->device);
    const size_t W = (size_t)(PF_NUM_FIXED + c->hc.T);
    pf::PairGroups tg;
    pf::group_pairs(c, a, b, 0, n, tg, [&](int64_t i) { blank_terms(head + i, terms + (size_t)i * W, 1, W); });
    return pf::run_pair_terms(c, tg.qidx, tg.slots, tg.dest, head, terms, d);
}

int pf_recommend_interest_all_terms(pf_ctx* c, const int32_t* q, int32_t nq, int32_t topk, int32_t* ou, float* os,
                                    int32_t* oc, pf_pair_terms_head* head, double* terms) {
    if (!c || nq < 0 || topk < 0 || (nq && (!q || !oc)) || (nq && topk && (!ou || !os || !head || !terms))) return PF_EINVAL;
    // the scan itself, whatever path it takes; its ids and scores are the caller's results as they are
    const int rc = pf_recommend_interest(c, q, nq, topk, PF_MODE_ALL, 0, ou, os, oc);
    if (rc != PF_OK) return rc;
    // the (query, winner) pairs, formed on the host from the list the scan returned
    pf::PairGroups tg;
    for (int32_t i = 0; i < nq; ++i) {
        if (oc[i] <= 0) continue;
        const int32_t ia = c->hc.idx_of(q[i]);
        for (int32_t j = 0; j < oc[i]; ++j) {
            const int32_t ib = c->hc.idx_of(ou[(size_t)i * topk + j]);
            if (ia < 0 || ib < 0) return c->fail(PF_EINTERNAL, "scan result without a profile");
            tg.add(ia, c->hs.slot_of_idx[ib], (int64_t)i * topk + j);
        }
    }
    return pf::run_pair_terms(c, tg.qidx, tg.slots, tg.dest, head, terms, c->sel);
}

static int profile_args(pf_ctx* c, const pf_query_profile* q, int32_t nq, int32_t topk, int32_t* ou, float* os, int32_t* oc) {
    if (!c) return PF_EINVAL;
    if (nq < 0 || topk < 0) return c->fail(PF_EINVAL, "query profile: negative nq / topk");
    if (nq && (!q || !oc || (topk && (!ou || !os)))) return c->fail(PF_EINVAL, "query profile: null argument with nq > 0");
    if (topk > pf::kMaxTopK) return c->fail(PF_EUNSUPP, "query profile: topk above the scan kernels' bound (64)");
    return PF_OK;
}

int pf_recommend_interest_profile(pf_ctx* c, const pf_query_profile* q, int32_t nq, int32_t topk, int32_t* ou, float* os,
                                  int32_t* oc) {
    int rc = profile_args(c, q, nq, topk, ou, os, oc);
    if (rc != PF_OK || nq == 0) return rc;
    (void)hipSetDevice(c->device);
    std::vector<pf::ProfileOwned> ps;
    if ((rc = pf::resolve_profiles(c, q, nq, ps)) != PF_OK) return rc;
    for (int i = 0; i < nq; ++i) oc[i] = 0;
    if (topk == 0) return PF_OK;
    pf::SyncScan S(c);
    return pf::recommend_profiles(c, S, ps, topk, ou, os, oc);
}

int pf_fas_profile_pairs(pf_ctx* c, const pf_query_profile* a, const int32_t* b, int64_t n, const pf_field_select* s,
                         float* out) {
    if (!c) return PF_EINVAL;
    if (n < 0 || !a || (n && (!b || !out))) return c->fail(PF_EINVAL, "profile pairs: null argument");
    pf::FieldSel d;
    if (pf::make_select(c, s, d) != PF_OK) return c->fail(PF_EINVAL, "profile pairs: unknown bits in fixed / flags");
    (void)hipSetDevice(c->device);
    std::vector<pf::ProfileOwned> ps;
    int rc = pf::resolve_profiles(c, a, 1, ps);
    if (rc != PF_OK) return rc;
    return scored_pairs(c, nullptr, b, n, out, d, &ps[0].v);
}

int pf_fas_profile_pairs_terms(pf_ctx* c, const pf_query_profile* a, const int32_t* b, int64_t n, const pf_field_select* s,
                               pf_pair_terms_head* head, double* terms) {
    if (!c) return PF_EINVAL;
    if (n < 0 || !a || (n && (!b || !head || !terms))) return c->fail(PF_EINVAL, "profile pairs terms: null argument");
    pf::FieldSel d;
    if (pf::make_select(c, s, d) != PF_OK) return c->fail(PF_EINVAL, "profile pairs terms: unknown bits in fixed / flags");
    (void)hipSetDevice(c->device);
    std::vector<pf::ProfileOwned> ps;
    const int rc = pf::resolve_profiles(c, a, 1, ps);
    if (rc != PF_OK) return rc;
    const size_t W = (size_t)(PF_NUM_FIXED + c->hc.T);
    pf::PairGroups pg;  // one group: the profile
    pf::group_pairs(c, nullptr, b, 0, n, pg);
    blank_terms(head, terms, n, W);  // an unknown uid keeps this
    return pf::run_pair_terms(c, pg.qidx, pg.slots, pg.dest, head, terms, d, &ps[0].v);
}

int pf_recommend_interest_profile_terms(pf_ctx* c, const pf_query_profile* q, int32_t nq, int32_t topk, int32_t* ou,
                                        float* os, int32_t* oc, pf_pair_terms_head* head, double* terms) {
    int rc = profile_args(c, q, nq, topk, ou, os, oc);
    if (rc != PF_OK || nq == 0) return rc;
    if (topk && (!head || !terms)) return c->fail(PF_EINVAL, "query profile: null argument with nq > 0");
    (void)hipSetDevice(c->device);
    std::vector<pf::ProfileOwned> ps;
    if ((rc = pf::resolve_profiles(c, q, nq, ps)) != PF_OK) return rc;
    for (int i = 0; i < nq; ++i) oc[i] = 0;
    if (topk == 0) return PF_OK;
    pf::SyncScan S(c);
    if ((rc = pf::recommend_profiles(c, S, ps, topk, ou, os, oc)) != PF_OK) return rc;
    // the (profile, winner) pairs, profile by profile: each has an image of its own
    for (int32_t i = 0; i < nq; ++i) {
        if (oc[i] <= 0) continue;
        pf::PairGroups pg;
        for (int32_t j = 0; j < oc[i]; ++j) {
            const int32_t ib = c->hc.idx_of(ou[(size_t)i * topk + j]);
            if (ib < 0) return c->fail(PF_EINTERNAL, "scan result without a profile");
            pg.add(0, c->hs.slot_of_idx[ib], (int64_t)i * topk + j);
        }
        if ((rc = pf::run_pair_terms(c, pg.qidx, pg.slots, pg.dest, head, terms, c->sel, &ps[(size_t)i].v)) != PF_OK) return rc;
    }
    return PF_OK;
}

int pf_recommend_interest(pf_ctx* c, const int32_t* q, int32_t nq, int32_t topk, int32_t mode, int32_t limit,
                          int32_t* ou, float* os, int32_t* oc) {
    if (!c || nq < 0 || topk < 0 || (nq && (!q || !oc))) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    for (int i = 0; i < nq; ++i) oc[i] = 0;
    if (topk == 0 || nq == 0) return PF_OK;
    if (mode == PF_MODE_ALL && topk <= pf::kMaxTopK) {
        pf::SyncScan S(c);
        return pf::recommend_uids(c, S, q, nq, topk, ou, os, oc);
    }
    if (mode == PF_MODE_ALL && c->coll_cap > 0)
        return c->fail(PF_EUNSUPP, "scan collect: topk above 64 runs in the job pipeline, which reads no collector");
    if (mode == PF_MODE_ALL && c->win.fields != 0u)
        return c->fail(PF_EUNSUPP, "scan window: topk above 64 runs in the job pipeline, which reads no window "
                                   "(page with the cursor instead)");
    // FoF-limited (reference) mode, or ALL with topk beyond the in-kernel bound
    return emit_jobs(c, make_jobs(c, pf::kJobInterest, q, nq, topk, limit, mode == PF_MODE_ALL), topk, ou, os, oc);
}

// recommender_graph.cpp:105-222
int pf_recommend_collab(pf_ctx* c, const int32_t* q, int32_t nq, int32_t topk, int32_t limit, int32_t* ou,
                        float* os, int32_t* oc) {
    if (!c || nq < 0 || topk < 0 || (nq && (!q || !oc))) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    return emit_jobs(c, make_jobs(c, pf::kJobCollab, q, nq, topk, limit, false), topk, ou, os, oc);
}

// recommender_clubs.cpp:10-73
int pf_recommend_clubs(pf_ctx* c, const int32_t* q, int32_t nq, int32_t topk, int32_t limit, int32_t* ou,
                       float* os, int32_t* oc) {
    if (!c || nq < 0 || topk < 0 || (nq && (!q || !oc))) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    return emit_jobs(c, make_jobs(c, pf::kJobClubs, q, nq, topk, limit, false), topk, ou, os, oc);
}

// Asynchronous forms: plan + launch now, outputs written by pf_wait (pokec_fas.h)
static int job_async(pf_ctx* c, int kind, const int32_t* q, int32_t nq, int32_t topk, int32_t limit, int32_t* ou,
                     float* os, int32_t* oc, uint64_t* ticket) {
    if (!c || !ticket || nq < 0 || topk < 0 || (nq && (!q || !oc || (topk && (!ou || !os))))) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    return pf::run_jobs_async(c, make_jobs(c, kind, q, nq, topk, limit, false), topk, ou, os, oc, ticket);
}

int pf_recommend_interest_async(pf_ctx* c, const int32_t* q, int32_t nq, int32_t topk, int32_t limit, int32_t* ou,
                                float* os, int32_t* oc, uint64_t* ticket) {
    return job_async(c, pf::kJobInterest, q, nq, topk, limit, ou, os, oc, ticket);
}
int pf_recommend_collab_async(pf_ctx* c, const int32_t* q, int32_t nq, int32_t topk, int32_t limit, int32_t* ou,
                              float* os, int32_t* oc, uint64_t* ticket) {
    return job_async(c, pf::kJobCollab, q, nq, topk, limit, ou, os, oc, ticket);
}
int pf_recommend_clubs_async(pf_ctx* c, const int32_t* q, int32_t nq, int32_t topk, int32_t limit, int32_t* ou,
                             float* os, int32_t* oc, uint64_t* ticket) {
    return job_async(c, pf::kJobClubs, q, nq, topk, limit, ou, os, oc, ticket);
}
int pf_wait(pf_ctx* c, uint64_t ticket) {
    if (!c) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    return pf::jobs_wait(c, ticket);
}

uint64_t pf_completed_ticket(const pf_ctx* c) {
    if (!c) return 0;
    // tickets are handed out in launch order and completed in launch order
    uint64_t t = c->jb.pending.empty() ? c->jb.next_ticket - 1 : c->jb.pending.front().ticket - 1;
    if (c->jb.carry.on) t = std::min(t, c->jb.carry.ticket - 1);
    return t;
}

int pf_fof_candidates(pf_ctx* c, int32_t uid, int32_t limit, int32_t flavour, int32_t* out, int32_t cap, int32_t* n) {
    if (!c || !n || (cap > 0 && !out)) return PF_EINVAL;
    if (flavour != PF_FOF_GRAPH && flavour != PF_FOF_COLLAB) return PF_EINVAL;
    std::vector<int32_t> v;  // K3 on the device (pf_jobs.hip gather_kernel)
    const int rc = pf::fof_device(c, uid, limit, flavour, v);
    if (rc != PF_OK) return rc;
    for (int32_t i = 0; i < (int32_t)v.size() && i < cap; ++i) out[i] = v[i];
    *n = (int32_t)v.size();
    return PF_OK;
}

int pf_set_adj(pf_ctx* c, int32_t uid, const int32_t* nbrs, int32_t n) {
    if (!c || (n > 0 && !nbrs)) return PF_EINVAL;
    const int rc = pf::jobs_set_adj(c, uid, nbrs, n);
    // the user's exclusions (adj_list row + self) changed: its resident K5 image is stale for good
    if (rc == PF_OK && c->rp.on) {
        const int32_t x = c->hc.idx_of(uid);
        if (x >= 0) c->rp.stale[(size_t)x] = 1;
    }
    return rc;
}

int pf_set_shard(pf_ctx* c, int32_t shard, int32_t nshards) {
    if (!c || nshards < 1 || shard < 0 || shard >= nshards) return PF_EINVAL;
    const auto& steps = c->hs.tile_steps;
    const int T = (int)steps.size();
    std::vector<uint64_t> pre(T + 1, 0);
    for (int t = 0; t < T; ++t) pre[t + 1] = pre[t] + steps[t];
    auto bound = [&](int s) -> int {
        if (s <= 0) return 0;
        if (s >= nshards) return T;
        uint64_t target = pre[T] * (uint64_t)s / (uint64_t)nshards;
        return (int)(std::lower_bound(pre.begin(), pre.end(), target) - pre.begin());
    };
    c->tile_begin = bound(shard);
    c->tile_end = bound(shard + 1);
    c->n_shards = nshards;
    // postings scan: contiguous block ranges of equal posting weight.  A block's cost is a
    // fixed part (headers, ranges, top-k: ~60 of ~210 us at cfg 2) plus
    // its share of the lists a query names, i.e. of the postings entries (tokens, clubs,
    // friends) its candidates hold: weight = kBlockFixedWords * candidates + entries.
    const int64_t nwb = c->ps.n_blocks;
    if (nwb > 0) {
        const auto& hc = c->hc;
        const int64_t bs = c->ps.bsize;
        constexpr int64_t kBlockFixedWords = 64;
        std::vector<uint64_t> wpre(nwb + 1, 0);
        for (int64_t b = 0; b < nwb; ++b) {
            const int64_t i0 = b * bs, i1 = std::min<int64_t>(hc.n, i0 + bs);
            wpre[b + 1] = wpre[b] + (uint64_t)(kBlockFixedWords * (i1 - i0) + pf::block_range_entries(hc, i0, i1));
        }
        auto wbound = [&](int s) -> int32_t {
            if (s <= 0) return 0;
            if (s >= nshards) return (int32_t)nwb;
            const uint64_t target = wpre[nwb] * (uint64_t)s / (uint64_t)nshards;
            return (int32_t)(std::lower_bound(wpre.begin(), wpre.end(), target) - wpre.begin());
        };
        c->wb_begin = wbound(shard);
        c->wb_end = wbound(shard + 1);
    }
    return PF_OK;
}

int pf_set_scan_kernel(pf_ctx* c, int32_t kind) {
    if (!c || kind < PF_SCAN_AUTO || kind > PF_SCAN_POSTINGS) return PF_EINVAL;
    if (kind == PF_SCAN_POSTINGS && !c->hp.ok) return c->fail(PF_EUNSUPP, "postings store unavailable: " + c->hp.why);
    c->scan_kind = kind;
    return PF_OK;
}

static_assert(PF_FILT_GENDER == pf::kFiltGender && PF_FILT_PUBLIC == pf::kFiltPublic && PF_FILT_AGE == pf::kFiltAge &&
                  PF_FILT_COMPLETION == pf::kFiltCompletion && PF_FILT_REGION == pf::kFiltRegion &&
                  PF_FILT_KEEP_MISSING == pf::kFiltKeepMissing,
              "pf_filter.h restates the public filter bits");
static_assert(sizeof(pf_cand_filter) == 48, "pf_cand_filter is 48 B");

int pf_set_scan_filter(pf_ctx* c, const pf_cand_filter* f) {
    if (!c) return PF_EINVAL;
    if (!f || f->fields == 0u) {
        c->filt = pf::CandFilter{};
        return PF_OK;
    }
    if ((f->fields & ~pf::kFiltAllFields) || (f->flags & ~pf::kFiltKeepMissing)) return c->fail(PF_EINVAL, "scan filter: unknown bits");
    if ((f->fields & PF_FILT_AGE) && f->age_min > f->age_max) return c->fail(PF_EINVAL, "scan filter: age_min > age_max");
    if ((f->fields & PF_FILT_COMPLETION) && f->completion_min > f->completion_max)
        return c->fail(PF_EINVAL, "scan filter: completion_min > completion_max");
    if ((f->fields & PF_FILT_REGION) && f->region[0] < 0 && f->region[1] < 0 && f->region[2] < 0)
        return c->fail(PF_EINVAL, "scan filter: PF_FILT_REGION with no part given");
    // the headers store public / gender as equality codes: the filter's values are translated once
    // here; a value no user has gets a code no header holds (and so does a negative one: a missing
    // field passes through PF_FILT_KEEP_MISSING only)
    auto code = [](const std::unordered_map<int32_t, uint32_t>& m, int32_t v) -> uint32_t {
        auto it = v < 0 ? m.end() : m.find(v);
        return it == m.end() ? pf::kFiltCodeNobody : it->second;
    };
    pf::CandFilter d{};
    d.fields = f->fields;
    d.flags = f->flags;
    d.pub = (f->fields & PF_FILT_PUBLIC) ? code(c->hc.pub_code, f->public_flag) : 0u;
    d.gen = (f->fields & PF_FILT_GENDER) ? code(c->hc.gen_code, f->gender) : 0u;
    d.age_min = f->age_min;
    d.age_max = f->age_max;
    d.comp_min = f->completion_min;
    d.comp_max = f->completion_max;
    for (int i = 0; i < 3; ++i) d.reg[i] = (f->fields & PF_FILT_REGION) ? f->region[i] : -1;
    c->filt = d;
    return PF_OK;
}

int pf_scan_filter_count(pf_ctx* c, int64_t* n) {
    if (!c || !n) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    // this shard's candidates, as the kernel the next scan uses sees them: K5's blocks in idx order
    // (postings headers), else K1's tiles in slot order (tile headers)
    pf::PostStore ps = c->ps;
    int64_t i0, i1;
    if (c->use_post()) {
        i0 = std::min<int64_t>((int64_t)c->wb_begin * c->ps.bsize, c->ps.n);
        i1 = std::min<int64_t>((int64_t)c->wb_end * c->ps.bsize, c->ps.n);
    } else {
        ps.hdr = nullptr;
        const auto& s0 = c->hs.tile_slot0;
        auto slot = [&](int32_t t) -> int64_t { return t < (int32_t)s0.size() ? (int64_t)s0[(size_t)t] : (int64_t)c->ds.n_slots; };
        i0 = slot(c->tile_begin);
        i1 = slot(c->tile_end);
    }
    if (c->filt.fields == 0u) {  // no filter: everybody
        *n = std::max<int64_t>(0, i1 - i0);
        return PF_OK;
    }
    HIPCHK(c, c->d_filt_count.ensure(sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->d_filt_count.p, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, pf::launch_filter_count(ps, c->ds, (int32_t)i0, (int32_t)i1, c->filt, c->d_filt_count.as<unsigned long long>(),
                                      c->stream));
    unsigned long long v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, c->d_filt_count.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n = (int64_t)v;
    return PF_OK;
}

static_assert(PF_WIN_MIN == pf::kWinMin && PF_WIN_AFTER == pf::kWinAfter && PF_WIN_COUNT == pf::kWinCount,
              "pf_window.h restates the public window bits");
static_assert(sizeof(pf_scan_window) == 24, "pf_scan_window is 24 B");

int pf_set_scan_window(pf_ctx* c, const pf_scan_window* w) {
    if (!c) return PF_EINVAL;
    pf_scan_window d;
    const int rc = pf::make_window(c, w, d);
    if (rc != PF_OK) return rc;
    c->win_pub = d;
    c->win = pf::window_make(d.fields, d.min_score, d.after_score, d.after_uid);
    return PF_OK;
}

int pf_scan_window_totals(pf_ctx* c, int64_t* out, int32_t cap, int32_t* n) {
    if (!c) return PF_EINVAL;
    if (!n || cap < 0 || (cap && !out)) return c->fail(PF_EINVAL, "scan window totals: null argument");
    if (!c->win_totals_set) return c->fail(PF_EINVAL, "scan window totals: no counted call has run");
    *n = (int32_t)c->win_totals.size();
    for (int32_t i = 0; i < std::min(cap, *n); ++i) out[i] = c->win_totals[(size_t)i];
    return PF_OK;
}

int pf_set_scan_collect(pf_ctx* c, int64_t cap) {
    if (!c) return PF_EINVAL;
    if (cap < 0 || cap > (int64_t)INT32_MAX) return c->fail(PF_EINVAL, "scan collect: cap below 0 or above INT32_MAX");
    if (cap > 0) {  // 0: cleared; the buffers stay for the next collector
        (void)hipSetDevice(c->device);
        const int rc = pf::collect_reserve(c, cap);
        if (rc != PF_OK) return rc;
    }
    c->coll_cap = cap;
    return PF_OK;
}

int pf_scan_collected(pf_ctx* c, int32_t* out_uid, float* out_score, int64_t out_cap, int64_t* n, int64_t* total) {
    if (!c) return PF_EINVAL;
    if (!n || !total || out_cap < 0 || (out_cap && (!out_uid || !out_score)))
        return c->fail(PF_EINVAL, "scan collected: null argument");
    if (!c->coll_set) return c->fail(PF_EINVAL, "scan collected: no collecting call has run");
    *total = c->coll_total;
    *n = (int64_t)c->coll_keys.size();
    const int64_t m = std::min<int64_t>(out_cap, *n);
    for (int64_t i = 0; i < m;) {  // pf_decode_keys' arithmetic, a slice at a time (its count is 32-bit)
        const int32_t step = (int32_t)std::min<int64_t>(m - i, 1 << 20);
        int32_t cnt = 0;
        pf_decode_keys(c->coll_keys.data() + i, step, out_uid + i, out_score + i, &cnt);
        i += step;
    }
    return PF_OK;
}

int pf_scan_keys_async(pf_ctx* c, const int32_t* q, int32_t nq, int32_t topk, uint64_t* d_keys, void* stream) {
    if (!c || nq < 0 || topk <= 0 || topk > pf::kMaxTopK || (nq && (!q || !d_keys))) return PF_EINVAL;
    if (c->win.fields & pf::kWinCount)
        return c->fail(PF_EUNSUPP, "scan window: PF_WIN_COUNT with pf_scan_keys_async (a count needs a synchronous call)");
    if (c->coll_cap > 0)
        return c->fail(PF_EUNSUPP, "scan collect: pf_scan_keys_async reads no collector (a collect needs a synchronous call)");
    (void)hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;  // as given: NULL is the null stream
    std::vector<int32_t> idx, rows;
    for (int i = 0; i < nq; ++i) {
        int32_t x = c->hc.idx_of(q[i]);
        if (x >= 0) { idx.push_back(x); rows.push_back(i); }
    }
    if ((int)idx.size() < nq)  // rows of unknown users stay empty
        HIPCHK(c, hipMemsetAsync(d_keys, 0xFF, (size_t)nq * topk * sizeof(uint64_t), s));
    // the call's options from the sticky state as it stands now
    const pf::ScanCall call = pf::make_scan_call(c->filt, c->sel, c->win_pub, c->hc.uid.data(), c->hc.uid.size(), 0, nullptr, nullptr);
    return pf::scan_all(c, call, idx, rows, topk, d_keys, s, true);
}

int pf_merge_keys_async(pf_ctx* c, const uint64_t* d_parts, int32_t nparts, int32_t nq, int32_t topk, uint64_t* d_out,
                        void* stream) {
    if (!c || nparts < 1 || nq < 0 || topk <= 0 || topk > pf::kMaxTopK) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, pf::launch_merge(d_parts, nparts, (int64_t)nq * topk, topk, nq, topk, d_out, s));
    return PF_OK;
}

int pf_jobs_stats_reset(pf_ctx* c, int32_t enable) { return c ? pf::jobs_stats_reset(c, enable) : PF_EINVAL; }
int pf_jobs_stats_read(pf_ctx* c, pf_jobs_stats* o) { return (c && o) ? pf::jobs_stats_read(c, o) : PF_EINVAL; }

int pf_scan_prune_stats(pf_ctx* c, int64_t* out, int32_t reset) {
    if (!c || !out) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    unsigned long long v[5];
    HIPCHK(c, pf::k5_prune_stats_read(v, reset != 0));
    for (int i = 0; i < 5; ++i) out[i] = (int64_t)v[i];
    return PF_OK;
}

int pf_scan_bytes(pf_ctx* c, const int32_t* q, int32_t nq, int64_t* out) {
    if (!c || nq < 0 || (nq && (!q || !out))) return PF_EINVAL;
    (void)hipSetDevice(c->device);
    return pf::scan_bytes(c, q, nq, out);
}

void pf_decode_keys(const uint64_t* keys, int32_t n, int32_t* ou, float* os, int32_t* count) {
    int32_t m = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (keys[i] == ~0ull) break;
        if (ou) ou[m] = pf::key_uid(keys[i]);
        if (os) os[m] = pf::key_score(keys[i]);
        ++m;
    }
    if (count) *count = m;
}

int pf_layout(const pf_ctx* c, pf_layout_stats* o) {
    if (!c || !o) return PF_EINVAL;
    o->n_slots = c->hc.n;
    o->stream_bytes = c->stream_bytes;
    o->header_bytes = (int64_t)c->hc.n * 48;
    o->alg_bytes = c->hs.alg_bytes;
    o->packed_tokens = c->hs.packed ? 1 : 0;
    o->n_tiles = (int32_t)c->hs.tile_steps.size();
    o->post_bytes = c->post_bytes;
    o->scan_kernel = c->use_post() ? PF_SCAN_POSTINGS : PF_SCAN_STREAM;
    o->resident_images = c->jb.pimg ? 1 : 0;
    o->shard_cands = 0;
    o->shard_entries = 0;
    if (c->use_post()) {
        const int64_t bs = c->ps.bsize, n = c->hc.n;
        const int64_t i0 = std::min<int64_t>(n, (int64_t)c->wb_begin * bs), i1 = std::min<int64_t>(n, (int64_t)c->wb_end * bs);
        o->shard_cands = i1 - i0;
        if (i1 > i0) o->shard_entries = pf::block_range_entries(c->hc, i0, i1);
    } else {
        for (int32_t t = c->tile_begin; t < c->tile_end; ++t) {
            const int64_t s0 = c->hs.tile_slot0[t];
            const int64_t s1 = t + 1 < (int32_t)c->hs.tile_slot0.size() ? (int64_t)c->hs.tile_slot0[t + 1] : (int64_t)c->hc.n;
            o->shard_cands += s1 - s0;
        }
    }
    return PF_OK;
}

float pf_last_scan_ms(const pf_ctx* c) {
    if (!c) return 0.f;
    float ms = c->last_scan_ms;
    if (c->last_ev1 && hipEventSynchronize(c->last_ev1) == hipSuccess)
        (void)hipEventElapsedTime(&ms, c->last_ev0, c->last_ev1);
    return ms;
}

int pf_profile_reset(pf_ctx* c) {
    if (!c) return PF_EINVAL;
    c->prof_on = true;
    c->prof_used = 0;
    c->prof_seen = 0;
    c->last_ev0 = c->last_ev1 = nullptr;  // pool events are re-recorded from here on
    return PF_OK;
}

int pf_profile_sample(pf_ctx* c, int32_t every) {
    if (!c || every < 0) return PF_EINVAL;
    if (every == 0) {  // profiling off: launches use the context's own event pair again
        c->prof_on = false;
        c->prof_used = 0;
        c->last_ev0 = c->last_ev1 = nullptr;
        return PF_OK;
    }
    c->prof_every = every;
    return PF_OK;
}

int pf_profile_read(pf_ctx* c, double* total_ms, int64_t* launches) {
    if (!c || !total_ms || !launches) return PF_EINVAL;
    double tot = 0.0;
    for (size_t i = 0; i < c->prof_used; ++i) {
        HIPCHK(c, hipEventSynchronize(c->prof_ev[i].second));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->prof_ev[i].first, c->prof_ev[i].second));
        tot += ms;
    }
    *total_ms = tot;
    *launches = (int64_t)c->prof_used;
    return PF_OK;
}

}  // extern "C"
