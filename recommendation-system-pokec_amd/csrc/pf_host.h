// pf_host.h — what the engine's host translation units share (as pf_batch.h does for the job
// pipeline): pf_scan_host.cpp (query images, staging, the K5 / K1 launches and their routing),
// pf_pairs_host.cpp (the pair kernels' chunks), pf_group_api.cpp, pf_clubs_api.cpp and pf_api.cpp
// (the C ABI, its setters and their validation).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "pf_ctx.h"
#include "pf_kernels.h"
#include "pf_pair_groups.h"
#include "pf_stage.h"
#include "pf_store.h"
#include "pokec_fas.h"

namespace pf {

// ---------------------------------------------------------------- query images (pf_scan_host.cpp)
// Query images -> one byte pool + refs.
struct Images {
    std::vector<uint8_t> pool;
    std::vector<QImageRef> refs;
    uint32_t max_lds = 0;  // dynamic LDS a block needs for the largest image (image_ref's thread count)
    bool gtab = false;     // some image probes its table in global memory
    uint32_t max_img = 0;  // the largest staged keys + vals (plan_images): K1t's LDS past the QConst
};
// image q's ref for an image starting at pool byte `start` (a multiple of 16), appended to im.refs,
// and its share of a launch's needs for blocks of `threads` threads; returns the image's bytes
size_t image_ref(Images& im, const QImageHost& q, size_t start, uint32_t threads);
// one image appended to im.pool (K1, the group kernel)
void add_image(Images& im, const QImageHost& q);
// Many images at once (the pair kernels): refs and offsets first (returns the pool bytes), then
// fill_images copies them on threads into `dst` (pinned; a few thousand images per chunk).
size_t plan_images(Images& im, const std::vector<QImageHost>& qs);
void fill_images(const Images& im, const std::vector<QImageHost>& qs, uint8_t* dst, size_t total);

// the exclusion list of a stored user's own query: its adj_list row, then itself
std::vector<int32_t> self_excl(const HostCorpus& hc, int32_t idx);
// a postings image's header (pf_types.h QPostHead, after the QConst) and its K5 launch's variable LDS
inline const QPostHead* post_head(const uint8_t* img) { return reinterpret_cast<const QPostHead*>(img + sizeof(QConst)); }
inline uint32_t post_var_lds(const QPostHead& h) { return post_var_lds(h.n_tok, h.n_tok + h.n_club + h.n_friend); }

// ---------------------------------------------------------------- staging and timing (pf_scan_host.cpp)
// One launch's staging buffer, laid out by L (pf_stage.h), to `buf` in one async copy on s: sections
// 0 - 2 from src[i] (nullptr: zeros), the last from `pool`, n_pool pieces end to end.  base = the
// device copy's start (section i at base + L.off[i]).  wait_stage: the host_prof stage that takes the
// time spent waiting for a free pinned slot (-1: none).
struct StagePiece {
    const void* p;
    size_t bytes;
};
int stage_send(pf_ctx* c, const StageLayout<4>& L, const void* const (&src)[3], const StagePiece* pool, size_t n_pool,
               DBuf& buf, hipStream_t s, uint8_t*& base, int wait_stage = -1);
// Timing events of one scan launch (the profiling pool when pf_profile_reset is on).  A
// launch the caller passes timed = false, or that sampling skips, records nothing and clears
// last_ev0/last_ev1, so pf_last_scan_ms never reports another launch's time.
int scan_events(pf_ctx* c, bool& timed, hipEvent_t& e0, hipEvent_t& e1);
// the same for launches that take no events of their own (K1, the group's passes): recorded around them on s
int timed_begin(pf_ctx* c, bool& timed, hipEvent_t& e0, hipEvent_t& e1, hipStream_t s);
int timed_end(pf_ctx* c, bool timed, hipEvent_t e0, hipEvent_t e1, hipStream_t s);

// ---------------------------------------------------------------- scans (pf_scan_host.cpp)
// One synchronous all-candidates call: by uid, by profile or by group, and the scan under a clubs
// call.  begin() refuses what a collector cannot serve, readies the result rows and the count words
// and makes the call's options a value (`call`, pf_scan_call.h), which the caller hands to its
// launches; keys() brings rows back and decodes them; finish() reads the counts and, for a
// collecting call, sorts the keys.  Rows: the launches get absolute result rows (row r of d_out,
// count word r) and the base of the count words; a launch that counts one query into word 0 names
// its row (scan_post_one, a group's passes).
struct SyncScan {
    pf_ctx* c;
    pf_scan_window win;   // the caller's own window (validated)
    int64_t cap;          // the collector's cap in keys; 0: none
    // the totals (only under the caller's own PF_WIN_COUNT) and the collected keys go to the context
    // (pf_scan_window_totals, pf_scan_collected).  false (the clubs calls): the context keeps what
    // it had; the total stays here and the sorted keys on the device (d_coll_sorted)
    bool store;
    ScanCall call{};
    int nq = 0;
    int64_t total = 0;    // a collecting call's matches, after finish()
    explicit SyncScan(pf_ctx* ctx) : c(ctx), win(ctx->win_pub), cap(ctx->coll_cap), store(true) {}
    SyncScan(pf_ctx* ctx, const pf_scan_window& w, int64_t k) : c(ctx), win(w), cap(k), store(false) {}
    // n queries (or groups) into `rows` rows of d_out, empty (0xFF) first when `fill`
    int begin(int n, size_t rows, int topk, bool fill);
    // rows [0, n) of d_out on the host, decoded; launched: a launch ran, whose events time the call
    int keys(int n, int topk, bool launched, int32_t* ou, float* os, int32_t* oc);
    int finish();
};

int scan_lanes();  // PF_DEBUG scan_lanes (pf_open creates the streams of lanes past the third)
// All-candidates scan for `idx` (valid query indices) into d_keys rows `rows`, K5 or K1 per query
int scan_all(pf_ctx* c, const ScanCall& C, const std::vector<int32_t>& idx, const std::vector<int32_t>& rows, int k,
             uint64_t* d_keys, hipStream_t s, bool timed);
// the synchronous calls over it: up to 64 results per query by uid, and by by-value profile
int recommend_uids(pf_ctx* c, SyncScan& S, const int32_t* q, int32_t nq, int32_t topk, int32_t* ou, float* os, int32_t* oc);
int recommend_profiles(pf_ctx* c, SyncScan& S, const std::vector<ProfileOwned>& ps, int32_t topk, int32_t* ou, float* os,
                       int32_t* oc);
// the collector's buffer, grown to hold cap keys
int collect_reserve(pf_ctx* c, int64_t cap);
// the by-value profiles of a call, checked and resolved against the engine's corpus
int resolve_profiles(pf_ctx* c, const pf_query_profile* q, int32_t nq, std::vector<ProfileOwned>& ps);
int build_resident_post(pf_ctx* c);  // at open: every user's K5 image part
int scan_bytes(pf_ctx* c, const int32_t* q, int32_t nq, int64_t* out);  // pf_scan_bytes
// bytes one K1 (or group) pass reads: the shard's record stream and headers, whatever the query
int64_t k1_pass_bytes(const pf_ctx* c);
// postings entries (tokens, clubs, friends) of the candidates [i0, i1)
int64_t block_range_entries(const HostCorpus& hc, int64_t i0, int64_t i1);

// ---------------------------------------------------------------- pairs (pf_pairs_host.cpp)
// FAS(A = qidx[g], B = slots[g][j]) for every group g, on the GPU (K1').
// keep (optional): every chunk's scores stay on the device in one buffer, group g at
// (*goff)[g] (the collaborative sums read their matrix rows there)
// sel (on == 0: none): a field selection every pair is scored under (pf_fas_pairs_select)
// pv (optional): the A side of every group is this by-value profile, not a stored user
int run_pairs(pf_ctx* c, const std::vector<int32_t>& qidx, const std::vector<std::vector<int32_t>>& slots,
              std::vector<std::vector<float>>& out, DBuf* keep = nullptr, std::vector<int64_t>* goff = nullptr,
              const FieldSel& sel = FieldSel{}, const ProfileView* pv = nullptr);
// The breakdown of the same pairs (K1t, pf_terms.hip): pair j of group g writes head[dest[g][j]] and
// the row (W = 7 + T doubles) terms + dest[g][j] * W.
int run_pair_terms(pf_ctx* c, const std::vector<int32_t>& qidx, const std::vector<std::vector<int32_t>>& slots,
                   const std::vector<std::vector<int64_t>>& dest, pf_pair_terms_head* head, double* terms,
                   const FieldSel& sel, const ProfileView* pv = nullptr);
// the pairs (a[i], b[i]) of [i0, i1) grouped against c's corpus (a == nullptr: one group, pf_pair_groups.h);
// unknown(i) for a pair with an unknown uid
template <class Unknown>
inline void group_pairs(const pf_ctx* c, const int32_t* a, const int32_t* b, int64_t i0, int64_t i1, PairGroups& pg, Unknown unknown) {
    pg.add_uids(a, b, i0, i1, [c](int32_t u) { return c->hc.idx_of(u); }, [c](int32_t i) { return c->hs.slot_of_idx[i]; }, unknown);
}
inline void group_pairs(const pf_ctx* c, const int32_t* a, const int32_t* b, int64_t i0, int64_t i1, PairGroups& pg) {
    group_pairs(c, a, b, i0, i1, pg, [](int64_t) {});
}

// ---------------------------------------------------------------- the setters' validation (pf_api.cpp)
void set_open_error(const std::string& m);  // pf_open's thread-local error text
// The device form of a public selection: PF_EINVAL for unknown bits; NULL, or one that leaves out
// nothing of this engine's T columns, is no selection (on == 0).
int make_select(const pf_ctx* c, const pf_field_select* s, FieldSel& d);
// a caller's window as a call's options take it (null or fields == 0: none), or PF_EINVAL with the reason
int make_window(pf_ctx* c, const pf_scan_window* w, pf_scan_window& d);

// ---------------------------------------------------------------- group query (pf_group_api.cpp)
int group_args(pf_ctx* c, const pf_group_query* g);
std::vector<int32_t> group_seeds(const pf_ctx* c, const pf_group_query& g);  // the kept seeds, in the caller's order
int recommend_groups(pf_ctx* c, SyncScan& S, const pf_group_query* g, int32_t ng, int32_t topk, int32_t* ou, float* os,
                     int32_t* oc);

}  // namespace pf
