// pf_jobs.h — launchers of the device job pipeline (pf_jobs.hip) and its per-image plan.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "pf_kernels.h"
#include "pf_types.h"

namespace pf {

// One query image K6 builds (layout of pf_scan_host.cpp image_ref): byte offsets into the image
// pool; lg = table log2 (load <= 0.4), lge = exclusion table log2, dlg = log2 of the set
// de-duplication table in scratch (u32 words from scr_off; the item list follows it; img_dlg).
struct ImgJob {
    int32_t idx, lg, lge, dlg;
    uint32_t const_off, keys_off, vals_off;
    uint32_t rows;  // (completion row + 1) | (age row + 1) << 16 in the image-builder tables (0: none;
                    // 0xFFFFFFFF: too many distinct values, K6 bisects the tables)
    int64_t scr_off;
};

inline int pow2_lg(int64_t n) {
    int lg = 4;
    while (((int64_t)1 << lg) < n) ++lg;
    return lg;
}

// images [0, n_small) build with kImgLdsSmall bytes of LDS, the next n_big with kImgLds, the next n_glob in
// global memory
constexpr uint32_t kImgLdsSmall = 16 * 1024;
hipError_t launch_qimages(const DevStore& st, const DevJobsStore& g, const ImgJob* ij, int n_small, int n_big, int n_glob,
                          uint8_t* pool, uint32_t* scratch, int32_t* fail, hipStream_t s);
uint32_t qimage_lds(int lg, int lge, int dlg, uint32_t nitems, bool packed);

// K6's inputs as host data, from the corpus alone (pf_store.cpp): what pf_open uploads into the K6 part
// of DevJobsStore, and what a device check of K6 uploads for a corpus of its own.
struct HostCorpus;
struct HostStore;
struct ImgTables {
    QConst tmpl;                           // the query-independent QConst fields
    std::vector<double> sig_reg;           // [a_regcnt 4][b 4][m 4] region rows
    std::vector<int32_t> comp_vals, age_vals;  // sorted distinct values > 0 ...
    std::vector<double> comp_rows, age_rows;   // ... and their rows [kValTab + 1] (glibc exp)
    // idf per column by tid rank (pf_store.h: the engine's token ids are column ranks), one dense
    // table for every column with an idf map (dense_off -1: none)
    std::vector<int64_t> dense_off;
    std::vector<int32_t> dense_len;
    std::vector<float> dense;
};
void build_img_tables(const HostCorpus& hc, bool packed, ImgTables& t);

// Per profile idx: the sizes of its K6 image (QConst | table | values).  lg[idx] == 0: the tables are
// outside the device limits, and nothing else of idx is meaningful.
struct ImgPlan {
    bool packed = true;
    int lge = 4;                 // the exclusion table is empty (the pair images carry no exclusions): lg_for(0)
    std::vector<uint8_t> lg;     // query-table log2 (pf_store.cpp build_query's first size)
    std::vector<int32_t> nset;   // clubs + friends words of the record
    std::vector<int32_t> ntok;   // its tokens
    std::vector<uint32_t> rows;  // ImgJob::rows (its completion / age rows in the image-builder tables)
};
void build_img_plan(const HostCorpus& hc, const HostStore& hs, const ImgTables& t, ImgPlan& p);

inline size_t img_a16(size_t x) { return (x + 15) & ~(size_t)15; }
inline size_t img_nkeys(const ImgPlan& p, int32_t idx) {  // 8-B entries: the table(s), then the exclusion table
    return ((size_t)(p.packed ? 1u : 3u) << p.lg[idx]) + ((size_t)1 << p.lge);
}
constexpr uint32_t kImgKeysOff = (uint32_t)sizeof(QConst);  // byte offsets from the image's start
inline uint32_t img_vals_off(const ImgPlan& p, int32_t idx) {
    return (uint32_t)img_a16(sizeof(QConst) + img_nkeys(p, idx) * 8);
}
inline size_t img_bytes(const ImgPlan& p, int32_t idx) {
    return img_vals_off(p, idx) + img_a16((size_t)p.ntok[idx] * sizeof(QVal));
}
// the set de-duplicating the record's clubs and friends at load <= 0.5; the wide format splits it into a half
// per kind (ids are any uint32 there, so the kind has no bit of the key to live in), each at that load
inline int img_dlg(const ImgPlan& p, int32_t idx) { return pow2_lg(2 * (int64_t)p.nset[idx] + 2) + (p.packed ? 0 : 1); }
inline ImgJob img_job(const ImgPlan& p, int32_t idx, uint32_t pool_off) {  // the image at byte pool_off of its pool
    ImgJob m{};
    m.idx = idx;
    m.lg = p.lg[idx];
    m.lge = p.lge;
    m.dlg = img_dlg(p, idx);
    m.rows = p.rows[idx];
    m.const_off = pool_off;
    m.keys_off = pool_off + kImgKeysOff;
    m.vals_off = pool_off + img_vals_off(p, idx);
    return m;
}
// K6 builds in three launches: 0 small LDS builds (<= kImgLdsSmall, many workgroups per CU),
// 1 large LDS builds (<= kImgLds), 2 hub users in global memory
inline int img_build_class(const ImgPlan& p, int32_t idx) {
    const int lg = p.lg[idx];
    const uint32_t need = lg ? qimage_lds(lg, p.lge, img_dlg(p, idx), (uint32_t)(p.nset[idx] + p.ntok[idx]), p.packed) : 0u;
    return need == 0 ? 2 : (need <= kImgLdsSmall ? 0 : 1);
}
// scratch words of a class-2 build: set + u64 items + the table's u64 copy (the SoA transform)
inline int64_t img_scratch_words(const ImgPlan& p, int32_t idx) {
    return ((int64_t)1 << img_dlg(p, idx)) + 2 * ((int64_t)p.nset[idx] + p.ntok[idx]) + 2 * (int64_t)img_nkeys(p, idx);
}
// One launch_qimages call over the images ij (their offsets set, any order): ordered small LDS builds |
// large LDS builds | global-memory builds, each global build's scratch after the last one's
struct ImgBatch {
    std::vector<ImgJob> ij;
    int nc[3] = {0, 0, 0};
    int64_t scr = 0;  // scratch words
};
inline void img_batch(const ImgPlan& p, const std::vector<ImgJob>& ij, ImgBatch& b) {
    std::vector<uint8_t> cls(ij.size());
    for (size_t x = 0; x < ij.size(); ++x) cls[x] = (uint8_t)img_build_class(p, ij[x].idx);
    b = ImgBatch{};
    b.ij.reserve(ij.size());
    for (int k = 0; k < 3; ++k)
        for (size_t x = 0; x < ij.size(); ++x)
            if (cls[x] == k) {
                ImgJob m = ij[x];
                m.scr_off = b.scr;
                if (k == 2) b.scr += img_scratch_words(p, m.idx);
                b.ij.push_back(m);
                ++b.nc[k];
            }
}

// K3's per-job hash table (DevJob::ht_lg; keys | pos | flags, 3 << lg int32 words): load <= 0.5 over
// row(u) + {u}, the kept candidates and one more round of claims.  kGatherChunk is K3's round (2 x
// pf_jobs.hip kGatherThreads): the last round claims up to this many table slots past the limit.
// all: a kDjAll job, whose table holds the exclusions only.
constexpr int64_t kGatherChunk = 2048;
inline int gather_ht_lg(bool all, int64_t nf, int64_t cap) {
    return all ? pow2_lg(2 * (nf + 1)) : pow2_lg(2 * (nf + 1 + cap + kGatherChunk));
}

// filt (fields == 0: none): the candidate filter of the batch's kDjAll jobs, tested on the tile headers of st
hipError_t launch_gather(const DevJobsStore& g, const DevView& v, const DevJob* jobs, int njobs, const int32_t* pool,
                         const int64_t* pool64, int32_t* ht, int32_t* seq, int32_t* cand_slot, int32_t* cand_id,
                         int32_t* ncand, const DevStore& st, const CandFilter& filt, hipStream_t s);
// K4' (+ the fused top-k of jobs with topk <= kMaxTopK: parts = gridDim.x * k keys per job,
// tickets = one zeroed counter per job, out = the chunk's key rows, k = their width)
hipError_t launch_collab(const DevJob* jobs, const int32_t* jix, int njobs, int max_cap, const int32_t* pool,
                         const float* pout, const int32_t* cand_slot, float* score, const int32_t* ids, uint64_t* parts,
                         unsigned int* tickets, uint64_t* out, int k, hipStream_t s);
hipError_t launch_clubs(const DevJobsStore& g, const DevView& v, const DevJob* jobs, const int32_t* jix, int njobs,
                        const int32_t* pool, const int64_t* pool64, const float* pout, double* acc,
                        float* score, int32_t* ids, int32_t* ncand, int64_t acc_stride, hipStream_t s);
// the pair blocks' dispatch order, longest first record first (pf_jobs.hip order_pairs_kernel)
hipError_t launch_expand_pairs(const PairGen* gens, int ngens, const int2* pool, int nblocks, PairBlock* blocks,
                               hipStream_t s);
hipError_t launch_order_pairs(const PairBlock* blocks, int nblocks, const int32_t* slots, int32_t n_slots,
                              int32_t* order, hipStream_t s);
// pair counts and bytes of the pair blocks (pf_jobs_stats)
hipError_t launch_pair_stats(const DevStore& st, const PairBlock* blocks, int nblocks, const int32_t* slots,
                             unsigned long long* acc, hipStream_t s);
hipError_t launch_job_topk(const DevJob* jobs, const int32_t* jix, int njobs, const float* score, const int32_t* ids,
                           const int32_t* slots, const int32_t* ncand, uint64_t* out, int k, hipStream_t s);

}  // namespace pf
