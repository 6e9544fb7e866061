// pf_kernels.h — host-callable launchers of the gfx950 kernels (pf_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "pf_scan_call.h"
#include "pf_types.h"

namespace pf {

// One block of the pair kernel, kPairThreads threads, one pair each: FAS(image qimg,
// slots[begin + i]) -> out[out + i] for i < count <= kPairThreads; a slot < 0 is skipped (its
// output is not written).  512: one staged image serves eight waves, and two workgroups per CU
// hold 16 waves where 256-thread ones held 12 (their LDS, mostly the per-lane hit lists).
constexpr int kPairThreads = 512;
struct PairBlock {
    int32_t qimg, begin, count, out;
};

// A run of pair blocks, expanded on the device (pf_jobs.hip expand_pairs_kernel): block
// first + x * nf + f (chunk x < nch, entry f < nf) scores image pool[fl + f].x against candidates
// [cand + x * kPairThreads, + min(kPairThreads, cap - x * kPairThreads)) into out + pool[fl + f].y * stride
// + x * kPairThreads (chunk-major: one candidate chunk's friends consecutive, sharing its records
// in cache)
struct PairGen {
    int32_t nf, nch, cap, cand, fl, stride, out, first;
};

// Each launcher takes one descriptor, filled with named members at the call; no member has a default,
// and a call that leaves out a reference does not compile.  A kernel's run-time choice of instantiation
// is made by one function in pf_kernels.hip, which its launch and its occupancy query both go through.
// K1, the record-stream scan of tiles [tile_begin, tile_end) for nq query images
struct ScanLaunch {
    const DevStore& st;  // st.packed and gtab are the instantiation
    const uint8_t* pool;
    const QImageRef* refs_dev;
    // dynamic LDS bytes per block = max over the batch of sizeof(QConst) + staged keys/vals + n_hits_max * threads + 2048
    uint32_t lds;
    // at least one image of the batch probes its table in global memory (lds_bytes == 0); the whole
    // launch then uses the global-table variant
    bool gtab;
    int nq, tile_begin, tile_end, k, blocks;
    uint64_t *parts, *out;
    ScanSync* sync;
    const int32_t* out_rows;
    hipStream_t s;
    const ScanExtras& x;  // the call's filter, selection, uid-keyed window, count words and collector (pf_scan_call.h)
};
hipError_t launch_scan(const ScanLaunch& L);
// resident scan blocks per CU at this dynamic LDS size (HIP occupancy API)
int scan_blocks_per_cu(bool packed, bool gtab, uint32_t lds);
// K5 postings scan over candidate blocks [blk_begin, blk_end) for nq query images (byte
// offsets img_off[] into pool); var_lds = post_var_lds(max n_tok, max lists of an image)
uint32_t post_var_lds(int n_tok, int n_lists);
uint32_t post_lds(uint32_t var_lds);
// mode flags (pf_scan_host.cpp post_mode).  Claimed launches and batches alike: kPostPrune = drop candidates
// below the query's shared score threshold (pf_prune.h; a batch query's is its own sync[q]),
// kPostPruneBlockOnly = at block starts only, kPostPruneStats = count them.  kPostFiltKeepBlocks (filtered launches, A/B): a block in which no
// candidate passes the filter runs to its end instead of leaving after its first barrier.
constexpr uint32_t kPostPrune = 1u << 16, kPostPruneStats = 1u << 17, kPostPruneBlockOnly = 1u << 18;
constexpr uint32_t kPostFiltKeepBlocks = 1u << 19;
// dynamic LDS a filtered launch takes on top of post_lds(var_lds): the filter, parked past the query's tables
constexpr uint32_t kFiltLds = (uint32_t)sizeof(CandFilter);
static_assert(kFiltLds % 16 == 0, "the window's words follow the filter's");
// ... and a windowed one: the window, parked past the filter
constexpr uint32_t kWinLds = 32;
static_assert(sizeof(ScanWindow) <= kWinLds, "the window's LDS");
struct PostLaunch {
    const PostStore& ps;
    const uint8_t* pool;
    const uint32_t* img_off;
    uint32_t var_lds;
    int nq, blk_begin, blk_end, k, blocks;
    uint64_t *parts, *out;
    ScanSync* sync;  // one per query, zeroed (theta and histogram included); the launch leaves each zeroed (post_tail)
    const int32_t* out_rows;
    // the block hand-out, which is the instantiation.  true (nq == 1 only): the grid's workgroups
    // claim every block per XCD group; false: workgroup x of query y takes every blocks-th block of
    // the range, in XCD-contiguous order (the batches, a class of one query of a batch included)
    bool claimed;
    uint32_t mode;
    // timed launches (both given): the kernel's own start and end timestamps, taken from its dispatch
    hipEvent_t e0, e1;
    hipStream_t s;
    // nullptr (each image starts with its QConst) or, for a one-query launch from the resident images, the
    // user's QConst elsewhere (its K1' resident image); the image = the resident part's start minus sizeof(QConst)
    const uint8_t* qconst;
    // the call's filter, selection, idx-keyed window, count words and collector (pf_scan_call.h): the
    // filter, the selection and the window each pick an instantiation (FILT, SEL, WIN)
    const ScanExtras& x;
};
hipError_t launch_post(const PostLaunch& L);
// workgroups per CU of the instantiation launch_post takes for `claimed`, `filtered` (a filter is
// set), `selected` (a field selection is set) and `windowed` (a score window is set)
int post_blocks_per_cu(uint32_t var_lds, bool claimed, bool filtered, bool selected, bool windowed);
// candidates of idx range [i0, i1) of the postings headers (ps.hdr), or with ps.hdr null of slots
// [i0, i1) of the tile headers, that pass filt: added to *count (device, zeroed by the caller)
hipError_t launch_filter_count(const PostStore& ps, const DevStore& st, int32_t i0, int32_t i1, const CandFilter& filt,
                               unsigned long long* count, hipStream_t s);
// K5 pruning counters of the launches with kPostPruneStats since the last reset (synchronises the device):
// out[5] = candidates seen, dropped at a block's start, dropped at a round's end, blocks, blocks
// begun with no threshold yet
hipError_t k5_prune_stats_read(unsigned long long* out, bool reset);
// plain merge of key lists (cross-shard merge after the all-gather)
hipError_t launch_merge(const uint64_t* in, int nparts, int64_t part_stride, int64_t query_stride, int nq, int k,
                        uint64_t* out, hipStream_t s);
// K1', one workgroup per PairBlock
struct PairsLaunch {
    const DevStore& st;  // st.packed and gtab are the instantiation
    const uint8_t* pool;
    const QImageRef* refs_dev;
    uint32_t max_lds;
    bool gtab;
    const PairBlock* blocks;
    int nblocks;
    const int32_t *order, *slots;  // order (nullable): the dispatch order, block blockIdx.x scores blocks[order[blockIdx.x]]
    float* out;
    hipStream_t s;
    // on == 0: none; applied to every block's staged constants (pf_fas_pairs_select, the pair stage of a job chunk)
    const FieldSel& sel;
};
hipError_t launch_pairs(const PairsLaunch& L);
// K1t (pf_terms.hip), the score breakdown: one workgroup of kTermsThreads per PairBlock of count <=
// kTermsPairs pairs, one wave per pair, the block's waves taking its pairs in turn against the one
// staged image.  Pair i of a block writes head[out + i] and the row terms[(out + i) * (PF_NUM_FIXED +
// st.n_cols)]; a slot < 0 writes score NaN, both masks 0 and the row 0.0, so every output is defined.
constexpr int kTermsThreads = 256;
constexpr int kTermsPairs = 32;
struct TermsLaunch {
    const DevStore& st;  // st.packed and gtab are the instantiation
    const uint8_t* pool;
    const QImageRef* refs_dev;
    // dynamic LDS bytes per block = sizeof(QConst) + the largest staged keys/vals of the launch's images
    // (the kernel keeps no hit list)
    uint32_t lds;
    bool gtab;
    const PairBlock* blocks;
    int nblocks;
    const int32_t* slots;
    pf_pair_terms_head* head;
    double* terms;
    hipStream_t s;
    // on == 0: none; applied to every block's staged constants, as in PairsLaunch
    const FieldSel& sel;
};
hipError_t launch_terms(const TermsLaunch& L);

}  // namespace pf
