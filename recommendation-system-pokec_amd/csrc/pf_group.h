// pf_group.h — the group scan (pf_recommend_group): host-callable launcher of fas_group_kernel
// (pf_group_kernel.h, compiled in pf_kernels.hip) and the plan of its passes.
//
// A group query scores every candidate of the shard against G seed images and ranks the per-candidate
// aggregate (mean, min or max of the G scores).  The seeds are packed, in the caller's order, into
// passes: one launch per pass stages the pass's images side by side in LDS, and a wave that holds a
// tile probes each of them in turn before it moves on, so the record stream is requested once per
// pass, not once per seed.  (As measured the later walks of a tile miss L2 like the first: the tiles
// of a CU's resident waves are more than its share of L2 holds.  profiles/GROUP_INDEX.md.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pf_scan_call.h"
#include "pf_types.h"

namespace pf {

// LDS carve of a pass: [image 0: QConst | tables | vals][image 1: ...] ... [hit lists hit_bytes x
// threads][hit counts 4 x threads][merge scratch 2 KiB].  The hit lists, hit counts and scratch exist
// once and are reused by every image of the pass (a wave finishes one image's epilogue before it walks
// the next).  An image whose tables are probed in global memory (QImageRef::lds_bytes == 0) takes
// only its QConst.
// The budget trades images per pass against workgroups per CU.  As measured (profiles/GROUP_INDEX.md,
// 1,632,803 users, device ms at G = 16 / 64 / 256): 40 KiB 6.70 / 26.8 / 112.5, 56 KiB 8.26 / 31.7 / 126.7,
// 80 KiB 7.83 / 31.7 / 131.5, 160 KiB 12.8 / 54.9 / 225.3: occupancy wins over images per pass (a tile's
// later walks miss L2 as the first does), so the default keeps four workgroups per CU.
constexpr uint32_t kGroupLdsBudgetDefault = 40u * 1024u;  // PF_DEBUG group_lds=BYTES
constexpr uint32_t kGroupTailLds = 4u * (uint32_t)kScanThreads + 2048u;

struct GroupPass {
    int32_t img0, nimg;   // images [img0, img0 + nimg) of the launch's refs
    uint32_t hits_off;    // byte offset of the hit lists in the carve (= the images' bytes)
    uint32_t lds;         // dynamic LDS bytes of the launch
    bool gtab;            // some image of the pass probes global memory
};

// The packing rule: a pass is the longest prefix of the remaining images whose carve fits `budget`
// (at least one image, at most `tile` images when tile > 0).  img_lds[i] = sizeof(QConst) + the
// image's staged table bytes; hit_bytes = hit-list bytes per lane.  off[i] = image i's byte offset
// in its pass's carve.
inline std::vector<GroupPass> group_pack(const std::vector<uint32_t>& img_lds, const std::vector<uint8_t>& global_tab,
                                         uint32_t hit_bytes, uint32_t budget, int tile, std::vector<uint32_t>& off) {
    std::vector<GroupPass> passes;
    off.assign(img_lds.size(), 0u);
    const uint32_t fixed = hit_bytes * (uint32_t)kScanThreads + kGroupTailLds;
    size_t i = 0;
    while (i < img_lds.size()) {
        GroupPass p{(int32_t)i, 0, 0u, 0u, false};
        uint32_t used = 0;
        while (i < img_lds.size() && (p.nimg == 0 || ((tile <= 0 || p.nimg < tile) && used + img_lds[i] + fixed <= budget))) {
            off[i] = used;
            used += img_lds[i];
            p.gtab = p.gtab || global_tab[i] != 0;
            ++p.nimg;
            ++i;
        }
        p.hits_off = used;
        p.lds = used + fixed;
        passes.push_back(p);
    }
    return passes;
}

constexpr int kGroupMean = 0, kGroupMin = 1, kGroupMax = 2;

// One pass of a group scan over tiles [tile_begin, tile_end).  Passes of one query are separate
// launches on one stream, in order: the stream orders a pass's reads of `acc` after the stores of
// the pass before it.
struct GroupLaunch {
    const DevStore& st;  // st.packed and pass.gtab are the instantiation
    const uint8_t* pool;
    const QImageRef* refs_dev;   // every image of the query
    const uint32_t* off_dev;     // per image: its byte offset in its pass's carve (group_pack)
    const GroupPass& pass;
    uint32_t hit_bytes;
    bool first, last;            // first: acc starts from the aggregate's identity; last: rank and merge
    int agg, n_seeds;            // kGroup*; the mean's divisor G
    int excl_img;                // last pass: the image (index in refs) whose exclusion table holds the union
    int tile_begin, tile_end, k, blocks;
    double* acc;                 // [n_slots] partial aggregate between passes (untouched by a one-pass query)
    uint64_t *parts, *out;       // last pass: post_tail's lists ((blocks + 8) x k) and the result row
    ScanSync* sync;              // last pass: one zeroed rendezvous
    hipStream_t s;
    const ScanExtras& x;         // the call's filter, selection, uid-keyed window, count word and collector (pf_scan_call.h)
};
hipError_t launch_group(const GroupLaunch& L);
// resident workgroups per CU of a pass's instantiation at its LDS size
int group_blocks_per_cu(bool packed, bool gtab, uint32_t lds);

}  // namespace pf
