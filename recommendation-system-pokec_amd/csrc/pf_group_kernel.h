// pf_group_kernel.h — fas_group_kernel, the group scan (pf_group.h), and its launcher.  Included by
// pf_kernels.hip after K1's pieces it is built from: walk_chunk, fas_epilogue,
// filter_pass_tile, excluded, topk_push and post_tail.  K1 (fas_scan_kernel) scores a tile against
// one staged image; this sibling scores it against every image of a pass and folds the scores into
// one aggregate per candidate.
#pragma once
#include "pf_group.h"

namespace pf {

// what the kernel needs of one pass besides the images (by value in the launch's arguments)
struct GroupArgs {
    int32_t img0, nimg;
    uint32_t hits_off, hit_bytes;
    int32_t first, last, agg, n_seeds;
    int32_t excl_img, tile_begin, tile_end, k;
};

// The view of the pass's image at carve offset `off`: stage_query's, with the hit lists, hit counts
// and scratch shared by the pass.  The sizes are workgroup-uniform and read into SGPRs.
template <bool GTAB>
__device__ __forceinline__ QView group_view(char* smem, const uint8_t* pool, const QImageRef& r, uint32_t off,
                                            const GroupArgs& A) {
    auto uni = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
    char* b = smem + off;
    const QConst* q = reinterpret_cast<const QConst*>(b);
    QView v;
    v.q = q;
    v.lg = (int)uni((uint32_t)q->lg);
    v.lge = (int)uni((uint32_t)q->lg_excl);
    v.hmul = uni(q->hmul);
    v.excl_off = uni(q->excl_off);
    const uint32_t kb = 8u * (v.excl_off + (1u << v.lge));
    if (!GTAB || r.lds_bytes != 0u) {
        v.tab = reinterpret_cast<const uint32_t*>(b + sizeof(QConst));
        v.vals = reinterpret_cast<const QVal*>(b + sizeof(QConst) + kb);
    } else {
        v.tab = reinterpret_cast<const uint32_t*>(pool + (size_t)r.const_off * 16u + r.keys_off);
        v.vals = reinterpret_cast<const QVal*>(pool + (size_t)r.const_off * 16u + r.vals_off);
    }
    v.hits = smem + A.hits_off;
    v.nh = reinterpret_cast<uint32_t*>(smem + A.hits_off + (size_t)A.hit_bytes * blockDim.x);
    return v;
}

// GTAB = false: every image of the pass has its tables in LDS.  GTAB = true: an image with lds_bytes
// == 0 is probed in global memory, the others of the pass in LDS all the same.
template <bool PACKED, bool GTAB>
__global__ __launch_bounds__(kScanThreads, 4) void fas_group_kernel(DevStore st, const uint8_t* __restrict__ pool,
                                                                 const QImageRef* __restrict__ refs,
                                                                 const uint32_t* __restrict__ offs, GroupArgs A,
                                                                 double* __restrict__ accbuf,
                                                                 uint64_t* __restrict__ parts,
                                                                 ScanSync* __restrict__ sync,
                                                                 uint64_t* __restrict__ out, CandFilter F, FieldSel S,
                                                                 ScanWindow WN, uint32_t* __restrict__ totals,
                                                                 uint64_t* __restrict__ cbuf, uint32_t ccap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // stage the pass's images side by side (stage_query's copies, per image)
    for (int i = 0; i < A.nimg; ++i) {
        const QImageRef r = refs[A.img0 + i];
        char* dst = smem + offs[A.img0 + i];
        const uint8_t* base = pool + (size_t)r.const_off * 16u;
        if (!GTAB || r.lds_bytes != 0u) {
            const QConst* g = reinterpret_cast<const QConst*>(base);
            const uint32_t kb = 8u * (g->excl_off + (1u << g->lg_excl)), vb = (uint32_t)g->n_vals * 16u;
            stage4(dst, g, sizeof(QConst));
            stage4(dst + sizeof(QConst), base + r.keys_off, kb);
            stage4(dst + sizeof(QConst) + kb, base + r.vals_off, vb);
        } else {
            stage(dst, base, sizeof(QConst));
        }
    }
    __syncthreads();
    // a field selection patches every staged copy of the constants, never an image
    if (S.on != 0u) {
        for (int i = (int)threadIdx.x; i < A.nimg; i += (int)blockDim.x)
            select_apply(*reinterpret_cast<QConst*>(smem + offs[A.img0 + i]), S);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t list = ~0ull;
    uint32_t wcnt = 0u;  // a counted window: the wave's keys in it
    // Static tile hand-out, longest tiles first: band b = tiles [b*W, (b+1)*W), wave w takes one per
    // band, alternating direction.  A slot is owned by one wave per pass, and the stream orders the passes.
    const int W = (int)gridDim.x * (kScanThreads / 64), wid = (int)blockIdx.x * (kScanThreads / 64) + wave;
    const int ntiles = A.tile_end - A.tile_begin;
    const double ident = A.agg == kGroupMean ? 0.0 : (A.agg == kGroupMin ? __builtin_huge_val() : -__builtin_huge_val());
    for (int b = 0; b * W < ntiles; ++b) {
        const int tile = A.tile_begin + b * W + ((b & 1) ? W - 1 - wid : wid);
        if (tile >= A.tile_end) continue;
        // K1's tile set-up, unchanged (split records: lgk > 0)
        const uint32_t lgk = st.tile_lgk[tile];
        const int slot0 = (int)st.tile_slot0[tile];
        const int cand = lane >> lgk, ci = lane & ((1 << lgk) - 1);
        const bool active = cand < min(kTileSlots >> lgk, st.n_slots - slot0);
        const int p = slot0 + cand;
        uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0, h2 = h0;
        if (active) {
            h2 = st.hdr2[p];
            h0 = st.hdr0[p];
            h1 = st.hdr1[p];
        }
        const uint32_t nc = h2.y, nset = h2.y + h2.z;
        const uint32_t len = record_words(h2, PACKED);
        const uint32_t q = chunk_words(len, lgk, PACKED);
        const uint32_t j0 = (uint32_t)ci * q;
        const uint32_t clen = (active && len > j0) ? min(q, len - j0) : 0u;
        const Loc l{tile, cand, lgk};
        uint32_t pend0 = 0;
        if (!PACKED && clen > 0 && j0 > 0) pend0 = word_at(st, l, q, j0 - 1);  // a token pair may straddle chunks
        // a candidate the filter fails is walked with its tile but gets no epilogue, no slot and no key
        const bool scored = active && ci == 0 && (F.fields == 0u || filter_pass_tile(F, h0, h1, h2));
        double acc = ident;
        if (scored && !A.first) acc = accbuf[p];
        const uint4* col = st.stream + st.tile_off[tile] + lane;
        for (int i = 0; i < A.nimg; ++i) {
            const QView v = group_view<GTAB>(smem, pool, refs[A.img0 + i], offs[A.img0 + i], A);
            Walk Wk;
            Wk.cnt = 0; Wk.nh = 0; Wk.pend = pend0;
            // every image walks the same tile: the first walk brings its lines in, the others ask for them again
            walk_chunk<PACKED, false>(Wk, col, j0, clen, nc, nset, v, blockDim.x);
            uint32_t cnt = Wk.cnt;
            for (int m = 1; m < (1 << lgk); m <<= 1) cnt += (uint32_t)__shfl_xor((int)cnt, m);
            v.nh[threadIdx.x] = Wk.nh;
            wave_sync();
            if (scored) {
                const uint32_t* nhp = v.nh + threadIdx.x;
                const TileRec rec{&st, l, q};
                const float f = fas_epilogue<PACKED>(v, rec, h0, h1, h2, cnt, threadIdx.x, 1u << lgk,
                                                     [&](uint32_t g) { return nhp[g]; });
                const double d = (double)f;
                if (A.agg == kGroupMean) acc += d;
                else if (A.agg == kGroupMin) acc = d < acc ? d : acc;
                else acc = d > acc ? d : acc;
            }
            wave_sync();  // the next image's walk rewrites the hit lists this epilogue read
        }
        if (!A.last) {
            if (scored) accbuf[p] = acc;
            continue;
        }
        uint64_t key = ~0ull;
        if (scored) {
            const int32_t uid = (int32_t)h1.w;
            const QView ve = group_view<GTAB>(smem, pool, refs[A.excl_img], offs[A.excl_img], A);
            const float f = A.agg == kGroupMean ? (float)(acc / (double)A.n_seeds) : (float)acc;
            if (!excluded<PACKED>(ve, (uint32_t)uid)) key = score_key(f, uid);
        }
        // the score window (pf_window.h; fields == 0: none), on the aggregate's key
        if (WN.fields != 0u) {
            if (!window_pass(key, WN)) key = ~0ull;
            if (WN.fields & kWinCount) wcnt += (uint32_t)__popcll(__ballot(key != ~0ull));
            // a collecting launch keeps the aggregate's key (the wave is whole here: the tile is the wave's)
            if (WN.fields & kWinCollect) collect_append(key, ~0ull, &sync->ccursor, cbuf, ccap, lane);
        }
        topk_push(list, key, A.k, lane);
    }
    if (!A.last) return;
    post_tail(list, A.k, reinterpret_cast<uint64_t*>(smem + A.hits_off + ((size_t)A.hit_bytes + 4u) * blockDim.x), sync,
              parts, out, nullptr, 0, (int)blockIdx.x, (int)gridDim.x, (WN.fields & kWinCount) != 0u, wcnt, totals);
}

using GroupKernel = decltype(&fas_group_kernel<false, false>);
static GroupKernel group_kernel(bool packed, bool gtab) {
    static constexpr GroupKernel tab[2][2] = {{fas_group_kernel<false, false>, fas_group_kernel<false, true>},
                                              {fas_group_kernel<true, false>, fas_group_kernel<true, true>}};
    return tab[packed][gtab];
}

hipError_t launch_group(const GroupLaunch& L) {
    if (L.pass.nimg <= 0) return hipSuccess;
    if (!extras_ok(L.x, 1)) return hipErrorInvalidValue;
    const GroupArgs A{L.pass.img0, L.pass.nimg, L.pass.hits_off, L.hit_bytes, L.first ? 1 : 0, L.last ? 1 : 0, L.agg,
                      L.n_seeds, L.excl_img, L.tile_begin, L.tile_end, L.k};
    hipLaunchKernelGGL(group_kernel(L.st.packed, L.pass.gtab), dim3(L.blocks), dim3(kScanThreads), L.pass.lds, L.s, L.st,
                       L.pool, L.refs_dev, L.off_dev, A, L.acc, L.parts, L.sync, L.out, L.x.filt, L.x.sel, L.x.win, L.x.totals,
                       L.x.collect, L.x.collect_cap);
    return hipGetLastError();
}

int group_blocks_per_cu(bool packed, bool gtab, uint32_t lds) {
    int nb = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, group_kernel(packed, gtab), kScanThreads, lds);
    return (e == hipSuccess && nb > 0) ? nb : 1;
}

}  // namespace pf
