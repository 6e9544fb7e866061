// pf_terms.hip — gfx950 kernel of the FAS score breakdown (DESIGN.md "Score breakdown").
//
//   fas_terms_kernel  K1t  per (query image, candidate slot) pair: the reference's per-field
//                          sigmoid terms (recommender_similarity.cpp:38-114), the mask of the
//                          slots that were added, and the score formed from them
//
// One wave per pair.  The scoring kernels give a lane one candidate and keep its token hits in a
// per-lane LDS list; here the wave reads one candidate's row-store record together, 64 words per
// round (one coalesced load), as the pair epilogue's overflow walk does.  Club and friend words
// are probed and counted by ballot; token hits are taken in record order through a ballot, so a
// column's dot is accumulated in ascending-tid order like everywhere else; lane t then owns text
// column t (T <= 64 = the wave) and computes its term, lanes 0..6 keep the fixed terms, and the
// row leaves in two coalesced stores.  There is no hit list, so no kHitCap overflow case.
// A workgroup is kTermsWaves waves that share one staged query image and take the block's pairs
// in turn.  Its own translation unit: the scoring kernels' code objects do not see it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_device.h"
#include "pf_kernels.h"
#include "pf_select.h"

namespace pf {

static_assert(sizeof(pf_pair_terms_head) == 16, "pf_pair_terms_head is one 16-B store");
static_assert(kMaxCols <= kWave, "lane t owns column t");
static_assert(kTermsThreads % kWave == 0, "whole waves");
constexpr int kTermsWaves = kTermsThreads / kWave;

__device__ __forceinline__ uint32_t uni32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) { return (uint64_t)uni32((uint32_t)x) | ((uint64_t)uni32((uint32_t)(x >> 32)) << 32); }

// The block's query image in LDS: [QConst][tables][vals] and nothing else (the scoring kernels'
// stage_query carves per-lane hit lists and merge scratch after them, which this kernel has not).
// GTAB = false: tables and values are staged, so every probe is a ds_read (the view's pointers come
// from the LDS symbol only); GTAB = true (some image of the launch is too large): only the
// constants are staged and the probes read global memory.  A field selection (uniform, on == 0:
// none) patches the staged copy of the constants, never the image, as in stage_query.
template <bool GTAB>
__device__ __forceinline__ QView stage_image(char* smem, const uint8_t* pool, const QImageRef& r, const FieldSel& S) {
    const uint8_t* base = pool + (size_t)r.const_off * 16u;
    if constexpr (!GTAB) {
        const QConst* g = reinterpret_cast<const QConst*>(base);
        const uint32_t kb = 8u * (g->excl_off + (1u << g->lg_excl)), vb = (uint32_t)g->n_vals * 16u;
        if (r.keys_off == sizeof(QConst) && r.vals_off == r.keys_off + kb) {
            stage4(smem, g, (uint32_t)sizeof(QConst) + kb + vb);
        } else {
            stage4(smem, g, sizeof(QConst));
            stage4(smem + sizeof(QConst), base + r.keys_off, kb);
            stage4(smem + sizeof(QConst) + kb, base + r.vals_off, vb);
        }
    } else {
        stage(smem, base, sizeof(QConst));
    }
    __syncthreads();
    if (S.on != 0u) {
        if (threadIdx.x == 0) select_apply(*reinterpret_cast<QConst*>(smem), S);
        __syncthreads();
    }
    const QConst* q = reinterpret_cast<const QConst*>(smem);
    QView v{};  // no hit list, no hit counts
    v.q = q;
    v.lg = (int)uni32((uint32_t)q->lg);
    v.lge = (int)uni32((uint32_t)q->lg_excl);
    v.hmul = uni32(q->hmul);
    v.excl_off = uni32(q->excl_off);
    if constexpr (!GTAB) {
        const uint32_t kb = 8u * (v.excl_off + (1u << v.lge));
        v.tab = reinterpret_cast<const uint32_t*>(smem + sizeof(QConst));
        v.vals = reinterpret_cast<const QVal*>(smem + sizeof(QConst) + kb);
    } else {
        v.tab = reinterpret_cast<const uint32_t*>(base + r.keys_off);
        v.vals = reinterpret_cast<const QVal*>(base + r.vals_off);
    }
    return v;
}

template <bool PACKED, bool GTAB>
__global__ __launch_bounds__(kTermsThreads) void fas_terms_kernel(DevStore st, const uint8_t* __restrict__ pool,
                                                                  const QImageRef* __restrict__ refs,
                                                                  const PairBlock* __restrict__ blocks,
                                                                  const int32_t* __restrict__ slots,
                                                                  pf_pair_terms_head* __restrict__ head,
                                                                  double* __restrict__ terms, FieldSel S) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PairBlock b = blocks[blockIdx.x];
    // the staged constants carry the selection (select_apply): a deselected slot is missing on the
    // query's side, and q.n_cols is the denominator's T'.  The row keeps the engine's width.
    const QView v = stage_image<GTAB>(smem, pool, refs[b.qimg], S);
    const QConst& q = *v.q;
    const int lane = (int)(threadIdx.x & 63u), wv = (int)uni32(threadIdx.x >> 6);
    const int T = st.n_cols, W = kNumFixed + T;
    const uint64_t qcols = uni64(q.colmask);
    for (int i = wv; i < b.count; i += kTermsWaves) {  // wave-uniform
        const int p = (int)uni32((uint32_t)slots[b.begin + i]);
        const size_t o = (size_t)(b.out + i);
        double* row = terms + o * (size_t)W;
        if (p < 0) {  // no such candidate: NaN, nothing present, the row all 0.0
            if (lane == 0) head[o] = pf_pair_terms_head{__int_as_float(0x7FC00000), 0u, 0ull};
            if (lane < kNumFixed) row[lane] = 0.0;
            if (lane < T) row[kNumFixed + lane] = 0.0;
            continue;
        }
        const uint4 h0 = st.hdr0[p], h1 = st.hdr1[p], h2 = st.hdr2[p];
        const uint64_t ro = st.row_off[p];
        const uint32_t nc = uni32(h2.y), nf = uni32(h2.z), ntok = uni32(h2.w), nset = nc + nf;
        const uint32_t len = nset + (PACKED ? ntok : 2u * ntok);
        const uint32_t* wl = reinterpret_cast<const uint32_t*>(st.rows + ro);
        const double* norms = reinterpret_cast<const double*>(st.rows + ro + ((len + 3u) >> 2));
        // clubs, then friends: the candidate's words the query has too, counted with duplicates
        uint32_t ic = 0, ifr = 0;
        for (uint32_t j0 = 0; j0 < nset; j0 += 64u) {
            const uint32_t j = j0 + (uint32_t)lane;
            bool hit = false;
            if (j < nset) {
                const uint32_t w = wl[j];
                if (PACKED) hit = probe_p(v, w) != 0u;
                else hit = probe(v, j < nc ? 0u : (1u << v.lg), v.lg, w) != kEmptyVal;
            }
            ic += (uint32_t)__popcll(__ballot(hit && j < nc));
            ifr += (uint32_t)__popcll(__ballot(hit && j >= nc));
        }
        // tokens (grouped by column ascending, ascending tid within one): every lane accumulates the
        // current column's dot in record order, and the column's lane keeps it when the column ends
        int cur = -1;
        double dot = 0.0, mydot = 0.0;
        bool myhas = false;
        for (uint32_t i0 = 0; i0 < ntok; i0 += 64u) {
            const uint32_t k = i0 + (uint32_t)lane;
            uint32_t col = 0;
            double pr = 0.0;
            bool hit = false;
            if (k < ntok) {
                if (PACKED) {
                    const uint32_t w = wl[nset + k];
                    const uint32_t val = probe_p(v, kTagTok | (w & 0xFFFFFFu));
                    col = (w >> kTidBits) & 63u;
                    hit = val != 0u;
                    if (hit) pr = hit_product(v, val & kTidMask, (int32_t)(w >> 24));
                } else {
                    const uint32_t key = wl[nset + 2u * k], w = wl[nset + 2u * k + 1u];
                    const uint32_t val = probe(v, 2u << v.lg, v.lg, key);
                    col = w & 0xFFu;
                    hit = val != kEmptyVal && (val & 0xFFu) == col;
                    if (hit) pr = hit_product(v, val >> 8, (int32_t)w >> 8);
                }
            }
            uint64_t hm = __ballot(hit);
            while (hm) {  // the hits in record order
                const int x = __ffsll((unsigned long long)hm) - 1;
                hm &= hm - 1ull;
                const int cx = __shfl((int)col, x);
                const double px = __shfl(pr, x);
                if (cx != cur) {
                    if (lane == cur) { mydot = dot; myhas = true; }
                    cur = cx;
                    dot = 0.0;
                }
                dot += px;
            }
        }
        if (lane == cur) { mydot = dot; myhas = true; }
        // lane t: column t's term where both sides have the column (s = 0 without a shared token)
        const uint64_t cmask = uni64((uint64_t)h0.x | ((uint64_t)h0.y << 32));
        const uint64_t common = qcols & cmask;
        double tterm = 0.0;
        if ((common >> lane) & 1ull) {
            if (myhas && mydot != 0.0) tterm = text_term(q, lane, mydot, norms[__popcll(cmask & ((1ull << lane) - 1ull))]);
            else tterm = q.sig0_col[lane];
        }
        // the seven fixed terms, by every lane alike; lane s keeps slot s
        uint32_t fmask = 0;
        double fterm = 0.0;
        auto put = [&](int slot, double term) {
            fmask |= 1u << slot;
            if (lane == slot) fterm = term;
        };
        header_terms_each(q, h2.x & 0xFFu, (h2.x >> 8) & 0xFFu, (int)h0.z, (int)h0.w, (int)h1.x, (int)h1.y, (int)h1.z, put);
        set_terms_each(q, (int)ic, nc, (int)ifr, nf, put);
        fmask = uni32(fmask);
        // the reference's sum: the present slots ascending
        double sum = 0.0;
#pragma unroll
        for (int s = 0; s < kNumFixed; ++s) {
            const double t = __shfl(fterm, s);
            if ((fmask >> s) & 1u) sum += t;
        }
        for (uint64_t cm = common; cm; cm &= cm - 1ull) sum += __shfl(tterm, __ffsll((unsigned long long)cm) - 1);
        const int used = __popc(fmask) + __popcll(common);
        const float score = fas_score(sum, used, (double)used / (double)(kNumFixed + q.n_cols));
        if (lane == 0) head[o] = pf_pair_terms_head{score, fmask, common};
        if (lane < kNumFixed) row[lane] = fterm;
        if (lane < T) row[kNumFixed + lane] = tterm;
    }
}

// the instantiation a launch's run-time choice names (pf_kernels.h)
using TermsKernel = decltype(&fas_terms_kernel<false, false>);
static TermsKernel terms_kernel(bool packed, bool gtab) {
    static constexpr TermsKernel tab[2][2] = {{fas_terms_kernel<false, false>, fas_terms_kernel<false, true>},
                                              {fas_terms_kernel<true, false>, fas_terms_kernel<true, true>}};
    return tab[packed][gtab];
}

hipError_t launch_terms(const TermsLaunch& L) {
    if (L.nblocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(terms_kernel(L.st.packed, L.gtab), dim3(L.nblocks), dim3(kTermsThreads), L.lds, L.s, L.st, L.pool,
                       L.refs_dev, L.blocks, L.slots, L.head, L.terms, L.sel);
    return hipGetLastError();
}

}  // namespace pf
