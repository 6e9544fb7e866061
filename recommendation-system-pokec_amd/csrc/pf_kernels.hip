// pf_kernels.hip — gfx950 kernels of the FAS engine.
//
//   fas_scan_kernel   K1   all-candidates FAS (A13) over a tile range, one query per
//                          blockIdx.y, fused per-wave / per-block top-k (K2a)
//   topk_merge_kernel K2b  per-query merge of per-block (or per-GPU) key lists
//   fas_pairs_kernel  K1'  FAS for explicit (query, candidate) pairs (A10/A12/A14/A15)
//
// One lane owns one candidate (64 candidates = one tile per wave).  Records are stored
// tile-interleaved, so each 16-B step of a wave is one coalesced 1 KiB load.  The walk
// over a record is branch-free: a word's kind follows from its position (clubs, friends,
// then self-describing packed tokens), and every word costs one 2-choice cuckoo probe
// of the query's LDS hash (clubs, friends, (column, token) weights, exclusions).  Only
// a token hit (rare) leaves the uniform path: its product is appended to a per-lane
// LDS list of column dot products.  All sigmoid work and the reference's summation
// order (recommender_similarity.cpp:38-113: public, gender, completion, age, region,
// clubs, friends, columns ascending) live in a per-candidate epilogue.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <unordered_map>
#include <vector>
#include <cstdio>
#include <cstdlib>

#include "pf_device.h"
#include "pf_filter.h"
#include "pf_kernels.h"
#include "pf_plan.h"
#include "pf_prune.h"
#include "pf_select.h"

namespace pf {

static_assert(sizeof(QConst) % 16 == 0, "QConst must keep the LDS carve 16-B aligned");
static_assert(sizeof(QVal) == 16, "QVal is one 16-B load");

#ifdef PF_K5_TIMERS
// profiling build only (make K5T=1): per-phase clock64() sums over every wave (K5: launch_post,
// K1': launch_pairs print them every 10th launch)
__device__ unsigned long long g_k5t[16];
// K1': staging, walk, epilogue, total, dense, assembly, overflow, waves, fas, then the epilogue's
// waves past the item queue (per-lane fallback), items, epilogue waves
__device__ unsigned long long g_k1t[12];
#endif

// K5 pruning counters (mode bit 17, PF_DEBUG k5_prune_stats=1; k5_prune_stats_read): candidates
// seen, dropped at a block's start, dropped at a round's end, blocks, blocks begun without a threshold
constexpr int kPruneStats = 5;
static_assert(kPruneBins <= (int)(sizeof(ScanSync::hist) / sizeof(unsigned int)), "the histogram holds every bin");
__device__ unsigned long long g_k5_prune[kPruneStats];

#ifdef PF_K5_BLOCKLOG
// profiling build only (tools/build_variant.sh blog XFLAGS=-DPF_K5_BLOCKLOG): K5's per-block start /
// end times (s_memrealtime, 100 MHz, one clock for every CU), summarised by launch_post
constexpr unsigned kBlogCap = 16384;
__device__ unsigned long long g_blog_t[2 * kBlogCap];
__device__ unsigned int g_blog_meta[kBlogCap];
__device__ unsigned int g_blog_n;
#endif

// Orders a wave's LDS accesses across its lanes (LDS serves a wave's operations in order;
// this keeps the compiler from moving accesses across the point).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Per-lane record walk state
struct Walk {
    uint32_t cnt;        // clubs intersections (low 16 bits) + friends intersections << 16
    uint32_t nh;         // token hits seen (entries beyond kHitCap are not stored)
    uint32_t pend;       // wide tokens: tid word waiting for its (tf, col) word
};

// A token hit is stored as its T2 val plus the candidate's tf:
//   packed: one word  vi | col << 18 | tf << 24        (the walk's only LDS write)
//   wide:   two words {col | vi << 8, tf << 8 | col}; the record's token words are
//           {tid | col << 26, tf << 8 | col}, the first being the table key
template <bool PACKED>
struct HitT;
template <>
struct HitT<true> {
    using type = uint32_t;
    __device__ static uint32_t col(type e) { return (e >> kTidBits) & 63u; }
    __device__ static uint32_t vi(type e) { return e & kTidMask; }
    __device__ static int32_t tf(type e) { return (int32_t)(e >> 24); }
};
template <>
struct HitT<false> {
    using type = uint2;
    __device__ static uint32_t col(type e) { return e.x & 0xFFu; }
    __device__ static uint32_t vi(type e) { return e.x >> 8; }
    __device__ static int32_t tf(type e) { return (int32_t)e.y >> 8; }
};

// One 16-B step (4 record words) of a lane, branch-free.  All four probes are issued
// before any result is used, so the step's 8 LDS reads are in flight together; then the
// words update the counters in order.  Every word costs one (possibly dead) hit-list
// store: a non-hit writes the lane's next free slot, which the next real hit
// overwrites; hits past kHitCap go to a dump slot (the list then reads as overflowed
// and the epilogue re-walks the record).
//
// Packed corpora: one tagged table, so a word's probe key is the word itself (sets) or
// kTagTok | its low 24 bits (tokens), and the probe's value is directly the club / friend
// counter increment or the token's value entry.  sj = the step's first word index in the
// chunk (wave-uniform), tb = nset - j0 = where the chunk's tokens start, lim = chunk
// length (MASKED only: lanes of different tiles, whose padding is not guaranteed).
template <bool MASKED>
__device__ __forceinline__ void walk_step_p(Walk& W, const uint4& cw, int sj, int tb, int lim, const QView& v,
                                            uint32_t hstride) {
    const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
    uint32_t val[4];
    bool tok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tok[i] = sj + i >= tb;
        uint32_t key = tok[i] ? (kTagTok | (w[i] & 0xFFFFFFu)) : w[i];
        if (MASKED) key = sj + i < lim ? key : kPadWord;
        val[i] = probe_p(v, key);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        W.cnt += tok[i] ? 0u : val[i];
        const uint32_t slot = (W.nh < kHitCap ? W.nh : kHitCap) * hstride + threadIdx.x;
        reinterpret_cast<uint32_t*>(v.hits)[slot] = (w[i] & 0xFF000000u) | (val[i] & 0xFFFFFFu);
        W.nh += (tok[i] && val[i] != 0u) ? 1u : 0u;
    }
}

// Wide corpora: three tables, token (tid, tf:col) word pairs probed at the second word.
__device__ __forceinline__ void walk_step_w(Walk& W, const uint4& cw, uint32_t j0, uint32_t nc, uint32_t nset,
                                            uint32_t len, const QView& v, uint32_t hstride) {
    const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
    uint32_t val[4];
    bool tok[4], fr[4], second[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t j = j0 + i;
        tok[i] = j >= nset;
        fr[i] = j >= nc;
        const uint32_t off = ((uint32_t)fr[i] + (uint32_t)tok[i]) << v.lg;  // T0 clubs, T1 friends, T2 tokens
        second[i] = tok[i] && ((j - nset) & 1u);
        const uint32_t key = second[i] ? (i ? w[i - 1] : W.pend) : w[i];
        val[i] = probe(v, off, v.lg, key);
    }
    W.pend = w[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t j = j0 + i;
        const bool ok = j < len;
        const bool hit = ok && (!tok[i] || second[i]) && val[i] != kEmptyVal &&
                         (!tok[i] || (val[i] & 0xFFu) == (w[i] & 0xFFu));
        W.cnt += (hit && !tok[i]) ? (fr[i] ? 0x10000u : 1u) : 0u;
        const uint32_t slot = (W.nh < kHitCap ? W.nh : kHitCap) * hstride + threadIdx.x;
        reinterpret_cast<uint2*>(v.hits)[slot] = make_uint2(val[i], w[i]);
        W.nh += (hit && tok[i]) ? 1u : 0u;
    }
}

// A candidate's record and column norms as the epilogue reads them: word j of the record, and
// sqrt(sum w_B^2) of column t (cmask = its non-empty columns).
//   TileRec: the tile store (K1, the record-stream scan): words interleaved per tile, norms in
//            the tile's [candidate][rank] block (two dependent loads);
//   RowRec:  the row store (K1', pairs): the record contiguous, its norms right after it.
struct TileRec {
    const DevStore* st;
    Loc l;
    uint32_t qw;
    __device__ uint32_t word(uint32_t j) const { return word_at(*st, l, qw, j); }
    __device__ double norm(uint64_t cmask, int t) const { return col_norm(*st, l, cmask, t); }
};
struct RowRec {
    const uint32_t* w;
    const double* n;
    __device__ uint32_t word(uint32_t j) const { return w[j]; }
    __device__ double norm(uint64_t cmask, int t) const { return n[__popcll(cmask & ((1ull << t) - 1ull))]; }
};

// Text terms of a candidate whose hit list overflowed: re-walk its token words from
// global memory, accumulating each column's dot in stream order (rare path).
template <bool PACKED, class Rec>
__device__ __forceinline__ double text_terms_slow(const QView& v, const Rec& rec, uint32_t nset, uint32_t len,
                                                  uint64_t cmask, double sum) {
    const QConst& q = *v.q;
    const uint32_t cap = 1u << v.lg;
    int cur = -1;
    double dot = 0.0;
    auto close = [&]() {
        if (cur >= 0 && ((q.colmask >> cur) & 1ull))
            sum += dot == 0.0 ? q.sig0_col[cur] : text_term(q, cur, dot, rec.norm(cmask, cur));
    };
    for (uint32_t j = nset; j < len; j += PACKED ? 1 : 2) {
        uint32_t key, col, val;
        int32_t tf;
        if (PACKED) {
            const uint32_t w = rec.word(j);
            key = kTagTok | (w & 0xFFFFFFu);
            col = (w >> kTidBits) & 63u;
            tf = (int32_t)(w >> 24);
            val = probe_p(v, key);
            if (val == 0u) val = kEmptyVal;
        } else {
            const uint32_t w = rec.word(j + 1);
            key = rec.word(j);
            col = w & 0xFFu;
            tf = (int32_t)w >> 8;
            val = probe(v, 2u * cap, v.lg, key);
            if (val != kEmptyVal && (val & 0xFFu) != col) val = kEmptyVal;
        }
        if ((int)col != cur) {
            close();
            cur = (int)col;
            dot = 0.0;
        }
        if (val != kEmptyVal) dot += hit_product(v, PACKED ? (val & kTidMask) : (val >> 8), tf);
    }
    close();
    return sum;
}

// The same for a record in the row store (the pair kernel's overflowed hit lists): the token
// words in 16-B steps, four steps in flight (a lane alone walks its record here, so the
// loads' latency is the cost).
__device__ __forceinline__ double text_terms_row(const QView& v, const uint4* base, const double* norms, uint32_t nset,
                                              uint32_t len, uint64_t cmask, double sum) {
    const QConst& q = *v.q;
    int cur = -1;
    double dot = 0.0;
    auto close = [&]() {
        if (cur >= 0 && ((q.colmask >> cur) & 1ull))
            sum += dot == 0.0 ? q.sig0_col[cur]
                              : text_term(q, cur, dot, norms[__popcll(cmask & ((1ull << cur) - 1ull))]);
    };
    const uint32_t steps = (len + 3) >> 2, s0 = nset >> 2;
    if (len <= nset) return sum;
    auto ld = [&](uint32_t s) { return base[s < steps ? s : steps - 1]; };
    uint4 r0 = ld(s0), r1 = ld(s0 + 1), r2 = ld(s0 + 2), r3 = ld(s0 + 3);
    for (uint32_t s = s0; s < steps; ++s) {
        const uint4 cw = r0;
        r0 = r1; r1 = r2; r2 = r3;
        r3 = ld(s + 4);
        const uint32_t w4[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t j = 4 * s + (uint32_t)i;
            if (j < nset || j >= len) continue;
            const uint32_t w = w4[i];
            const int col = (int)((w >> kTidBits) & 63u);
            if (col != cur) {
                close();
                cur = col;
                dot = 0.0;
            }
            const uint32_t val = probe_p(v, kTagTok | (w & 0xFFFFFFu));
            if (val != 0u) dot += hit_product(v, val & kTidMask, (int32_t)(w >> 24));
        }
    }
    close();
    return sum;
}

// Walk record words [j0, j0 + clen) of the lane's chunk; base = the lane's stream column
// (step s at base[s * kTileSlots]).  Every lane of the wave calls it (clen = 0 when idle).
// Double buffer of 4-step groups: the next group's 4 loads are issued before the current
// group is walked, so every wait is covered by a whole group of work.  (Loads kept in
// flight across the loop back-edge make the waitcnt pass drain them at the loop head.)
// MASKED = false (scan): every lane of the wave is in one tile, whose steps come in whole
// groups with padding words past each chunk, and the stream ends with a group of
// padding, so loads need no clamp and words no mask.  MASKED = true (pairs): lanes of
// different tiles; loads are clamped to the lane's last step and words past the chunk
// are masked.
// STRIDE: uint4 distance between a lane's successive steps (kTileSlots in the tile stream,
// 1 in the row store).
template <bool PACKED, bool MASKED, int STRIDE = kTileSlots>
__device__ __forceinline__ void walk_chunk(Walk& W, const uint4* base, uint32_t j0, uint32_t clen, uint32_t nc,
                                           uint32_t nset, const QView& v, uint32_t hstride) {
    const uint32_t steps = (clen + 3) >> 2;
    const uint32_t smax = wave_max_u32(steps);
    const uint32_t last = steps ? steps - 1 : 0;
    auto ld = [&](uint32_t s) { return base[(size_t)(MASKED ? (s < last ? s : last) : s) * STRIDE]; };
    const int tb = (int)nset - (int)j0, lim = (int)clen;
    const uint32_t len = j0 + clen;
    auto walk = [&](const uint4& c, uint32_t s) {
        if (PACKED) walk_step_p<MASKED>(W, c, (int)s * 4, tb, lim, v, hstride);
        else walk_step_w(W, c, j0 + s * 4, nc, nset, len, v, hstride);
    };
    uint4 c0 = ld(0), c1 = ld(1), c2 = ld(2), c3 = ld(3);
    for (uint32_t s = 0; s < smax; s += 4) {
        const uint4 n0 = ld(s + 4), n1 = ld(s + 5), n2 = ld(s + 6), n3 = ld(s + 7);
        walk(c0, s);
        walk(c1, s + 1);
        walk(c2, s + 2);
        walk(c3, s + 3);
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
}

// FAS(A = staged query, B = slot p) from the walk's results: the reference's terms in the
// reference's order.  The candidate's token hits are the hit lists of threads
// first .. first + nl - 1 (its chunks, in record order); nh_of(g) = hits of thread first + g.
// RAW (packed only): the list holds the hit record words themselves (the pair walk), whose
// values are probed again here.
template <bool PACKED, bool RAW = false, class Rec, class NH>
__device__ __forceinline__ float fas_epilogue(const QView& v, const Rec& rec, const uint4& h0, const uint4& h1,
                                              const uint4& h2, uint32_t cnt, uint32_t first, uint32_t nl, NH nh_of,
                                              uint64_t* tep = nullptr) {
    static_assert(PACKED || !RAW, "raw hit words: packed corpora only");
    using H = HitT<PACKED>;
    const QConst& q = *v.q;
    const uint32_t hstride = blockDim.x;
    const uint32_t nc = h2.y, nf = h2.z;
    const uint64_t cmask = (uint64_t)h0.x | ((uint64_t)h0.y << 32);
    uint64_t common = q.colmask & cmask;
    bool overflow = false;
    for (uint32_t g = 0; g < nl; ++g) overflow |= nh_of(g) > kHitCap;
    // token hits of the chunks in order: (g, h) walks thread first + g's list
    const typename H::type* hits = reinterpret_cast<const typename H::type*>(v.hits);
    uint32_t g = 0, h = 0, nhg = overflow ? 0u : nh_of(0);
    typename H::type e{};
    auto next = [&]() -> bool {
        while (h >= nhg) {
            if (++g >= nl) return false;
            h = 0;
            nhg = nh_of(g);
        }
        e = hits[h * hstride + first + g];
        if constexpr (RAW) {
            const uint32_t w = (uint32_t)e;
            e = (w & 0xFF000000u) | (probe_p(v, kTagTok | (w & 0xFFFFFFu)) & 0xFFFFFFu);
        }
        ++h;
        return true;
    };
    bool have = next();
    // the first hit column's norm (global) is requested now and lands under the fixed terms
    double nrm = have ? rec.norm(cmask, (int)H::col(e)) : 0.0;

    double sum = 0.0;
    int used = 0;
    header_terms(q, h2.x & 0xFFu, (h2.x >> 8) & 0xFFu, (int)h0.z, (int)h0.w, (int)h1.x, (int)h1.y, (int)h1.z, sum, used);
    set_terms(q, (int)(cnt & 0xFFFFu), nc, (int)(cnt >> 16), nf, sum, used);
    used += __popcll(common);
    if (tep) tep[0] = clock64();
    if (!overflow) {
        // One pass in the reference's column order, driven by the HIT columns: the wave's
        // i-th iteration computes every lane's i-th hit column (the only place the
        // expensive term runs, so lanes stay aligned), after adding the s = 0 term of each
        // common column the lane skips on the way (cheap table reads).  The next hit
        // column's norm is requested before this column's term is computed.
        while (have) {
            const int t = (int)H::col(e);
            const double nrm_t = nrm;
            double dot = 0.0;
            while (have && (int)H::col(e) == t) {  // this column's hits, in stream (ascending tid) order
                dot += hit_product(v, H::vi(e), H::tf(e));
                have = next();
            }
            if (have) nrm = rec.norm(cmask, (int)H::col(e));
            // a hit column the query's colmask lacks is one a field selection (pf_select.h) left
            // out: the walk still finds its tokens in the table, and it gets no term
            if (!((common >> t) & 1ull)) continue;
            uint64_t below = common & ((1ull << t) - 1ull);
            common &= ~below & ~(1ull << t);
            while (below) {
                const int c = __ffsll((unsigned long long)below) - 1;
                below &= below - 1;
                sum += q.sig0_col[c];
            }
            sum += dot == 0.0 ? q.sig0_col[t] : text_term(q, t, dot, nrm_t);
        }
        while (common) {
            const int c = __ffsll((unsigned long long)common) - 1;
            common &= common - 1;
            sum += q.sig0_col[c];
        }
    } else if constexpr (RAW) {
        sum = text_terms_row(v, reinterpret_cast<const uint4*>(rec.w), rec.n, nc + nf, record_words(h2, true), cmask, sum);
    } else {
        sum = text_terms_slow<PACKED>(v, rec, nc + nf, record_words(h2, PACKED), cmask, sum);
    }
    if (tep) tep[1] = clock64();
    return fas_score(sum, used, (double)used / (double)(kNumFixed + q.n_cols));
}

// ---------------------------------------------------------------- K1' record walk (packed)
// A pair-kernel lane walks one candidate's contiguous row-store record against the staged
// query table.  The probe compares keys only (one 4-B read per cuckoo choice, the value is
// probed again for the few hits in the epilogue) and every word stores itself, the raw record
// word, at the lane's next hit slot, which only a token hit advances; so a token word costs
// its key, hash, two addresses, two reads, two compares and the slot pointer.  Groups of 4
// steps past every lane's last club / friend word take the token-only step (no set
// bookkeeping).  A lane past its record loads the padding line (kPadWord never matches, and
// build_store pads the record's last step with it), so no word needs a mask.
struct RowWalk {
    uint32_t cnt;  // clubs intersections (low 16 bits) + friends intersections << 16
    uint32_t ptr;  // the lane's next hit slot, hit list word index (slot * kPairThreads + lane)
};

__device__ __forceinline__ bool has_key(const QView& v, uint32_t key, uint32_t x) {
    // the table's keys (SoA: the packed table T is at entry offset 0, its keys in words [0, 2^lg))
    const uint32_t k1 = v.tab[cuckoo_h1(x, v.lg)];
    // cuckoo_h2 as one bit-field extract (the compiler emits a shift and a mask)
    const uint32_t k2 = v.tab[__builtin_amdgcn_ubfe(x, 32u - 2u * (uint32_t)v.lg, (uint32_t)v.lg)];
    return (k1 == key) | (k2 == key);
}

// words j0 .. j0 + 3; SETS: the step may hold club / friend words (j < nset; clubs j < nc)
template <bool SETS>
__device__ __forceinline__ void row_step(RowWalk& W, const uint4& cw, uint32_t j0, uint32_t nc, uint32_t nset,
                                         const QView& v, uint32_t pcap) {
    const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
    bool hit[4], tok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tok[i] = !SETS || j0 + i >= nset;
        const uint32_t key = tok[i] ? (kTagTok | (w[i] & 0xFFFFFFu)) : w[i];
        hit[i] = has_key(v, key, cuckoo_x(key, v.hmul));
    }
    uint32_t* hl = reinterpret_cast<uint32_t*>(v.hits);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (SETS) W.cnt += (hit[i] && !tok[i]) ? (j0 + i < nc ? 1u : 0x10000u) : 0u;
        hl[W.ptr] = w[i];
        W.ptr += (hit[i] && tok[i]) ? kPairThreads : 0u;
    }
    W.ptr = W.ptr < pcap ? W.ptr : pcap;  // <= 3 writes past pcap per step: the dump slots
}

__device__ __forceinline__ void walk_row(RowWalk& W, const uint4* base, const uint4* pad, uint32_t len, uint32_t nc,
                                         uint32_t nset, const QView& v, uint32_t pcap) {
    const uint32_t steps = (len + 3) >> 2;
    const uint32_t smax = wave_max_u32(steps);
    const uint32_t sset = wave_max_u32((nset + 3) >> 2);  // steps holding a set word on some lane
    auto ld = [&](uint32_t s) { return *(s < steps ? base + s : pad); };
    uint4 c0 = ld(0), c1 = ld(1), c2 = ld(2), c3 = ld(3);
    uint32_t s = 0;
    for (; s < sset; s += 4) {
        const uint4 n0 = ld(s + 4), n1 = ld(s + 5), n2 = ld(s + 6), n3 = ld(s + 7);
        row_step<true>(W, c0, 4 * s, nc, nset, v, pcap);
        row_step<true>(W, c1, 4 * s + 4, nc, nset, v, pcap);
        row_step<true>(W, c2, 4 * s + 8, nc, nset, v, pcap);
        row_step<true>(W, c3, 4 * s + 12, nc, nset, v, pcap);
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    for (; s < smax; s += 4) {
        const uint4 n0 = ld(s + 4), n1 = ld(s + 5), n2 = ld(s + 6), n3 = ld(s + 7);
        row_step<false>(W, c0, 0, 0, 0, v, pcap);
        row_step<false>(W, c1, 0, 0, 0, v, pcap);
        row_step<false>(W, c2, 0, 0, 0, v, pcap);
        row_step<false>(W, c3, 0, 0, 0, v, pcap);
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
}

// K1' epilogue, wave-dense (packed).  fas_epilogue's per-lane loop runs the expensive terms (two
// FP64 divisions and an exp per text column, a sqrt more per set term) once per hit column of
// the lane with the most, so a wave pays ~8 rounds for a mean of ~4 hit columns per pair.  Here
// every lane turns its hit words (held in registers) into items — one per hit column (its dot,
// in the record's ascending-tid order) and one per nonzero club / friend intersection — written
// as 16-B entries to a queue in the wave's strip of the (now consumed) hit lists; the wave then
// computes every item's term one per lane, and each lane adds its terms in the reference's order
// (public .. friends, then the common columns ascending, s = 0 terms between).  A wave whose
// items exceed its strip (320) takes fas_epilogue; overflowed hit lists take its record re-walk.
enum : uint32_t { kItemText = 0, kItemClubs = 1, kItemFriends = 2 };

// the candidate's column norm a text item needs (row store), 0 for a set item
__device__ __forceinline__ double item_norm(const DevStore& st, const uint4& it) {
    return (it.w >> 16) == kItemText ? reinterpret_cast<const double*>(st.rows + it.z)[(it.w >> 8) & 0xFFu] : 0.0;
}

__device__ __forceinline__ double item_term(const QConst& q, const uint4& it, double nrm) {
    const uint32_t kind = it.w >> 16;
    if (kind == kItemText) {
        const int t = (int)(it.w & 0xFFu);
        const double dot = __hiloint2double((int)it.y, (int)it.x);
        return dot == 0.0 ? q.sig0_col[t] : text_term(q, t, dot, nrm);
    }
    const bool cl = kind == kItemClubs;  // one inlined chain for both (a call here would spill the loop)
    return set_term_inl(q, cl ? PF_F_CLUBS : PF_F_FRIENDS, (int)it.x, (int)it.y, cl ? q.sqrt_clubs : q.sqrt_friends);
}

__device__ __forceinline__ float pair_epilogue(const QView& v, const DevStore& st, const RowRec& rec, uint64_t ro,
                                               uint32_t len, const uint4& h0, const uint4& h1, const uint4& h2,
                                               uint32_t cnt, uint32_t nh, bool active, uint64_t* tep) {
    const QConst& q = *v.q;
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const bool overflow = nh > kHitCap;
    uint32_t* hl = reinterpret_cast<uint32_t*>(v.hits);
    const uint32_t nhl = (active && !overflow) ? nh : 0u;
    // the hit words of the lane's LDS hit list (its own walk)
    uint32_t hw[kHitCap];
#pragma unroll
    for (int i = 0; i < (int)kHitCap; ++i) hw[i] = (uint32_t)i < nhl ? hl[i * kPairThreads + threadIdx.x] : 0u;
    auto colw = [](uint32_t w) { return (w >> kTidBits) & 63u; };
    // the query's columns (uniform: scalar registers).  A hit column not among them is one a field
    // selection (pf_select.h) left out: the walk still finds its tokens, and it gets no item
    // (each half through uint32_t: readfirstlane returns int, and bit 31 must not extend)
    const uint64_t qcm = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)q.colmask) |
                         ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(q.colmask >> 32)) << 32);
    uint32_t ncol = 0;
#pragma unroll
    for (int i = 0; i < (int)kHitCap; ++i)
        ncol += ((uint32_t)i < nhl && (i == 0 || colw(hw[i]) != colw(hw[i > 0 ? i - 1 : 0])) && ((qcm >> colw(hw[i])) & 1ull))
                    ? 1u : 0u;
    const uint32_t nc = h2.y, nf = h2.z;
    const int ic = (int)(cnt & 0xFFFFu), ifr = (int)(cnt >> 16);
    const bool dense = active && !overflow;
    const bool club_it = dense && q.n_clubs > 0 && nc > 0 && ic > 0;
    const bool fr_it = dense && q.n_friends > 0 && nf > 0 && ifr > 0;
    const uint32_t nit = dense ? ncol + (club_it ? 1u : 0u) + (fr_it ? 1u : 0u) : 0u;
    uint32_t x = nit;
    x = wave_incl_scan(x);
    const uint32_t base = x - nit, total = wave_last(x);
    constexpr uint32_t kQueue = kHitSlots * 64u / 4u;
    // A wave whose items exceed the queue takes two rounds: the lanes whose items end within it
    // (a prefix of the lanes) first, then the others from the queue's start; only a second round
    // past the queue too takes the per-lane epilogue (r3: 11 % of the waves needed two rounds)
    const uint32_t rnd = x > kQueue ? 1u : 0u;
    const uint64_t r1m = __ballot(rnd != 0u);
    const uint32_t total0 = r1m ? (uint32_t)__shfl((int)base, __ffsll((unsigned long long)r1m) - 1) : total;
    const uint32_t total1 = total - total0;
#ifdef PF_K5_TIMERS
    if (lane == 0) {
        atomicAdd(&g_k1t[9], total1 > kQueue ? 1ull : 0ull);
        atomicAdd(&g_k1t[10], (unsigned long long)total);
        atomicAdd(&g_k1t[11], 1ull);
    }
#endif
    if (total1 > kQueue) {  // (wave-uniform) the per-lane epilogue, hit lists intact
        if (!active) return 0.0f;
        return fas_epilogue<true, true>(v, rec, h0, h1, h2, cnt, threadIdx.x, 1u, [nh](uint32_t) { return nh; }, tep);
    }
    auto item = [&](uint32_t k) {  // 16-B entry k of the wave's strip (rows of 64 words)
        return reinterpret_cast<uint4*>(hl + ((4u * k) >> 6) * kPairThreads + (uint32_t)wv * 64u + ((4u * k) & 63u));
    };
    auto term_at = [&](uint32_t kk) {
        const uint4 it = *item(kk);
        return __hiloint2double((int)it.y, (int)it.x);
    };
    const uint64_t cmask = (uint64_t)h0.x | ((uint64_t)h0.y << 32);
    const uint32_t nbase = (uint32_t)(ro + ((len + 3u) >> 2));  // the record's column norms (uint4 index)
    // every active lane: the fixed terms (an overflowed lane computes its set terms itself)
    double sum = 0.0;
    int used = 0;
    header_terms(q, h2.x & 0xFFu, (h2.x >> 8) & 0xFFu, (int)h0.z, (int)h0.w, (int)h1.x, (int)h1.y, (int)h1.z, sum, used);
    const bool has_clubs = q.n_clubs > 0 && nc > 0, has_friends = q.n_friends > 0 && nf > 0;
    used += (has_clubs ? 1 : 0) + (has_friends ? 1 : 0);
    uint64_t common = q.colmask & cmask;
    used += __popcll(common);
    const uint32_t rbase = rnd ? base - total0 : base;  // the lane's first item in its round
    const uint32_t nrounds = r1m ? 2u : 1u;
#pragma unroll
    for (uint32_t r = 0; r < 2u; ++r) {
        if (r >= nrounds) break;
        const bool mine = rnd == r;
        wave_sync();  // every lane holds its hit words / the previous round is consumed: the strip is free
        if (mine && nit) {
            uint32_t k = rbase;
            if (club_it) *item(k++) = make_uint4((uint32_t)ic, nc, 0u, kItemClubs << 16);
            if (fr_it) *item(k++) = make_uint4((uint32_t)ifr, nf, 0u, kItemFriends << 16);
            double dot = 0.0;
#pragma unroll
            for (int i = 0; i < (int)kHitCap; ++i) {
                if ((uint32_t)i < nhl) {
                    const uint32_t w = hw[i], col = colw(w);
                    const uint32_t val = probe_p(v, kTagTok | (w & 0xFFFFFFu));
                    const bool first = i == 0 || col != colw(hw[i > 0 ? i - 1 : 0]);
                    dot = (first ? 0.0 : dot) + hit_product(v, val & kTidMask, (int32_t)(w >> 24));
                    const bool last = (uint32_t)(i + 1) == nhl || col != colw(hw[i + 1 < (int)kHitCap ? i + 1 : i]);
                    if (last && ((qcm >> col) & 1ull)) {
                        const uint32_t rank = (uint32_t)__popcll(cmask & ((1ull << col) - 1ull));
                        *item(k++) = make_uint4((uint32_t)__double2loint(dot), (uint32_t)__double2hiint(dot), nbase,
                                                (kItemText << 16) | (rank << 8) | col);
                    }
                }
            }
        }
        wave_sync();
        const uint32_t tr = r ? total1 : total0;
        for (uint32_t j = (uint32_t)lane; j < tr; j += 64u) {  // the round's terms, one per lane
            uint4 it = *item(j);
            const double term = item_term(q, it, item_norm(st, it));
            it.x = (uint32_t)__double2loint(term);
            it.y = (uint32_t)__double2hiint(term);
            *item(j) = it;
        }
        wave_sync();
        if (tep && r == 0) tep[0] = clock64();
        if (!mine) continue;
        // the lane's round: clubs, friends, then the common columns ascending (a hit column's term,
        // the items being in column order, else s = 0), recommender_similarity.cpp:80-113
        uint32_t kk = rbase;
        if (has_clubs)
            sum += ic == 0 ? q.sig0_clubs : (overflow ? set_term(q, PF_F_CLUBS, ic, (int)nc, q.sqrt_clubs) : term_at(kk++));
        if (has_friends)
            sum += ifr == 0 ? q.sig0_friends
                            : (overflow ? set_term(q, PF_F_FRIENDS, ifr, (int)nf, q.sqrt_friends) : term_at(kk++));
        if (active && !overflow) {
            // a uniform loop over the query's columns (scalar control, the s = 0 term a broadcast
            // read), adding where the candidate has the column too
            const uint32_t ke = rbase + nit;
            uint32_t nextc = kk < ke ? (item(kk)->w & 0xFFu) : 0xFFu;
            uint64_t qm = qcm;
            while (qm) {
                const uint32_t c = (uint32_t)__ffsll((unsigned long long)qm) - 1u;
                qm &= qm - 1ull;
                const double s0 = q.sig0_col[c];
                if ((common >> c) & 1ull) {
                    if (c == nextc) {
                        sum += term_at(kk++);
                        nextc = kk < ke ? (item(kk)->w & 0xFFu) : 0xFFu;
                    } else {
                        sum += s0;
                    }
                }
            }
        }
    }
    if (tep) tep[1] = clock64();
    // Overflowed hit lists (> kHitCap token hits, ~0.4 % of pairs, a quarter of the waves): the
    // wave walks each such record together, 64 words per round (one coalesced load), and
    // accumulates the hits' products in record order on every lane (the reference's per-column
    // dot order); lane t then computes column t's term, and the owner's sum takes the common
    // columns ascending.
    uint64_t ovm = __ballot(active && overflow);
    while (ovm) {
        const int l = __ffsll((unsigned long long)ovm) - 1;
        ovm &= ovm - 1ull;
        const uint64_t rol = (uint64_t)__shfl((long long)ro, l), cml = (uint64_t)__shfl((long long)cmask, l);
        const uint32_t lenl = (uint32_t)__shfl((int)len, l), nsetl = (uint32_t)__shfl((int)(nc + nf), l);
        const uint32_t* wl = reinterpret_cast<const uint32_t*>(st.rows + rol);
        int cur = -1;
        double dot = 0.0, mydot = 0.0;
        bool myhas = false;
        for (uint32_t b = nsetl; b < lenl; b += 64u) {
            const uint32_t j = b + (uint32_t)lane;
            const uint32_t w = j < lenl ? wl[j] : kPadWord;
            const uint32_t val = j < lenl ? probe_p(v, kTagTok | (w & 0xFFFFFFu)) : 0u;
            const double pr = val != 0u ? hit_product(v, val & kTidMask, (int32_t)(w >> 24)) : 0.0;
            uint64_t hm = __ballot(val != 0u);
            while (hm) {  // the hits in record order
                const int x = __ffsll((unsigned long long)hm) - 1;
                hm &= hm - 1ull;
                const int cx = (int)(((uint32_t)__shfl((int)w, x) >> kTidBits) & 63u);
                const double px = __shfl(pr, x);
                if (cx != cur) {
                    if (cur >= 0 && lane == cur) { mydot = dot; myhas = true; }
                    cur = cx;
                    dot = 0.0;
                }
                dot += px;
            }
        }
        if (cur >= 0 && lane == cur) { mydot = dot; myhas = true; }
        double term = 0.0;
        if (myhas) {
            const double nrm = reinterpret_cast<const double*>(st.rows + rol + ((lenl + 3u) >> 2))
                [__popcll(cml & ((1ull << lane) - 1ull))];
            term = mydot == 0.0 ? q.sig0_col[lane] : text_term(q, lane, mydot, nrm);
        }
        const uint64_t hasm = __ballot(myhas);
        uint64_t cm = q.colmask & cml;
        double sl = __shfl(sum, l);
        while (cm) {
            const int c = __ffsll((unsigned long long)cm) - 1;
            cm &= cm - 1ull;
            const double tc = __shfl(term, c);
            sl += ((hasm >> c) & 1ull) ? tc : q.sig0_col[c];
        }
        if (lane == l) sum = sl;
    }
    if (tep) tep[2] = clock64();
    if (!active) return 0.0f;
    return fas_score(sum, used, (double)used / (double)(kNumFixed + q.n_cols));
}

// FAS of slot p by one lane alone (pairs kernel): the lane walks the slot's record in the row
// store (contiguous 16-B steps, so the lane's loads consume whole cache lines), its own hit list
// then holds the whole record's hits in order; the column norms follow the record in the row
// store, so no tile lookup sits in front of them.
// A pair candidate's headers and row offset, loaded before the block stages its image (the loads
// are in flight across the staging round trip and its barrier)
struct PairHdr {
    uint4 h0, h1, h2;
    uint64_t ro;
};
__device__ __forceinline__ PairHdr load_pair_hdr(const DevStore& st, int p, bool active) {
    PairHdr H;
    H.h0 = H.h1 = H.h2 = make_uint4(0, 0, 0, 0);
    H.ro = 0;
    if (active) {
        H.h0 = st.hdr0[p];
        H.h1 = st.hdr1[p];
        H.h2 = st.hdr2[p];
        H.ro = st.row_off[p];
    }
    return H;
}

template <bool PACKED>
__device__ __forceinline__ float fas_slot(const DevStore& st, const QView& v, const PairHdr& H, bool active,
                                          uint64_t* twalk = nullptr) {
    const uint4 h0 = H.h0, h1 = H.h1, h2 = H.h2;
    const uint64_t ro = H.ro;
    const uint32_t nc = h2.y, nset = h2.y + h2.z;
    const uint32_t len = active ? record_words(h2, PACKED) : 0u;
    const RowRec rec{reinterpret_cast<const uint32_t*>(st.rows + ro),
                     reinterpret_cast<const double*>(st.rows + ro + ((len + 3) >> 2))};
    if constexpr (PACKED) {
        const uint32_t pcap = kHitCap * kPairThreads + threadIdx.x;
        RowWalk W{0u, threadIdx.x};
        walk_row(W, st.rows + ro, st.row_pad, len, nc, active ? nset : 0u, v, pcap);
        if (twalk) twalk[0] = clock64();
        // a list that reached kHitCap reads as overflowed (the slow path re-walks the record)
        const uint32_t nh = W.ptr >= pcap ? kHitCap + 1 : (W.ptr - threadIdx.x) / kPairThreads;
        return pair_epilogue(v, st, rec, ro, len, h0, h1, h2, W.cnt, nh, active, twalk ? twalk + 1 : nullptr);
    } else {
        Walk W;
        W.cnt = 0; W.nh = 0; W.pend = 0;
        walk_chunk<false, true, 1>(W, st.rows + ro, 0u, len, nc, nset, v, kPairThreads);
        if (!active) return 0.0f;
        const uint32_t nh = W.nh;
        return fas_epilogue<false>(v, rec, h0, h1, h2, W.cnt, threadIdx.x, 1u, [&](uint32_t) { return nh; });
    }
}

// ---------------------------------------------------------------- LDS staging
// (the copies: stage, stage4 in pf_device.h)
// LDS carve: [QConst][tables][vals][hit lists kHitCap x blockDim][merge scratch 2 KiB].
// GTAB = false: the cuckoo table and the token values are staged in LDS, so every probe
// is a ds_read (pointer provenance is the LDS symbol only, never merged with a global
// pointer: a merged pointer would compile to flat loads, whose waits also drain the
// HBM prefetch).  GTAB = true (query too large for LDS): probes read global memory.
template <bool GTAB>
__device__ __forceinline__ QView stage_query(char* smem, const uint8_t* pool, const QImageRef& r, char** scratch,
                                             const FieldSel& S) {
    if constexpr (!GTAB) {
        // the sizes from the image in global memory; QConst | tables | values are contiguous in
        // every image pool (tables of >= 2^4 8-B entries keep the values 16-B aligned)
        const uint8_t* base = pool + (size_t)r.const_off * 16u;
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
        stage(smem, pool + (size_t)r.const_off * 16u, sizeof(QConst));
    }
    __syncthreads();
    // a field selection (pf_select.h; uniform, on == 0: none) patches the staged copy of the
    // constants, never the image: the fixed terms, the common columns and the denominator follow
    if (S.on != 0u) {
        if (threadIdx.x == 0) select_apply(*reinterpret_cast<QConst*>(smem), S);
        __syncthreads();
    }
    const QConst* q = reinterpret_cast<const QConst*>(smem);
    // the image's sizes are workgroup-uniform: read into SGPRs (as LDS loads they would sit in a
    // VGPR each for the whole kernel, and the walk loops are register-bound)
    auto uni = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
    QView v;
    v.q = q;
    v.lg = (int)uni((uint32_t)q->lg);
    v.lge = (int)uni((uint32_t)q->lg_excl);
    v.hmul = uni(q->hmul);
    v.excl_off = uni(q->excl_off);
    const uint32_t kb = 8u * (v.excl_off + (1u << v.lge)), vb = uni((uint32_t)q->n_vals) * 16u;
    char* p = smem + sizeof(QConst);
    if constexpr (!GTAB) {
        v.tab = reinterpret_cast<const uint32_t*>(p);
        v.vals = reinterpret_cast<const QVal*>(p + kb);
        p += kb + vb;
    } else {
        v.tab = reinterpret_cast<const uint32_t*>(pool + (size_t)r.const_off * 16u + r.keys_off);
        v.vals = reinterpret_cast<const QVal*>(pool + (size_t)r.const_off * 16u + r.vals_off);
    }
    v.hits = p;
    p += (size_t)uni(q->n_hits_max) * blockDim.x;  // n_hits_max = bytes per lane of the hit list
    v.nh = reinterpret_cast<uint32_t*>(p);     // per-thread hit counts (split records)
    p += 4u * blockDim.x;
    *scratch = p;
    return v;
}

// ---------------------------------------------------------------- K1: scan
// write-through store / L1-bypassing load of a word handed between workgroups of a launch
__device__ __forceinline__ void st_agent(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_agent(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the low n bits
__device__ __forceinline__ uint64_t low_bits(uint32_t n) { return n >= 64u ? ~0ull : ((1ull << n) - 1ull); }

// The k smallest keys of nl ascending k-lists (list w at at(w), read with L1-bypassing loads), ascending
// in lanes < k, by one wave.  Any k distinct keys of the lists bound the k-th smallest from above:
// t0 = the smaller of the k-th smallest list head (when there are >= k lists: a wave sort of each
// lane's smallest head) and the smallest k-th key of a list.  Only keys <= t0 are gathered, into buf
// (LDS, 64 keys) while they fit, and sorted once; a list is read only down to its first key past t0.
// (The k-th keys alone bound it loosely: ~450 of a cfg-2 XCD group's 1,280 keys pass.)  More than 64
// such keys take the push path.  The 128 lists of a one-query launch's XCD group went through five
// 64-key sort-and-merge pushes per wave before.
template <class At>
__device__ __forceinline__ uint64_t merge_lists(At at, int nl, int k, uint64_t* buf, int lane) {
    uint64_t tk = ~0ull, hd = ~0ull;
    for (int w = lane; w < nl; w += 64) {
        const uint64_t x = ld_agent(at(w) + k - 1), h = ld_agent(at(w));
        tk = x < tk ? x : tk;
        hd = h < hd ? h : hd;
    }
    uint64_t t0 = wave_min64(tk);
    if (nl >= k) {
        const uint64_t th = rdlane64(wave_sort64(hd, lane), k - 1);
        t0 = th < t0 ? th : t0;
    }
    uint32_t ns = 0;
    for (int w0 = 0; w0 < nl; w0 += 64) {
        const int w = w0 + lane;
        const uint64_t* L = at(min(w, nl - 1));
        for (int e0 = 0; e0 < k; e0 += 4) {
            uint64_t x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = (w < nl && e0 + u < k) ? ld_agent(L + e0 + u) : ~0ull;
            bool more = false;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool in = x[u] <= t0 && x[u] != ~0ull;
                const uint64_t m = __ballot(in);
                const uint32_t pos = ns + (uint32_t)__popcll(m & low_bits((uint32_t)lane));
                if (in && pos < 64u) buf[pos] = x[u];
                ns += (uint32_t)__popcll(m);
                more = in;  // the batch's last key in range: the list may hold more below t0
            }
            if (!__ballot(more)) break;  // ascending lists: nothing further down is <= t0
        }
    }
    if (ns <= 64u) return wave_sort64(lane < (int)ns ? buf[lane] : ~0ull, lane);
    uint64_t acc = ~0ull;
    for (int w0 = 0; w0 < nl; w0 += 64) {
        const int w = w0 + lane;
        const uint64_t* L = at(min(w, nl - 1));
        for (int e = 0; e < k; ++e) {
            const uint64_t x = w < nl ? ld_agent(L + e) : ~0ull;
            const bool in = x <= t0 && x != ~0ull;
            if (!__ballot(in)) break;
            topk_push(acc, in ? x : ~0ull, k, lane);
        }
    }
    return acc;
}

// The scans' (K5, K1) fused cross-block merge, in two levels.  The workgroups of group g = bx mod 8 (with the
// round-robin dispatch, the workgroups of one XCD) publish their k-lists and take a ticket on the
// group's counter; the group's last workgroup merges the group's lists into slot nbx + g and takes
// a ticket on the query's counter; the last of those merges the <= 8 group lists into out[row].
// Each counter sees ~nbx / 8 tickets: with one counter for all 1,024 workgroups of a one-query
// launch the tail cost ~15 us of a 185 us launch (r4n, a no-merge build).  After the workgroup's
// own list only wave 0 runs: no barrier on the launch's critical path past the last block.
// parts: per query (nbx + 8) lists of k keys.  sc: LDS for max(nw * k, 64) keys.  Hand-offs
// (pf_device.h take_ticket): a list is published with write-through stores drained before the
// ticket and read with L1-bypassing loads after it.
// counted (a window with PF_WIN_COUNT, pf_window.h): wcnt is the wave's share of the candidates in the
// window (K5: the workgroup's, in wave 0).  Its add to the query's count word has returned before the
// barrier below, hence before the workgroup's ticket, as the last block's histogram record has; the
// final merger reads the word after the last ticket and writes it to totals[row] before it zeroes the
// struct.  A launch that does not count passes false and is the code it was.
// The collector's append (a launch with kWinCollect, pf_window.h), by a whole wave at a keying point:
// a ballot of the lanes whose key is in the window, one returning relaxed agent-scope add of its
// popcount to the query's cursor word by the first lane, the base broadcast, and each in-window lane's
// key stored at base + its rank among the ballot, only below cap: plain vector stores, none past the
// buffer however many match.  A wave with no match issues nothing.  The add has returned before the
// stores, hence before the workgroup's ticket and the final merger's zeroing of the word.  K5 calls
// it with its block's two keys per lane under one add (key1; ~0 elsewhere).
__device__ __forceinline__ void collect_append(uint64_t key0, uint64_t key1, unsigned int* cursor,
                                               uint64_t* __restrict__ cbuf, uint32_t ccap, int lane) {
    const uint64_t b0 = __ballot(key0 != ~0ull), b1 = __ballot(key1 != ~0ull);
    if ((b0 | b1) == 0ull) return;
    const uint32_t n0 = (uint32_t)__popcll(b0), n1 = (uint32_t)__popcll(b1);
    uint32_t base = 0u;
    if (lane == 0) base = __hip_atomic_fetch_add(cursor, n0 + n1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    const uint64_t below = (1ull << lane) - 1ull;
    if (key0 != ~0ull) {
        const uint32_t at = base + (uint32_t)__popcll(b0 & below);
        if (at < ccap) cbuf[at] = key0;
    }
    if (key1 != ~0ull) {
        const uint32_t at = base + n0 + (uint32_t)__popcll(b1 & below);
        if (at < ccap) cbuf[at] = key1;
    }
}

__device__ __forceinline__ void post_tail(uint64_t list, int k, uint64_t* sc, ScanSync* __restrict__ sync,
                                          uint64_t* __restrict__ parts, uint64_t* __restrict__ out,
                                          const int32_t* __restrict__ out_rows, int qy, int bx, int nbx,
                                          bool counted = false, uint32_t wcnt = 0u, uint32_t* __restrict__ totals = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    if (counted && lane == 0 && wcnt != 0u) {
        const uint32_t old = __hip_atomic_fetch_add(&sync[qy].wcount, wcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::"v"(old));
    }
    __syncthreads();
    if (lane < k) sc[wave * k + lane] = list;
    __syncthreads();
    if (wave != 0) return;
    ScanSync* sy = sync + qy;
    uint64_t* qparts = parts + (size_t)qy * (nbx + 8) * k;
    const int ng = min(8, nbx), g = bx % ng, n_g = (nbx - g + ng - 1) / ng;
    uint64_t acc;
    {  // the workgroup's list: its waves' lists (one sort when they fit a wave)
        const int n = nw * k;
        if (n <= 64) {
            acc = wave_sort64(lane < n ? sc[lane] : ~0ull, lane);
        } else {
            acc = ~0ull;
            for (int b = 0; b < n; b += 64) topk_push(acc, b + lane < n ? sc[b + lane] : ~0ull, k, lane);
        }
    }
    if (lane < k) st_agent(qparts + (size_t)bx * k + lane, acc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __atomic_signal_fence(__ATOMIC_SEQ_CST);  // program order: stores, wait, ticket
    unsigned t = 0;
    if (lane == 0) t = take_ticket(&sy->grp[g * 16]);
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    if (t != (unsigned)n_g - 1u) return;
    ticket_acquire();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    // the group's lists: workgroups g, g + ng, ...
    acc = merge_lists([&](int w) { return qparts + (size_t)(g + w * ng) * k; }, n_g, k, sc, lane);
    if (lane < k) st_agent(qparts + (size_t)(nbx + g) * k + lane, acc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    t = 0;
    if (lane == 0) t = take_ticket(&sy->done);
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    if (t != (unsigned)ng - 1u) return;
    ticket_acquire();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const uint64_t fin = merge_lists([&](int w) { return qparts + (size_t)(nbx + w) * k; }, ng, k, sc, lane);
    const int row = out_rows ? out_rows[qy] : qy;
    if (lane < k) out[(size_t)row * k + lane] = fin;
    if (counted && lane == 0) totals[row] = __hip_atomic_load(&sy->wcount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the query's rendezvous left zeroed for the next launch that uses it (a one-query launch from
    // the resident images reuses its lane's ScanSync with no upload): every workgroup of the query
    // took its group ticket after its last block claim, and every group its done ticket, so nothing
    // reads, claims or counts from it any more (plain vector stores; the next launch sees them)
    uint4* z = reinterpret_cast<uint4*>(sy);
    for (int i = lane; i < (int)(sizeof(ScanSync) / 16); i += 64) z[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <bool PACKED, bool GTAB>
__global__ __launch_bounds__(kScanThreads, 4) void fas_scan_kernel(DevStore st, const uint8_t* __restrict__ pool,
                                                                const QImageRef* __restrict__ refs, int32_t tile_begin,
                                                                int32_t tile_end, int32_t k,
                                                                uint64_t* __restrict__ parts,
                                                                ScanSync* __restrict__ sync,
                                                                uint64_t* __restrict__ out,
                                                                const int32_t* __restrict__ out_rows, CandFilter F,
                                                                FieldSel S, ScanWindow WN, uint32_t* __restrict__ totals,
                                                                uint64_t* __restrict__ cbuf, uint32_t ccap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const QImageRef r = refs[blockIdx.y];
    char* scratch;
    const QView v = stage_query<GTAB>(smem, pool, r, &scratch, S);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t list = ~0ull;
    uint32_t wcnt = 0u;  // a counted window: the wave's keys in it
    // Tile hand-out, longest tiles first.  Static zig-zag for all but the last two bands
    // (band b = tiles [b*W, (b+1)*W) holds W near-equal tiles; wave w takes one per band,
    // alternating direction), then the tail from per-XCD counters, so waves that drew
    // cheap tiles (few hits) take more.  One shared counter for every tile serialises at
    // ~13 ns per fetch and halved the streaming rate; per-XCD counters on the last
    // bands only keep the fetches few and uncontended.
    const int W = (int)gridDim.x * (kScanThreads / 64), wid = (int)blockIdx.x * (kScanThreads / 64) + wave;
    const int ntiles = tile_end - tile_begin;
    const int nstatic = max(0, ntiles / W - 2) * W;
    // blocks are dispatched to the 8 XCDs round-robin; with fewer than 8 blocks every
    // group still has one, so every residue class of the tail is drained
    const int ngrp = min(8, (int)gridDim.x), xcd = (int)blockIdx.x % ngrp;
    unsigned* xctr = &sync[blockIdx.y].xcd_next[xcd * 16];
    for (int b = 0;; ++b) {
        int tile;
        if (b * W < nstatic) {
            tile = tile_begin + b * W + ((b & 1) ? W - 1 - wid : wid);
        } else {
            unsigned t = 0;
            if (lane == 0) t = atomicAdd(xctr, 1u);
            t = __builtin_amdgcn_readfirstlane(t);
            tile = tile_begin + nstatic + (int)t * ngrp + xcd;  // group x drains tail tiles = x (mod ngrp)
        }
        if (tile >= tile_end) break;
        const uint32_t lgk = st.tile_lgk[tile];
        const int slot0 = (int)st.tile_slot0[tile];
        const int cand = lane >> lgk, ci = lane & ((1 << lgk) - 1);
        const bool active = cand < min(kTileSlots >> lgk, st.n_slots - slot0);
        const int p = slot0 + cand;
        // h0 / h1 are loaded after the walk (the epilogue's first reads): holding them across the
        // walk's double buffer spilled registers
        uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0, h2 = h0;
        if (active) h2 = st.hdr2[p];
        const uint32_t nc = h2.y, nset = h2.y + h2.z;
        const uint32_t len = record_words(h2, PACKED);
        const uint32_t q = chunk_words(len, lgk, PACKED);
        const uint32_t j0 = (uint32_t)ci * q;
        const uint32_t clen = (active && len > j0) ? min(q, len - j0) : 0u;
        const Loc l{tile, cand, lgk};
        Walk W;
        W.cnt = 0; W.nh = 0; W.pend = 0;
        if (!PACKED && clen > 0 && j0 > 0) W.pend = word_at(st, l, q, j0 - 1);  // a token pair may straddle chunks
        walk_chunk<PACKED, false>(W, st.stream + st.tile_off[tile] + lane, j0, clen, nc, nset, v, blockDim.x);
        // one epilogue site (a second inlined copy for split records cost K1 64 B of scratch per
        // lane): a split record sums its chunk counters over its lanes, publishes the hit counts,
        // and its first lane finishes it; a whole record (lgk = 0) is the one-chunk case
        if (active) {
            h0 = st.hdr0[p];
            h1 = st.hdr1[p];
        }
        float f = 0.0f;
        uint32_t cnt = W.cnt;
        for (int m = 1; m < (1 << lgk); m <<= 1) cnt += (uint32_t)__shfl_xor((int)cnt, m);
        v.nh[threadIdx.x] = W.nh;
        __builtin_amdgcn_wave_barrier();
        // a candidate the context's filter (pf_filter.h; fields == 0: none) fails gets no epilogue and no key
        const bool scored = active && ci == 0 && (F.fields == 0u || filter_pass_tile(F, h0, h1, h2));
        if (scored) {
            const uint32_t* nhp = v.nh + threadIdx.x;
            const TileRec rec{&st, l, q};
            f = fas_epilogue<PACKED>(v, rec, h0, h1, h2, cnt, threadIdx.x, 1u << lgk, [&](uint32_t g) { return nhp[g]; });
        }
        uint64_t key = ~0ull;
        if (scored) {
            const int32_t uid = (int32_t)h1.w;
            if (!excluded<PACKED>(v, (uint32_t)uid)) key = score_key(f, uid);
        }
        // the score window (pf_window.h; fields == 0: none): a key outside it is no key
        if (WN.fields != 0u) {
            if (!window_pass(key, WN)) key = ~0ull;
            if (WN.fields & kWinCount) wcnt += (uint32_t)__popcll(__ballot(key != ~0ull));
            // a collecting launch keeps the key (the wave is whole here: the tile is the wave's)
            if (WN.fields & kWinCollect) collect_append(key, ~0ull, &sync[blockIdx.y].ccursor, cbuf, ccap, lane);
        }
        topk_push(list, key, k, lane);
    }
    post_tail(list, k, reinterpret_cast<uint64_t*>(scratch), sync, parts, out,
              out_rows, (int)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, (WN.fields & kWinCount) != 0u, wcnt, totals);
}

// ---------------------------------------------------------------- K5: postings scan
// All-candidates FAS (A13) through the postings store (pf_types.h): a workgroup scores one
// block of kBlockCands (512) consecutive candidates at a time (thread i owns candidates i and
// i + 256) from the lists the query names, never the candidates' records:
//   1. ranges: every list's sub-range for this block (one cell lookup per list);
//   2. sets: club / friend list entries add their multiplicity to per-candidate LDS
//      counters (integer, order-free) and the exclusion list marks adj[q] + {q};
//   3. fixed terms (public .. friends) per owned candidate from its 32-B header;
//   4. text, in ROUNDS of <= 64 query tokens (whole columns where they fit, the columns in
//      ascending order) whose list entries in the block fit the round's kRoundCap hit slots:
//      a. walk: every entry of the round's lists, flattened over the workgroup (all loads in
//         flight at once), sets bit (token - round start) of its candidate's 64-bit hit mask;
//      b. slots: each wave gives its candidates' hits a contiguous range of hit slots, a
//         candidate's hits in token order (= column, then tid ascending);
//      c. place: every entry writes its tf and token into its slot (the slot index is the
//         popcount of the mask below its bit), and the first hit of a column its
//         (candidate, column) norm;
//      d. terms, wave-dense: one lane per (candidate, column) item sums the products of its
//         hits in ascending tid order (recommender.cpp:74-85) and computes the cosine ->
//         sigmoid term (recommender_similarity.cpp:93-113), so the FP64 divisions and exp
//         run on as many lanes as there are items, not once per column for the whole wave;
//      e. the owners add, in the reference's order, each common column's term, or its s = 0
//         term when the candidate has no hit in it.
//      A column longer than a round (> 64 tokens, or more entries than kRoundCap) is split
//      over rounds; its owners carry the dot in registers and compute its term themselves.
//   5. FAS (recommender_similarity.cpp:114-123), idx-keyed wave top-k, fused cross-block merge.
// A block costs 2 + 4 x rounds barriers and one memory round trip per round (the walk); the
// round-1 design paid two barriers and a round trip per 8-token pass (21.6 passes per block).

// A query token in LDS: its weight and idf (the product wq * (tf * idf), recommender.cpp:74-85)
struct PTok {
    double wq, idf;
};

// LDS carve of the fixed part (after QConst)
constexpr uint32_t kLdsMask = 0;                                          // u64 [kBlockCands] hit masks
constexpr uint32_t kLdsSlot = kLdsMask + 8 * kBlockCands;                 // f64 [kRoundCap] norm -> term
constexpr uint32_t kLdsHit = kLdsSlot + 8 * kRoundCap;                    // u16 [kRoundCap] hits
constexpr uint32_t kLdsHbase = kLdsHit + 2 * kRoundCap;                   // u16 [kBlockCands] first slot
// the set counters and exclusion bits are read by the fixed terms only, before any thread passes
// round 0's walk barrier and writes a slot: they live in the slots
constexpr uint32_t kLdsCnt = kLdsSlot;                                    // u32 [kBlockCands] set counters
constexpr uint32_t kLdsExb = kLdsCnt + 4 * kBlockCands;                   // u32 [kBlockCands / 32] excluded
static_assert(4 * kBlockCands + 4 * (kBlockCands / 32) <= 8 * kRoundCap, "set counters alias the slots");
constexpr uint32_t kLdsItem = kLdsHbase + 2 * kBlockCands;                // u16 [kRoundCap] term items
constexpr uint32_t kLdsMisc = (kLdsItem + 2 * kRoundCap + 15) & ~15u;       // u32 [16]
constexpr uint32_t kLdsCols = kLdsMisc + 64;                              // QCol [kPostMaxCols]
constexpr uint32_t kLdsFtab = kLdsCols + 16 * kPostMaxCols;               // f64 [7 + 48 + 1] F by used
constexpr uint32_t kLdsSeg = kLdsFtab + 8 * (kNumFixed + kPostMaxCols + 1);  // u32 [kRoundToks] token segments
constexpr uint32_t kLdsCidx = kLdsSeg + 4 * kRoundToks;                   // end of the fixed tables
// round list maps, two buffers (the next round's is built during this one): flat entry f < kRoundCap
// -> its list without a search (bits of the nonempty lists' starts, nonempty lists before each
// 64-entry word, and per nonempty list {entry index of flat 0, token - round start})
constexpr uint32_t kMapWords = kRoundCap / 64;
constexpr uint32_t kLdsMapB = (kLdsCidx + 7) & ~7u;                            // u64 [2][kMapWords]
constexpr uint32_t kLdsMapN = kLdsMapB + 2 * 8 * kMapWords;                   // uint2 [2][kRoundToks]
constexpr uint32_t kLdsMapC = kLdsMapN + 2 * 8 * kRoundToks;                  // u8 [2][kMapWords]
// per column number of the current round: the round-relative tokens before its end (a mask); per
// active column index c: the column numbers of active columns < c as a mask (a round's columns
// [ca, ce) = cpre[ce] & ~cpre[ca])
constexpr uint32_t kLdsLmk = (kLdsMapC + 2 * kMapWords + 7) & ~7u;            // u64 [kPostMaxCols]
constexpr uint32_t kLdsCpre = kLdsLmk + 8 * kPostMaxCols;                     // u64 [kPostMaxCols + 1]
// pruning (pf_prune.h): the block's need[u] by terms used
constexpr uint32_t kLdsNeed = kLdsCpre + 8 * (kPostMaxCols + 1);              // f64 [7 + 48 + 1]
constexpr uint32_t kPostFixedLds = (kLdsNeed + 8 * (kNumFixed + kPostMaxCols + 1) + 15) & ~15u;
static_assert(kBlockCands == 2 * kPostThreads, "two candidates per thread");
static_assert(kRoundCap < 65536 && kBlockCands <= kRoundCap, "u16 slots; a one-token round fits");
static_assert(kPostWaves * kMaxTopK * 8 + 16 + 4 * kMaxTopK <= 8 * kRoundCap, "post_tail scratch in the slots");

// hit slot: tf | token - round start << 8 | first hit of its column segment | first hit of its candidate
constexpr uint32_t kHitFirst = 1u << 14;
constexpr uint32_t kHitCand = 1u << 15;
// token segment (per token of a round): segment start | end << 8 (round-relative) | column << 16 |
// split (the column spans several rounds) << 24
constexpr uint32_t kSegSplit = 1u << 24;
// colof of a token whose column a field selection left out (active column indices are < kPostMaxCols)
constexpr uint8_t kColDead = 0xFFu;

#ifdef PF_K5_CHECK
// checked build (tools/build_variant.sh k5chk XFLAGS=-DPF_K5_CHECK): every global index of K5 is
// range-checked; a bad one is reported and replaced by 0 instead of faulting
__device__ __forceinline__ uint32_t k5_chk(uint32_t i, uint32_t n, int what) {
    if (i >= n) {
        printf("K5 CHECK %d: index %u >= %u (block %d thread %d)\n", what, i, n, (int)blockIdx.x, (int)threadIdx.x);
        return 0u;
    }
    return i;
}
#define K5CHK(i, n, w) k5_chk((i), (n), (w))
#else
#define K5CHK(i, n, w) (i)
#endif


// K5 under a field selection: the high word of a deselected column's token's weight in the staged
// tokens (a NaN no real weight has).  The block's prefix scan counts such a token's range as empty,
// so no entry of it is ever walked.
constexpr uint32_t kTokDeadHi = 0xFFFFFFFFu;

// entries of list L for candidates [c0, c1] (cells c0 >> shift .. c1 >> shift)
__device__ __forceinline__ uint2 list_range(const PostStore& ps, const PList& L, uint32_t c0, uint32_t c1) {
    return make_uint2(L.off + ps.cells[K5CHK(L.cell_off + (c0 >> L.shift), ps.n_cells, 1)],
                      L.off + ps.cells[K5CHK(L.cell_off + (c1 >> L.shift) + 1, ps.n_cells, 2)]);
}

// the set list of flat entry f < spre[n]: the last j with spre[j] <= f (a nonempty one)
__device__ __forceinline__ int set_list(const uint32_t* spre, int n, uint32_t f) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (spre[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// gpre[j] = sum of the lengths of ranges 0 .. j-1 (j <= nl), by one wave
// DEAD: list j whose staged token weight carries the dead mark (dead[j], kTokDeadHi) counts as empty
template <bool DEAD = false>
__device__ __forceinline__ void wave_prefix(uint32_t* gpre, const uint2* rng, int nl, int lane, const PTok* dead = nullptr) {
    uint32_t carry = 0;
    for (int b = 0; b < nl; b += 64) {
        const int j = b + lane;
        uint32_t len = j < nl ? rng[j].y - rng[j].x : 0u;
        if constexpr (DEAD) {
            if (j < nl && reinterpret_cast<const uint32_t*>(dead)[4 * j + 1] == kTokDeadHi) len = 0u;
        }
        uint32_t x = len;
        x = wave_incl_scan(x);
        if (j < nl) gpre[j] = carry + x - len;
        carry += wave_last(x);
    }
    if (lane == 0) gpre[nl] = carry;
}

// the list of flat round entry g (gpre[ja] <= g < gpre[jb], jb - ja <= 64): the last list
// starting at or before g, branch-free (a probe past the round reads gpre[jb] > g)
__device__ __forceinline__ int round_list(const uint32_t* gpre, int ja, int jb, uint32_t g) {
    int j = ja;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) j += gpre[min(j + s, jb)] <= g ? s : 0;
    return j;
}

// The list map of round [ja, jb) into buffer (mb, mc, mn), by one wave (lane = its lane): bit
// s_j of mb for each list j whose entries start at flat s_j < kRoundCap and are nonempty, mc[w] =
// such lists starting before word w, mn[k] = the k-th one's {entry index of flat 0, j - ja}.
template <int CAP = kRoundCap>
__device__ __forceinline__ void build_map(uint64_t* mb, uint8_t* mc, uint2* mn, const uint32_t* gpre,
                                          const uint2* rng, int ja, int jb, int lane) {
    constexpr int kMW = CAP / 64;
    const uint32_t g0 = gpre[ja];
    const int j = ja + lane;
    uint32_t s = 0;
    bool ne = false;
    if (j < jb) {
        s = gpre[j] - g0;
        ne = gpre[j + 1] - g0 > s && s < (uint32_t)CAP;
    }
    if (lane < kMW) mb[lane] = 0ull;
    const uint64_t bal = __ballot(ne);
    const uint32_t k = (uint32_t)__popcll(bal & low_bits((uint32_t)lane));
    wave_sync();
    if (ne) {
        atomicOr(reinterpret_cast<unsigned long long*>(&mb[s >> 6]), 1ull << (s & 63u));
        mn[k] = make_uint2(rng[j].x - s, (uint32_t)lane);
    }
    wave_sync();
    const uint32_t c = lane < kMW ? (uint32_t)__popcll(mb[lane]) : 0u, x = wave_incl_scan(c);
    if (lane < kMW) mc[lane] = (uint8_t)(x - c);
}

// A term item: the slot of a (candidate, column)'s first hit in the round and the column's hit
// count there (kItemRunMax: count the run by the hit flags instead)
constexpr uint32_t kItemRunShift = 11, kItemSlotMask = (1u << kItemRunShift) - 1u, kItemRunMax = 31;
static_assert(kRoundCap <= (int)kItemSlotMask + 1, "item slots fit 11 bits");
// hits of a candidate's column segment [lo, hi) of the round (its mask's bits there), capped
__device__ __forceinline__ uint32_t hit_run(uint64_t m, uint32_t lo, uint32_t hi) {
    return min((uint32_t)__popcll((m >> lo) & low_bits(hi - lo)), kItemRunMax);
}
// dot + slot[r + 1] + ... + slot[r + run - 1], added in that order (recommender.cpp:74-85 sums a
// column's products one by one): the reads are independent, four issued ahead of the adds
__device__ __forceinline__ double run_dot(const double* slot, uint32_t r, uint32_t run, double dot) {
    for (uint32_t k = 1; k < run; k += 4) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = k + u < run ? slot[r + k + u] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k + u < run) dot += v[u];
    }
    return dot;
}

// product of one shared token, recommender.cpp:74-85: wA * wB, wB = tf * idf
__device__ __forceinline__ double tok_product(const PTok* pt, int j, uint32_t tf) {
    const PTok v = pt[j];
    return v.wq * ((double)tf * v.idf);
}

// (Round, the serial next_round and the lane-parallel plan_round: pf_plan.h)

// The query's score histogram and theta (ScanSync, pf_prune.h).  At a block's end every wave folds
// the score bits of the best of its top-k keys that is the block's own (idx in [c0, c1]: each
// candidate at most once; a key evicted later was still a real candidate with that score) and scores
// at least thb, the theta the block began with, into one LDS word with a max (positive float bits
// order as integers): the workgroup's record of the block, nonzero when there is one.  One key per
// workgroup and block, not one per wave or all k of them: the true top k of the candidates processed
// so far are almost surely the best of their own block, and every agent-scope atomic is served at
// the memory side, one address at a time (with k keys per wave the first resident round's 36,000
// adds on a few dozen bins cost a cfg-2 launch 70 us, 0.128 -> 0.200 ms per step).
// Any subset recorded is valid: theta is the lower edge of the highest bin with >= k recorded scores
// at or above it, so >= k real candidates score >= theta.  Relaxed atomics: theta only rises and every
// value it held is valid, so a reader that sees an older one only prunes less.
__device__ __forceinline__ void prune_fold(uint32_t* word, uint64_t best, int k, uint32_t c0, uint32_t c1,
                                           uint32_t thb, int lane) {
    uint32_t sb = 0u;
    bool rec = false;
    if (lane < k && best != ~0ull) {
        const uint32_t idx = (uint32_t)best ^ 0x80000000u;
        sb = __float_as_uint(key_score(best));
        rec = idx >= c0 && idx <= c1 && sb >= thb && prune_bin(sb) >= 0;
    }
    const uint64_t bal = __ballot(rec);
    if (bal == 0ull) return;
    if (lane == __ffsll((unsigned long long)bal) - 1) atomicMax(word, sb);  // ascending keys: the lowest lane holds the best
}

// theta from the histogram, by one wave at the start of the block after one in which the workgroup
// recorded (rec, that block's record): the slabs of pf_prune.h, all loads issued together with the
// load of theta itself.  The wave counts its own record in its registers and sends the record's add
// only once the loads are back, so the add is not among what they saw and nothing waits for it.
// The max is sent only if the derived value exceeds both thb and the theta just read.  Returns the
// block's theta: the highest of thb, the theta read and the derived one (each was valid when read).
// Out of line: its 13 counts per lane stay out of the block loop's register budget.  Three
// arguments, not five: with k and the lane passed on their own the filtered instantiations spilled
// two VGPRs (16 B of scratch).  thk = thb | k: a theta is 0 or a bin's lower edge, its low
// kPruneShift bits clear, and k <= kMaxTopK fits them.
static_assert(kMaxTopK < (1 << kPruneShift), "k rides in a theta's low bits");
static __device__ __attribute__((noinline)) uint32_t prune_derive(ScanSync* sy, uint32_t thk, uint32_t rec) {
    constexpr uint32_t kLow = (1u << kPruneShift) - 1u;
    const int lane = (int)(threadIdx.x & 63u), k = (int)(thk & kLow);
    const uint32_t thb = thk & ~kLow;
    const int ns = prune_slabs(thb), rb = prune_bin(rec);
    uint32_t cb[kPruneSlabs];
#pragma unroll
    for (int i = 0; i < kPruneSlabs; ++i) {
        const int b = prune_slab_bin(i, lane);
        cb[i] = 0u;
        if (i < ns && prune_bin_live(b, thb)) cb[i] = __hip_atomic_load(&sy->hist[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t cur = __hip_atomic_load(&sy->theta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t above = 0u, nt = 0u;
#pragma unroll
    for (int i = 0; i < kPruneSlabs; ++i) {
        if (i < ns && above < (uint32_t)k) {  // wave-uniform
            const int b = prune_slab_bin(i, lane);
            const uint32_t c = cb[i] + ((b == rb && prune_bin_live(b, thb)) ? 1u : 0u);
            const uint32_t incl = wave_incl_scan(c);
            if (prune_pick(above, incl, c, (uint32_t)k)) nt = prune_edge(b);
            above += wave_last(incl);
        }
    }
    nt = wave_max_u32(nt);
    if (lane == 0) {
        __hip_atomic_fetch_add(&sy->hist[rb], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nt > thb && nt > cur) __hip_atomic_fetch_max(&sy->theta, nt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    nt = nt > cur ? nt : cur;
    return nt > thb ? nt : thb;
}

#ifdef PF_K5_TIMERS
// profiling build only (make K5T=1): per-phase clock64() sums over every wave, printed by
// launch_post every 10th launch
#define K5T(slot) do { const uint64_t t_ = clock64(); tacc[slot] += t_ - tprev; tprev = t_; } while (0)
#else
#define K5T(slot) do { } while (0)
#endif

#ifndef PF_K5_MINB
#define PF_K5_MINB 4  // workgroups per CU the register budget is sized for (LDS allows 4 for most queries)
#endif
// XD: how the launch's blocks (B = ps.bsize candidates each) are handed out; launch_post's caller
// picks the instantiation (`claimed`).
//   <true>  the one-query launch (grid x = workgroups): every block is claimed per XCD group.
//   <false> the batches (grid = workgroups x queries): a static stride, workgroup bx takes blocks
//           pb, pb + nbx, ... of its query, pb = bx in XCD-contiguous order.
// The pruning bound and its counters are one text for both: a batch workgroup prunes against its
// query's sync[qy], whose theta warms over the ~32 blocks the workgroup runs in turn.
// FILT: the context has a candidate filter (pf_filter.h, F; launch_post picks the instantiation): a
// candidate whose header fails it is dropped like an excluded one, a block in which nobody passes
// is left after its first barrier.  <XD, false> never reads F and is the code it was without it.
// SEL: the context has a field selection (pf_select.h, S; launch_post picks the instantiation): the
// staged copy of the query's constants is patched before the staging barrier publishes it, so the
// fixed terms, pend, ftab and need[] (the pruning bound's 7 + T') follow by themselves; the
// deselected columns are left out of scol / cpre / colof, their tokens count no entries in any
// block's prefix (no entry is walked, no round is planned for them), and the deselected club /
// friend lists are left out of the set lists.  S is read during staging only: nothing of it lives
// through the block loop.  <XD, FILT, false> never reads S and is the code it was without it.
// WIN: the context has a score window (pf_window.h, W with its cursor in idx space; launch_post picks
// the instantiation).  A key outside the window becomes ~0 before the lane's 2-key sort: it is never
// pushed, never in `best` and never folded into the histogram, so "only keyed candidates are
// recorded" (pf_prune.h) holds and theta stays valid under a cursor.  A floor seeds every block's
// theta with W.theta0, valid before the first block: the bound drops only candidates strictly below
// theta, so nobody at or above the floor dies, and the exact >= min_score test is the key's.  A
// counted launch keeps theta at the seed (no record, no derive: candidates between the floor and a
// risen theta would be dropped uncounted), counts its in-window keys into misc[6] and hands the sum
// to post_tail.  W's words are parked in LDS past the filter's, like the filter.  <XD, FILT, SEL,
// false> never reads W and is the code it was without it.
template <bool XD, bool FILT, bool SEL, bool WIN>
__global__ __launch_bounds__(kPostThreads, PF_K5_MINB) void fas_post_kernel(PostStore ps, const uint8_t* __restrict__ pool,
                                                              const uint32_t* __restrict__ img_off, int32_t blk_begin,
                                                              int32_t blk_end, int32_t k, uint64_t* __restrict__ parts,
                                                              ScanSync* __restrict__ sync, uint64_t* __restrict__ out,
                                                              const int32_t* __restrict__ out_rows, uint32_t mode,
                                                              const uint8_t* __restrict__ qconst, CandFilter F,
                                                              FieldSel S, ScanWindow W, uint32_t* __restrict__ totals,
                                                              uint64_t* __restrict__ cbuf, uint32_t ccap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int qy = XD ? 0 : (int)blockIdx.y;
    const int bx = (int)blockIdx.x;
    const int nbx = (int)gridDim.x;
    const uint8_t* img = pool + img_off[qy];
    // the query's QConst: the image's own prefix, or (qconst given: one-query launches from the
    // resident images) the job pipeline's resident K1' image of the same user, whose QConst K6
    // builds from the same tables; the image's own part then starts sizeof(QConst) past img
    const uint8_t* qcp = qconst ? qconst : img;
    QPostHead H = *reinterpret_cast<const QPostHead*>(img + sizeof(QConst));
    const QTok* toks = reinterpret_cast<const QTok*>(img + H.tok_off);
    const QCol* cols = reinterpret_cast<const QCol*>(img + H.col_off);
    const PList* sets = reinterpret_cast<const PList*>(img + H.set_off);
    const int n_act_img = H.n_act;  // the image's active columns (SEL: H.n_act becomes the selected ones)
    if constexpr (SEL) {
        // a deselected set's lists (the clubs' come first) are not there at all: the LDS carve below
        // only shrinks
        if (!(S.fixed & kSelClubs)) { sets += H.n_club; H.n_club = 0; }
        if (!(S.fixed & kSelFriends)) H.n_friend = 0;
        int na = 0;
        for (int j = 0; j < n_act_img; ++j) na += (int)((S.cols >> cols[j].t) & 1ull);
        H.n_act = na;
    }
    const uint32_t* excl = reinterpret_cast<const uint32_t*>(img + H.excl_off);
    const int tid = (int)threadIdx.x, lane = tid & 63;
    char* base = smem + sizeof(QConst);
    uint64_t* mask = reinterpret_cast<uint64_t*>(base + kLdsMask);
    double* slot = reinterpret_cast<double*>(base + kLdsSlot);
    uint16_t* hit = reinterpret_cast<uint16_t*>(base + kLdsHit);
    uint16_t* hbase = reinterpret_cast<uint16_t*>(base + kLdsHbase);
    uint16_t* item = reinterpret_cast<uint16_t*>(base + kLdsItem);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(base + kLdsCnt);
    uint32_t* exb = reinterpret_cast<uint32_t*>(base + kLdsExb);
    uint32_t* misc = reinterpret_cast<uint32_t*>(base + kLdsMisc);  // [0] next block, [1] hit slots taken
    QCol* scol = reinterpret_cast<QCol*>(base + kLdsCols);
    double* ftab = reinterpret_cast<double*>(base + kLdsFtab);  // F = used / (7 + T) by used
    uint32_t* seg = reinterpret_cast<uint32_t*>(base + kLdsSeg);
    const int nsets = H.n_club + H.n_friend;
    const int nl = H.n_tok + nsets;
    PTok* pt = reinterpret_cast<PTok*>(base + kPostFixedLds);
    // (the list descriptors are not staged: each block reads them from the image, an L2 hit, so a
    // query with ~200 tokens still fits four workgroups per CU)
    uint2* rng = reinterpret_cast<uint2*>(pt + H.n_tok);
    uint2* rtab = rng + nl;  // the block's rounds (ja | jb << 16, ca | ce << 16), <= n_tok of them
    uint32_t* gpre = reinterpret_cast<uint32_t*>(rtab + H.n_tok + 1);
    uint32_t* spre = gpre + H.n_tok + 1;  // the set lists' prefix [nsets + 1]
    uint8_t* colof = reinterpret_cast<uint8_t*>(spre + nsets + 1);  // token -> active column index
    uint64_t* mapb = reinterpret_cast<uint64_t*>(base + kLdsMapB);
    uint2* mapn = reinterpret_cast<uint2*>(base + kLdsMapN);
    uint8_t* mapc = reinterpret_cast<uint8_t*>(base + kLdsMapC);
    uint64_t* lmk = reinterpret_cast<uint64_t*>(base + kLdsLmk);
    uint64_t* cpre = reinterpret_cast<uint64_t*>(base + kLdsCpre);
    double* need = reinterpret_cast<double*>(base + kLdsNeed);
    // mode bit 16 (both hand-outs; a batch workgroup works on its query's own sync[qy]): candidates
    // that cannot reach the query's shared threshold theta (ScanSync, pf_prune.h) are dropped before
    // their text work; bit 18 leaves out the re-check at round ends; bit 17 counts (g_k5_prune).
    // Uniform over the launch.  A sharded launch prunes against the theta of its own block range.
    // A dropped candidate's skip bit is set and its pending columns cleared; its owner thread
    // clears its hit mask in each round's slot phase, so it takes no hit slot, and the place phase
    // passes over the entries whose mask bit is gone: the compaction, the ordered dots, the terms
    // and its row of the owner sums vanish with them.  (The walk still ORs its bits: testing there
    // needs a bitmap in LDS, a barrier per block and a read per entry, and spilled registers.)
    const bool prune = (mode & kPostPrune) != 0u;
    const bool prune_rnd = prune && !(mode & kPostPruneBlockOnly);
    const bool pstats = (mode & kPostPruneStats) != 0u;
    // The drop mechanics (pend cleared, the mask cleared in the slot phase, place passing over the
    // candidate) serve the filter as well: a filtered instantiation always has them, the batch and
    // k5_prune=0 included; the theta bound itself stays behind `prune`.
    const bool drop = FILT || prune;
    // The filter's 12 uniform words would live in scalar registers through the whole block loop, which
    // already keeps 84 of them in spill lanes (<true> with them: 125 spilled, 2 VGPRs and 16 B of
    // scratch): they are parked once in the kFiltLds bytes a filtered launch allocates past the
    // query's variable part, and each block's header test reads them from there.
    CandFilter* fl = reinterpret_cast<CandFilter*>(
        smem + (((uint32_t)(reinterpret_cast<char*>(colof) + H.n_tok - smem) + 15u) & ~15u));
    if constexpr (FILT) {
        if (tid == 0) *fl = F;
    }
    // the window's words, in the kWinLds bytes a windowed launch allocates past the filter's
    const ScanWindow* wl = reinterpret_cast<const ScanWindow*>(reinterpret_cast<char*>(fl) + (FILT ? kFiltLds : 0u));
    if constexpr (WIN) {
        if (tid == 0) *const_cast<ScanWindow*>(wl) = W;
    }
    if (tid < 16) misc[tid] = 0u;
    stage(smem, qcp, sizeof(QConst));
    if constexpr (!SEL) {
        for (int j = tid; j < H.n_act; j += kPostThreads) {
            const QCol c = cols[j];
            scol[j] = c;
            for (int x = c.j0; x < c.j1; ++x) colof[x] = (uint8_t)j;
        }
        if (tid == 0) {  // prefix masks of the active columns (<= 48, ascending)
            uint64_t m = 0;
            for (int j = 0; j < H.n_act; ++j) { cpre[j] = m; m |= 1ull << cols[j].t; }
            cpre[H.n_act] = m;
        }
        for (int j = tid; j <= kNumFixed + kPostMaxCols; j += kPostThreads)
            ftab[j] = (double)j / (double)(kNumFixed + reinterpret_cast<const QConst*>(qcp)->n_cols);
    } else {
        // the selected columns only, in their order; a deselected column's tokens keep their place
        // in the token arrays (the images are not edited) and are marked kColDead here and
        // kTokDeadHi in the staged tokens below, so every block's prefix scan counts them no entries
        for (int j = tid; j < n_act_img; j += kPostThreads) {
            const QCol c = cols[j];
            int js = 0;  // selected columns before this one
            for (int x = 0; x < j; ++x) js += (int)((S.cols >> cols[x].t) & 1ull);
            const bool on = (S.cols >> c.t) & 1ull;
            if (on) scol[js] = c;
            for (int x = c.j0; x < c.j1; ++x) colof[x] = on ? (uint8_t)js : kColDead;
        }
        if (tid == 0) {
            uint64_t m = 0;
            int js = 0;
            for (int j = 0; j < n_act_img; ++j) {
                const int t = cols[j].t;
                if ((S.cols >> t) & 1ull) { cpre[js++] = m; m |= 1ull << t; }
            }
            cpre[js] = m;
        }
        const int ncs = select_ncols(S.cols, reinterpret_cast<const QConst*>(qcp)->n_cols);
        for (int j = tid; j <= kNumFixed + kPostMaxCols; j += kPostThreads)
            ftab[j] = (double)j / (double)(kNumFixed + ncs);
        // the constants' patch: after every thread's part of the copy, before the barrier below
        // publishes the staged tables
        __syncthreads();
        if (tid == 0) select_apply(*reinterpret_cast<QConst*>(smem), S);
    }
    for (int j = tid; j < H.n_tok; j += kPostThreads) {
        const QTok t = toks[j];
        pt[j] = PTok{t.wq, t.idf};
        if constexpr (SEL) {  // (colof is complete: SEL's barrier above)
            if (colof[j] == kColDead) reinterpret_cast<uint32_t*>(pt + j)[1] = kTokDeadHi;
        }
    }
    __syncthreads();  // the staged tables are read by other threads
    const QConst& q = *reinterpret_cast<const QConst*>(smem);
    uint64_t best = ~0ull;
#ifdef PF_K5_TIMERS
    uint64_t tacc[14] = {0};
    uint64_t tprev = clock64();
    const uint64_t tstart = tprev;
#endif
    const uint32_t B = (uint32_t)ps.bsize;
    const uint32_t cend = min((uint32_t)blk_end * B, (uint32_t)ps.n);  // the range's end
    const bool short_excl = H.n_excl <= kPostThreads;
    const uint32_t ex0 = short_excl && H.n_excl > 0 ? excl[min(tid, H.n_excl - 1)] : ~0u;  // the query's, once
    // <false>: blocks pb, pb + nbx, ... of the query.  The workgroups of XCD x (bx mod 8 under the
    // round-robin dispatch when nbx is a multiple of 8) take blocks [x nbx/8, (x + 1) nbx/8) of each
    // stride round, so a list segment's boundary cache lines are shared inside one L2 instead of
    // fetched by two XCDs (cfg 2 PMC traffic 236 -> 175 MB per launch, r4w -> r5h)
    const int pb = (nbx & 7) == 0 ? (bx & 7) * (nbx >> 3) + (bx >> 3) : bx;
    // <true>: every block claimed, per group g = bx mod 8 (with round-robin dispatch, one XCD) from
    // a contiguous eighth of the range, in order, from the group's own counter.  The workgroups
    // dispatched last (the third and fourth of a CU) lose VALU arbitration to the older ones by age
    // and ran a static share of blocks ~25 % slower every round (r6j block log): claimed blocks let
    // the faster workgroups take more.  The next block is claimed at the start of a block's last
    // text round, so the claim's round trip hides behind that round.
    const int xng = min(8, nbx), xg = bx % xng;
    const int x_lo = blk_begin + (int)((int64_t)(blk_end - blk_begin) * xg / xng);
    const int x_hi = blk_begin + (int)((int64_t)(blk_end - blk_begin) * (xg + 1) / xng);
    const int x_nwg = (nbx - xg + xng - 1) / xng;
    unsigned int* xctr = &sync[qy].xcd_next[xg * 16];
    const int blk_last = XD ? x_hi : blk_end;
    for (int blk = XD ? x_lo + bx / xng : blk_begin + pb; blk < blk_last;) {
        unsigned int xclaim = 0;
        // The next block, behind a barrier (the next block rewrites the exclusion bits the owners
        // read in this one).  <true>: thread 0 publishes the group's next claim through misc[0],
        // the one fetched at the start of the last text round (xclaim) or, `now`, one taken on the
        // spot; <false>: the stride.
        auto next_block = [&](bool now) __attribute__((always_inline)) {
            if constexpr (XD) {
                if (tid == 0) misc[0] = (uint32_t)(x_lo + x_nwg) + (now ? atomicAdd(xctr, 1u) : xclaim);
                __syncthreads();
                blk = (int)misc[0];
            } else {
                __syncthreads();
                blk += nbx;
            }
        };
        const uint32_t c0 = (uint32_t)blk * B;
        const uint32_t c1 = min(c0 + B, cend) - 1;  // last candidate of the block
#ifdef PF_K5_BLOCKLOG
        const unsigned long long blog_t0 = __builtin_amdgcn_s_memrealtime();
#endif
        // 1. headers of the owned candidates and every list's range in this block: all loads
        // issued before the first wait, one memory round trip.  (Loading the next static block's
        // headers and ranges before this block's FAS measured slower: 184.8 -> 188.0 us, r4n,
        // the 16 registers they hold spilled)
        uint4 ha[kCandsPerThread], hb[kCandsPerThread];
#pragma unroll
        for (int kk = 0; kk < kCandsPerThread; ++kk) {  // clamped (always valid) index, zeroed below
            const uint32_t c = min(c0 + kk * kPostThreads + tid, c1);
            ha[kk] = ps.hdr[2 * (size_t)c];
            hb[kk] = ps.hdr[2 * (size_t)c + 1];
        }
        // the threshold as of now (only ever raised: a stale value prunes less), with the headers' loads
        uint32_t thb = 0u;
        if (prune) thb = __hip_atomic_load(&sync[qy].theta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (WIN) {  // a floor's seed: no block begins cold (published by the staging barrier)
            if (prune) thb = max(thb, wl->theta0);
        }
#pragma unroll 1  // (unrolled by two, its second lane set's masks and trip count lived through the block loop)
        for (int j = tid; j < nl; j += kPostThreads)
            rng[j] = list_range(ps, j < H.n_tok ? toks[j].l : sets[j - H.n_tok], c0, c1);
#pragma unroll
        for (int kk = 0; kk < kCandsPerThread; ++kk) {
            const uint32_t c = c0 + kk * kPostThreads + tid;
            if (!(c <= c1 && (uint32_t)(kk * kPostThreads + tid) < B)) {
                ha[kk] = make_uint4(0, 0, 0, 0);
                hb[kk] = make_uint4(0, 0, 0, 0);
            }
            cnt[kk * kPostThreads + tid] = 0u;
            mask[kk * kPostThreads + tid] = 0ull;
        }
        if (tid < kBlockCands / 32) exb[tid] = 0u;
        K5T(0);
        if constexpr (FILT) {
            uint32_t fskip = 0;  // bit kk: candidate kk is there and fails the filter
            // the header test rides on the block's first barrier: when no candidate of the block
            // passes, the block ends here (no sets, no rounds, no top-k push); kPostFiltKeepBlocks
            // (A/B) runs such blocks to their end
            bool any = false;
            const CandFilter f = *fl;  // (published by the staging barrier before the block loop)
#pragma unroll
            for (int kk = 0; kk < kCandsPerThread; ++kk) {
                const bool there = c0 + kk * kPostThreads + tid <= c1 && (uint32_t)(kk * kPostThreads + tid) < B;
                const bool ok = filter_pass_post(f, ha[kk], hb[kk]);
                if (there && !ok) fskip |= 1u << kk;
                any |= there && ok;
            }
            if (!__syncthreads_or(any) && !(mode & kPostFiltKeepBlocks)) {
                if (pstats && tid == 0) {  // seen, in neither dead counter
                    misc[8] += c1 - c0 + 1u;
                    misc[11] += 1u;
                    misc[12] += thb == 0u ? 1u : 0u;
                }
                next_block(true);  // nothing of this block was claimed ahead
                continue;
            }
            // a candidate that fails is marked like an excluded one (the bits were zeroed before the
            // barrier; the exclusion list ORs into the same words below), so step 3 needs no word of
            // the filter and no register carries the result there
#pragma unroll
            for (int kk = 0; kk < kCandsPerThread; ++kk) {
                const uint64_t bal = __ballot((fskip >> kk) & 1u);
                const uint32_t w = (uint32_t)(bal >> (lane & 32));
                if ((lane & 31) == 0 && w != 0u) atomicOr(&exb[(kk * kPostThreads + tid) >> 5], w);
            }
        } else {
            __syncthreads();
        }
        K5T(1);
        if (prune && tid >= kPostThreads - 64) {
            // the block's need[u], by the last wave (wave 0 plans the rounds); read after the barrier
            // below.  After a block in which the workgroup recorded (misc[5], that block's record, folded
            // before its last barrier) the wave takes the record, sends it and derives theta anew.
            thb = (uint32_t)__builtin_amdgcn_readfirstlane((int)thb);
            const uint32_t rec = misc[5];
            if (rec != 0u) {
                thb = prune_derive(sync + qy, thb | (uint32_t)k, rec);
                wave_sync();
                if (lane == 0) misc[5] = 0u;
            }
            const int u = tid - (kPostThreads - 64);
            if (u == 0) misc[4] = thb;  // the block's theta: read again at its end
            if (u >= 0 && u <= kNumFixed + kPostMaxCols) need[u] = prune_need(thb, u, kNumFixed + q.n_cols);
        }
        if (tid < 64) {  // read after the barrier below
            // (the columns' tokens, read again in every block although they never change: held
            // through the block loop they would cost every wave two VGPRs for wave 0's sake; the
            // read is in flight under the prefix)
            ColPlan cpl = col_tokens(scol, H.n_act, lane);
            wave_prefix<SEL>(gpre, rng, H.n_tok, lane, pt);  // SEL: a deselected column's tokens count no entries
            wave_sync();
            col_ends(cpl, gpre, H.n_act, lane);
            // the block's rounds, once (every thread used to walk the columns' prefix chain per round)
            {
                int ci0 = 0, j0 = 0, nr = 0;
                while (ci0 < H.n_act) {
                    // (a round never starts among the tokens of deselected columns before column ci0)
                    if constexpr (SEL) j0 = max(j0, __builtin_amdgcn_readlane(cpl.j0, ci0));
                    const Round Rr = plan_round(cpl, gpre, H.n_act, lane, ci0, j0);
                    if (lane == 0)
                        rtab[nr] = make_uint2((uint32_t)Rr.ja | (uint32_t)Rr.jb << 16, (uint32_t)Rr.ca | (uint32_t)Rr.ce << 16);
                    if (nr == 0) build_map(mapb, mapc, mapn, gpre, rng, Rr.ja, Rr.jb, lane);
                    ++nr;
                }
                if (lane == 0) misc[3] = (uint32_t)nr;
            }
        }
        // exclusion list (sorted idx of adj[q] + {q}): whole list when short (loaded above, no
        // barrier of its own), else bisect and walk until past the block
        if (short_excl) {
            const uint32_t p = ex0 - c0;
            if (tid < H.n_excl && p < B) atomicOr(&exb[p >> 5], 1u << (p & 31));
        } else {
            uint32_t lo = 0, hi = (uint32_t)H.n_excl;
            while (lo < hi) {  // first entry >= c0
                const uint32_t mid = (lo + hi) >> 1;
                if (excl[mid] < c0) lo = mid + 1; else hi = mid;
            }
            hi = (uint32_t)H.n_excl;
            for (uint32_t b = lo; b < hi; b += kPostThreads) {
                const uint32_t x = b + tid;
                const uint32_t e = x < hi ? excl[x] : ~0u;
                const uint32_t p = e - c0;
                if (p < B) atomicOr(&exb[p >> 5], 1u << (p & 31));
                if (__syncthreads_or(e >= c0 + B)) break;  // sorted: the rest lies beyond the block
            }
        }
        // 2. clubs / friends, by waves 1-3 while wave 0 plans the rounds: each computes the set
        // lists' prefix itself (the same values, so no barrier) and takes flat entries by bisection
        // (the round-4 walk scanned every set list per entry group on every thread: 17 us of a
        // cfg-2 launch, r6l)
        if (tid >= 64 && nsets > 0) {
            wave_prefix(spre, rng + H.n_tok, nsets, lane);
            wave_sync();
            const uint32_t tot = spre[nsets];
            constexpr uint32_t kSetThreads = kPostThreads - 64;
            for (uint32_t f0 = (uint32_t)tid - 64u; f0 < tot; f0 += 2u * kSetThreads) {
                int js[2];
                uint32_t e[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t f = f0 + u * kSetThreads;
                    js[u] = f < tot ? set_list(spre, nsets, f) : -1;
                    e[u] = js[u] >= 0 ? ps.post[K5CHK(rng[H.n_tok + js[u]].x + (f - spre[js[u]]), ps.n_post, 3)] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t p = (e[u] >> 8) - c0;
                    if (js[u] >= 0 && p < B) atomicAdd(&cnt[p], (e[u] & 0xFFu) << (js[u] < H.n_club ? 0 : 16));
                }
            }
        }
        K5T(2);
        __syncthreads();
        K5T(1);
        // 3. fixed terms, recommender_similarity.cpp:38-91
        double sum[kCandsPerThread];
        uint32_t used = 0;  // byte kk: terms used by candidate kk (<= 7 + 48)
        uint64_t pend[kCandsPerThread];
        uint32_t skip = 0;  // bit kk: candidate kk absent or excluded
#pragma unroll
        for (int kk = 0; kk < kCandsPerThread; ++kk) {
            const int p = kk * kPostThreads + tid;
            const uint32_t ct = cnt[p];
            if ((uint32_t)p >= B || c0 + p > c1 || ((exb[p >> 5] >> (p & 31)) & 1u)) skip |= 1u << kk;
            const uint64_t cm = (uint64_t)ha[kk].x | ((uint64_t)(ha[kk].y & 0xFFFFu) << 32);
            pend[kk] = cm & q.colmask;
            double s = 0.0;
            int u = 0;
            header_terms(q, (ha[kk].y >> 16) & 0xFFu, ha[kk].y >> 24, (int)(int16_t)(ha[kk].z & 0xFFFFu),
                         (int)(int16_t)(ha[kk].z >> 16), (int)hb[kk].x, (int)hb[kk].y, (int)hb[kk].z, s, u);
            set_terms(q, (int)(ct & 0xFFFFu), ha[kk].w & 0xFFFFu, (int)(ct >> 16), ha[kk].w >> 16, s, u);
            sum[kk] = s;
            used |= (uint32_t)(u + __popcll(pend[kk])) << (8 * kk);
        }
        // 3b. the bound at the block's start: every text term still to come counts 1.  The excluded
        // and absent candidates lose their text work the same way.
        if (drop) {
#pragma unroll
            for (int kk = 0; kk < kCandsPerThread; ++kk) {
                const bool sk = (skip >> kk) & 1u;
                const bool d = prune && !sk && prune_dead(sum[kk], (double)__popcll(pend[kk]), need[(used >> (8 * kk)) & 0xFFu]);
                if (sk || d) {
                    skip |= 1u << kk;
                    pend[kk] = 0ull;
                }
                if (pstats) {  // (counted in LDS as they come: no register lives through the block loop for them)
                    const int p = kk * kPostThreads + tid;
                    const uint64_t bs = __ballot((uint32_t)p < B && c0 + p <= c1), bd = __ballot(d);
                    if (lane == 0) {
                        atomicAdd(&misc[8], (uint32_t)__popcll(bs));
                        atomicAdd(&misc[9], (uint32_t)__popcll(bd));
                    }
                }
            }
            if (pstats && tid == 0) {
                misc[11] += 1u;
                misc[12] += misc[4] == 0u ? 1u : 0u;
            }
        }
        K5T(3);
        // 4. text columns in rounds (ascending tokens = ascending columns, then tids)
        double cdot[kCandsPerThread], cnrm[kCandsPerThread];  // a split column's dot / norm so far
        uint32_t chit = 0;                                     // bit kk: the split column has a hit
#pragma unroll
        for (int kk = 0; kk < kCandsPerThread; ++kk) { cdot[kk] = 0.0; cnrm[kk] = 0.0; }
        int nrounds = (int)misc[3];  // written before the barrier above
        if (XD && nrounds == 0 && tid == 0) xclaim = atomicAdd(xctr, 1u);
        for (int rnd = 0; rnd < nrounds; ++rnd) {
            if (XD && rnd == nrounds - 1 && tid == 0) xclaim = atomicAdd(xctr, 1u);
            const uint2 rr = rtab[rnd];
            Round R;
            R.ja = (int)(rr.x & 0xFFFFu);
            R.jb = (int)(rr.x >> 16);
            R.ca = (int)(rr.y & 0xFFFFu);
            R.ce = (int)(rr.y >> 16);
            const int mbuf = rnd & 1;  // this round's list map buffer
            const int ja = R.ja, jb = R.jb;
            const uint32_t g0 = gpre[ja], F = gpre[jb] - g0;  // the round's flat entries
            if (F > 0) {
                // token segments of the round (read after the walk's barrier)
                if (tid < jb - ja) {
                    const int j = ja + tid;
                    // (SEL: a deselected column's token inside the round has no entries; its segment is never read)
                    const QCol c = scol[SEL ? min((int)colof[j], kPostMaxCols - 1) : (int)colof[j]];
                    const int lo = max(c.j0, ja) - ja, hi = min(c.j1, jb) - ja;
                    seg[tid] = (uint32_t)lo | (uint32_t)hi << 8 | (uint32_t)c.t << 16 |
                               ((c.j0 < ja || c.j1 > jb) ? kSegSplit : 0u);
                }
                // per round column (number t): the round-relative tokens before its end (the owner sums
                // take a candidate's hits in t as the mask bits below lmk[t] not taken by earlier columns)
                if (tid < R.ce - R.ca) {
                    const QCol c = scol[R.ca + tid];
                    lmk[c.t] = low_bits((uint32_t)(min((int)c.j1, jb) - ja));
                }
                if (tid == 0) misc[1] = 0u;
                // a. walk: the round's entries flattened over the workgroup, all loads in flight
                constexpr int U = kRoundCap / kPostThreads;
                uint32_t kp[U];  // p | token << 10 | tf << 16, or ~0
                double kn[U];  // (norms loaded in the place phase for first hits only: 184.6 -> 199.1 us, r4q)
                {
                    uint32_t xs[U];
                    int js[U];
                    // (the thread's flat indices and their map words rebuilt per round: as loop
                    // invariants they held 2 U registers through the whole block loop)
                    uint32_t ft = (uint32_t)tid;
                    asm volatile("" : "+v"(ft));
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const uint32_t f = ft + (uint32_t)(kPostThreads * u);
                        // the list map: nonempty lists starting at or before f, minus one
                        js[u] = -1;
                        xs[u] = 0u;  // a valid address
                        if (f < F) {
                            const uint32_t w = f >> 6;
                            const uint32_t kk = (uint32_t)mapc[mbuf * kMapWords + w] +
                                                (uint32_t)__popcll(mapb[mbuf * kMapWords + w] & low_bits((f & 63u) + 1u)) - 1u;
                            const uint2 L = mapn[mbuf * kRoundToks + kk];
                            js[u] = ja + (int)L.y;
                            xs[u] = L.x + f;
                        }
                    }
                    uint32_t ent[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {  // unconditional: every load of the round in flight
                        ent[u] = ps.post[K5CHK(xs[u], ps.n_tok_entries, 4)];
                        kn[u] = ps.pnorm[K5CHK(xs[u], ps.n_tok_entries, 5)];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const uint32_t p = (ent[u] >> 8) - c0;
                        kp[u] = ~0u;
                        if (js[u] >= 0 && p < B) {
                            const uint32_t jr = (uint32_t)(js[u] - ja);
                            kp[u] = p | jr << 10 | (ent[u] & 0xFFu) << 16;
                            atomicOr(reinterpret_cast<unsigned long long*>(&mask[p]), 1ull << jr);
                        }
                    }
                }
                for (uint32_t f = (uint32_t)(tid + kRoundCap); f < F; f += kPostThreads) {  // one-token rounds past the cap
                    const int j = round_list(gpre, ja, jb, g0 + f);
                    const uint32_t p = (ps.post[K5CHK(rng[j].x + (g0 + f - gpre[j]), ps.n_tok_entries, 6)] >> 8) - c0;
                    if (p < B) atomicOr(reinterpret_cast<unsigned long long*>(&mask[p]), 1ull << (j - ja));
                }
                K5T(4);
                __syncthreads();
                K5T(5);
                if (tid < 64 && rnd + 1 < nrounds) {  // the next round's list map (published by the slots barrier)
                    const uint2 r1 = rtab[rnd + 1];
                    const int nb = mbuf ^ 1;
                    build_map(mapb + nb * kMapWords, mapc + nb * kMapWords, mapn + nb * kRoundToks, gpre, rng,
                              (int)(r1.x & 0xFFFFu), (int)(r1.x >> 16), lane);
                }
                // b. hit slots: the wave's candidates' hits in one contiguous range
                uint32_t nk[kCandsPerThread], tot = 0;
#pragma unroll
                for (int kk = 0; kk < kCandsPerThread; ++kk) {
                    uint64_t m = mask[kk * kPostThreads + tid];
                    if (drop && ((skip >> kk) & 1u) && m != 0ull) {  // dropped: no slots, and place passes over its entries
                        mask[kk * kPostThreads + tid] = 0ull;
                        m = 0ull;
                    }
                    nk[kk] = (uint32_t)__popcll(m);
                    tot += nk[kk];
                }
                uint32_t incl = tot;
                incl = wave_incl_scan(incl);
                const uint32_t wn = wave_last(incl);
                uint32_t wb = 0;
                if (lane == 0) wb = atomicAdd(&misc[1], wn);
                wb = (uint32_t)__shfl((int)wb, 0);
                {
                    uint32_t h0 = wb + incl - tot;
#pragma unroll
                    for (int kk = 0; kk < kCandsPerThread; ++kk) {
                        hbase[kk * kPostThreads + tid] = (uint16_t)h0;
                        h0 += nk[kk];
                    }
                }
                K5T(6);
                __syncthreads();
                K5T(1);
                // c. place every hit at its slot, the column's first hit with its norm
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (kp[u] == ~0u) continue;
                    const uint32_t p = kp[u] & 1023u, jr = (kp[u] >> 10) & 63u, tf = kp[u] >> 16;
                    if (drop && !((mask[p] >> jr) & 1ull)) continue;  // a dropped candidate's
                    const uint64_t below = mask[p] & low_bits(jr);
                    const uint32_t r = K5CHK(hbase[p] + (uint32_t)__popcll(below), (uint32_t)kRoundCap, 8);
                    const uint32_t sg = seg[jr], lo = sg & 0xFFu;
                    const bool first = (below >> lo) == 0ull;
                    hit[r] = (uint16_t)(tf | jr << 8 | (first ? kHitFirst : 0u) | (below == 0ull ? kHitCand : 0u));
                    // the column's first hit holds its norm, the others their product (one per lane here,
                    // so the terms below only add them up); the first hit of a column wholly inside the
                    // round records the column's hit count in the round (>= 1), every other slot 0 (item[r],
                    // read once by the compaction below)
                    slot[r] = first ? kn[u] : tok_product(pt, ja + (int)jr, tf);
                    item[r] = (first && !(sg & kSegSplit)) ? (uint16_t)hit_run(mask[p], lo, (sg >> 8) & 0xFFu) : (uint16_t)0;
                }
                for (uint32_t f = (uint32_t)(tid + kRoundCap); f < F; f += kPostThreads) {
                    const int j = round_list(gpre, ja, jb, g0 + f);
                    const uint32_t x = K5CHK(rng[j].x + (g0 + f - gpre[j]), ps.n_tok_entries, 7);
                    const uint32_t e = ps.post[x];
                    const uint32_t p = (e >> 8) - c0;
                    if (p >= B) continue;
                    const uint32_t jr = (uint32_t)(j - ja);
                    if (drop && !((mask[p] >> jr) & 1ull)) continue;  // a dropped candidate's
                    const uint64_t below = mask[p] & low_bits(jr);
                    const uint32_t r = K5CHK(hbase[p] + (uint32_t)__popcll(below), (uint32_t)kRoundCap, 9);
                    const uint32_t sg = seg[jr];
                    const bool first = (below >> (sg & 0xFFu)) == 0ull;
                    hit[r] = (uint16_t)((e & 0xFFu) | jr << 8 | (first ? kHitFirst : 0u) | (below == 0ull ? kHitCand : 0u));
                    slot[r] = first ? ps.pnorm[x] : tok_product(pt, ja + (int)jr, e & 0xFFu);
                    item[r] = (first && !(sg & kSegSplit)) ? (uint16_t)hit_run(mask[p], sg & 0xFFu, (sg >> 8) & 0xFFu) : (uint16_t)0;
                }
                K5T(7);
                __syncthreads();
                K5T(8);
                // d. terms, one (candidate, column) item per lane over the wave's slots
                {
                // the wave's items (first hits of whole columns; the owner carries a split column),
                // compacted so the terms run on dense lanes
                // (in place: an item is written at or below the slot it was read from, after the read)
                uint16_t* wit = item + wb;
                uint32_t ni = 0;
                for (uint32_t r0 = wb; r0 < wb + wn; r0 += 64) {
                    const uint32_t r = r0 + (uint32_t)lane;
                    const uint32_t run = r < wb + wn ? (uint32_t)item[r] : 0u;
                    const bool is = run != 0u;
                    const uint64_t bal = __ballot(is);
                    wave_sync();
                    if (is) wit[ni + (uint32_t)__popcll(bal & low_bits((uint32_t)lane))] = (uint16_t)(r | run << kItemRunShift);
                    ni += (uint32_t)__popcll(bal);
                }
                wave_sync();
                for (uint32_t i = (uint32_t)lane; i < ni; i += 64) {
                    const uint32_t it = wit[i];
                    const uint32_t r = it & kItemSlotMask, run = it >> kItemRunShift;
                    const uint32_t h = hit[r];
                    const uint32_t jr = (h >> 8) & 63u, sg = seg[jr];
                    const int t = (int)((sg >> 16) & 0xFFu);
                    const double nrm = slot[r];
                    double dot = tok_product(pt, ja + (int)jr, h & 0xFFu);
                    if (run < kItemRunMax) {
                        dot = run_dot(slot, r, run, dot);  // the column's further hits, tid ascending
                    } else {  // a long run (>= kItemRunMax hits): walk it by the hit flags
                        const uint32_t hi = (sg >> 8) & 0xFFu;
                        for (uint32_t r2 = r + 1; r2 < wb + wn; ++r2) {
                            const uint32_t h2 = hit[r2];
                            const uint32_t j2 = (h2 >> 8) & 63u;
                            if ((h2 & kHitCand) || j2 >= hi) break;
                            dot += slot[r2];
                        }
                    }
                    slot[r] = dot == 0.0 ? q.sig0_col[t] : text_term(q, t, dot, nrm);
                }
                }
                wave_sync();
                K5T(9);
            }
            // e. the owners add the round's common columns in ascending order (the candidate's
            // columns among the round's: ~3 per round instead of every round column)
            const uint64_t rtm = cpre[R.ce] & ~cpre[R.ca];  // the round's columns, by column number
            // the round's split columns (<= 2, the only ones not wholly inside it): its first if that
            // began in an earlier round, its last if that goes on past it (column numbers, or -1)
            int t_in = -1, t_on = -1;
            if (R.ce > R.ca) {
                const QCol cf = scol[R.ca], cl = scol[R.ce - 1];
                if (cf.j0 < ja) t_in = cf.t;
                if (cl.j1 > jb) t_on = cl.t;
            }
#pragma unroll
            for (int kk = 0; kk < kCandsPerThread; ++kk) {
                const int p = kk * kPostThreads + tid;
                // the candidate's hits lie in its common columns only, in ascending token order: the
                // remaining mask and a running slot index walk them column by column
                uint64_t mr = F > 0 ? mask[p] : 0ull;
                uint32_t rr = F > 0 ? hbase[p] : 0u;
                for (uint64_t pr = pend[kk] & rtm; pr; pr &= pr - 1) {
                    const int t = __ffsll((unsigned long long)pr) - 1;
                    const uint64_t lm = lmk[t];  // (stale in an empty round: mr is 0 there)
                    const uint64_t h = mr & lm;
                    mr &= ~lm;
                    const uint32_t r0 = rr;
                    rr += (uint32_t)__popcll(h);
                    if (t != t_in && t != t_on) {
                        sum[kk] += h ? slot[r0] : q.sig0_col[t];
                        continue;
                    }
                    // split column (rare): the dot over its segments in ascending order
                    if (h) {
                        uint64_t v = h;
                        uint32_t r = r0;
                        while (v) {
                            const int jr = __ffsll((unsigned long long)v) - 1;
                            v &= v - 1;
                            cdot[kk] += tok_product(pt, ja + jr, hit[r++] & 0xFFu);
                        }
                        cnrm[kk] = slot[r0];
                        chit |= 1u << kk;
                    }
                    if (t != t_on) {
                        const bool hh = (chit >> kk) & 1u;
                        sum[kk] += (hh && cdot[kk] != 0.0) ? text_term(q, t, cdot[kk], cnrm[kk]) : q.sig0_col[t];
                        cdot[kk] = 0.0;
                        chit &= ~(1u << kk);
                    }
                }
                if (F > 0) mask[p] = 0ull;
            }
            // f. the bound again with the round's terms in: still to come are the pending columns past
            // the round, a split column that goes on (t_on) among them
            if (prune_rnd && rnd + 1 < nrounds) {
                const uint64_t togo = ~(cpre[R.ce] & ~(t_on >= 0 ? 1ull << t_on : 0ull));
#pragma unroll
                for (int kk = 0; kk < kCandsPerThread; ++kk) {
                    const bool d = !((skip >> kk) & 1u) &&
                                   prune_dead(sum[kk], (double)__popcll(pend[kk] & togo), need[(used >> (8 * kk)) & 0xFFu]);
                    if (d) {
                        skip |= 1u << kk;
                        pend[kk] = 0ull;
                    }
                    if (pstats) {
                        const uint64_t bal = __ballot(d);
                        if (lane == 0) atomicAdd(&misc[10], (uint32_t)__popcll(bal));
                    }
                }
            }
            K5T(10);
            if (F == 0 && rnd + 1 < nrounds) {  // an empty round built no list map for the next one
                if (tid < 64) {
                    const uint2 r1 = rtab[rnd + 1];
                    const int nb = mbuf ^ 1;
                    build_map(mapb + nb * kMapWords, mapc + nb * kMapWords, mapn + nb * kRoundToks, gpre, rng,
                              (int)(r1.x & 0xFFFFu), (int)(r1.x >> 16), lane);
                }
                __syncthreads();
            }
            if (F > 0) __syncthreads();  // the next round rewrites the masks, slots and segments
        }
        K5T(11);
        // 5. FAS (recommender_similarity.cpp:114-123) and the wave top-k
        uint64_t keys[kCandsPerThread];
#pragma unroll
        for (int kk = 0; kk < kCandsPerThread; ++kk) {
            uint64_t key = ~0ull;
            if (!((skip >> kk) & 1u)) {
                const int uk = (int)((used >> (8 * kk)) & 0xFFu);
                const float f = fas_score(sum[kk], uk, ftab[uk]);  // (double)uk / (double)(kNumFixed + q.n_cols)
                // keyed by idx (idx order = uid order); uids are filled in before the merge
                key = score_key(f, (int32_t)(c0 + kk * kPostThreads + tid));
                if constexpr (WIN) {
                    if (!window_pass(key, *wl)) key = ~0ull;
                }
            }
            keys[kk] = key;
        }
        if constexpr (WIN) {
            if (wl->fields & kWinCount) {  // the wave's keys in the window, one LDS add
                const uint32_t nin = (uint32_t)__popcll(__ballot(keys[0] != ~0ull)) + (uint32_t)__popcll(__ballot(keys[1] != ~0ull));
                if (lane == 0 && nin != 0u) atomicAdd(&misc[6], nin);
            }
            // a collecting launch keeps the block's in-window keys, with the uid in the id word (the
            // header word the tail's idx -> uid step reads): the buffer holds uid keys whoever filled it
            if (wl->fields & kWinCollect) {
                uint64_t ck[kCandsPerThread];
#pragma unroll
                for (int kk = 0; kk < kCandsPerThread; ++kk) {
                    ck[kk] = keys[kk];
                    if (ck[kk] != ~0ull) {
                        const uint32_t idx = (uint32_t)ck[kk] ^ 0x80000000u;
                        ck[kk] = (ck[kk] & 0xFFFFFFFF00000000ull) | (ps.hdr[2 * (size_t)idx + 1].w ^ 0x80000000u);
                    }
                }
                collect_append(ck[0], ck[1], &sync[qy].ccursor, cbuf, ccap, lane);
            }
        }
        // the lane's 2 keys ascending, then pushed best-first: after the first push the
        // wave's threshold rejects most of the rest
        static_assert(kCandsPerThread == 2, "2-key sort");
        if (keys[1] < keys[0]) { const uint64_t x = keys[0]; keys[0] = keys[1]; keys[1] = x; }
#pragma unroll
        for (int kk = 0; kk < kCandsPerThread; ++kk) topk_push(best, keys[kk], k, lane);
        // 6. the block's best survivor becomes the workgroup's record (sent at the next block's start)
        // (a counted launch records nothing: its theta stays at the window's seed)
        if (prune && !(WIN && (wl->fields & kWinCount))) prune_fold(&misc[5], best, k, c0, c1, misc[4], lane);
        K5T(12);
#ifdef PF_K5_BLOCKLOG
        if (tid == 0) {
            const unsigned i = atomicAdd(&g_blog_n, 1u);
            if (i < kBlogCap) {
                g_blog_t[2 * i] = blog_t0;
                g_blog_t[2 * i + 1] = __builtin_amdgcn_s_memrealtime();
                g_blog_meta[i] = (unsigned)bx | (unsigned)blk << 16;
            }
        }
#endif
        next_block(false);
    }
    // The record of the workgroup's last block has no next block to send it: the deriving wave's
    // first lane sends it here (the other workgroups of the query still derive from it) and waits
    // for the add's return, so it has arrived before the tail's barrier, hence before this
    // workgroup's ticket and before the query's last workgroup zeroes the ScanSync.
    if (prune && tid == kPostThreads - 64) {
        const uint32_t rec = misc[5];  // (folded before the last block's closing barrier)
        if (rec != 0u) {
            const uint32_t old = __hip_atomic_fetch_add(&sync[qy].hist[prune_bin(rec)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(old));
        }
    }
#ifdef PF_K5_TIMERS
    tacc[13] = clock64() - tstart;
    if (lane == 0) {
        for (int i = 0; i < 14; ++i) atomicAdd(&g_k5t[i], (unsigned long long)tacc[i]);
        atomicAdd(&g_k5t[15], 1ull);
    }
#endif
    if (pstats) {  // a few atomics per workgroup per launch
        __syncthreads();
        if (tid < kPruneStats) atomicAdd(&g_k5_prune[tid], (unsigned long long)misc[8 + tid]);
    }
    // idx -> uid in the wave's list (the same order: uid ascending == idx ascending)
    if (lane < k && best != ~0ull) {
        const uint32_t idx = (uint32_t)best ^ 0x80000000u;
        best = (best & 0xFFFFFFFF00000000ull) | (ps.hdr[2 * (size_t)idx + 1].w ^ 0x80000000u);
    }
    // tail scratch in the (idle) slots: merge keys, then flag / threshold / block ids
    uint64_t* sc = reinterpret_cast<uint64_t*>(slot);

    if constexpr (WIN) {
        // misc[6] is complete: its adds came before each block's closing barrier.  (The tail's scratch is
        // the slots, not misc.)
        const bool counted = (wl->fields & kWinCount) != 0u;
        post_tail(best, k, sc, sync, parts, out, out_rows, qy, bx, nbx, counted, tid == 0 ? misc[6] : 0u, totals);
    } else {
        post_tail(best, k, sc, sync, parts, out, out_rows, qy, bx, nbx);
    }
}

// ---------------------------------------------------------------- K2: merge
// Key lists in[part * part_stride + q * query_stride + j] (j < k) -> out[q * k + j]
// (the cross-shard merge after the all-gather; one block per query, every wave pushes
// its share of the keys, then wave 0 merges the wave lists).
constexpr int kMergeThreads = 1024;
__global__ __launch_bounds__(kMergeThreads) void topk_merge_kernel(const uint64_t* __restrict__ in, int32_t nparts,
                                                                   int64_t part_stride, int64_t query_stride, int32_t k,
                                                                   uint64_t* __restrict__ out,
                                                                   const int32_t* __restrict__ out_rows) {
    __shared__ uint64_t sc[16 * 64];
    const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = (int64_t)nparts * k;
    uint64_t list = ~0ull;
    for (int64_t base = 0; base < total; base += (int64_t)blockDim.x * 8) {
        uint64_t x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t i = base + (int64_t)u * blockDim.x + threadIdx.x;
            x[u] = ~0ull;
            if (i < total) {
                const int32_t part = (int32_t)(i / k), j = (int32_t)(i - (int64_t)part * k);
                x[u] = in[(int64_t)part * part_stride + q * query_stride + j];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) topk_push(list, x[u], k, lane);
    }
    if (lane < k) sc[wave * k + lane] = list;
    __syncthreads();
    if (wave == 0) {
        uint64_t acc = ~0ull;
        const int n = (int)(blockDim.x >> 6) * k;
        for (int b = 0; b < n; b += 64) topk_push(acc, b + lane < n ? sc[b + lane] : ~0ull, k, lane);
        const int row = out_rows ? out_rows[q] : q;
        if (lane < k) out[(size_t)row * k + lane] = acc;
    }
}

// ---------------------------------------------------------------- K1': pairs
#ifdef PF_K1P_WPE  // experiment builds: waves per SIMD the pair kernel's registers are sized for
#define PF_K1P_BOUNDS __launch_bounds__(kPairThreads) __attribute__((amdgpu_waves_per_eu(PF_K1P_WPE, PF_K1P_WPE)))
#else
#define PF_K1P_BOUNDS __launch_bounds__(kPairThreads, 4)
#endif
template <bool PACKED, bool GTAB>
__global__ PF_K1P_BOUNDS void fas_pairs_kernel(DevStore st, const uint8_t* __restrict__ pool,
                                                        const QImageRef* __restrict__ refs,
                                                        const PairBlock* __restrict__ blocks,
                                                        const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ slots, float* __restrict__ out,
                                                        FieldSel S) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef PF_K5_TIMERS
    const uint64_t t0 = clock64();
    uint64_t tw[4] = {0, 0, 0, 0};
    uint64_t* twp = tw;
#else
    uint64_t* twp = nullptr;
#endif
    const PairBlock b = blocks[order ? order[blockIdx.x] : (int)blockIdx.x];
    // a block scores b.count <= kPairThreads pairs against its one staged image; the plan sizes
    // candidate blocks by the candidate bound, so a block past a job's candidates has none
    const int i = (int)threadIdx.x;
    int p = i < b.count ? slots[b.begin + i] : -1;
    const bool active = p >= 0;
    if (!__syncthreads_or(active)) return;
    const PairHdr H = load_pair_hdr(st, p, active);
    char* scratch;
    const QView v = stage_query<GTAB>(smem, pool, refs[b.qimg], &scratch, S);
#ifdef PF_K5_TIMERS
    const uint64_t t1 = clock64();
#endif
    const float f = fas_slot<PACKED>(st, v, H, active, twp);
    if (active) out[b.out + i] = f;
#ifdef PF_K5_TIMERS
    const uint64_t t3 = clock64();
    // the wave's phase ends: the walk is wave-uniform; the epilogue's phases end at the wave's
    // last lane (max over the lanes that ran it)
    // (the epilogue's clocks are taken by every lane at wave-uniform points: lane 0's are the wave's)
    uint64_t we = tw[0], fe = tw[1], he = tw[2], oe = tw[3];
    we = (uint64_t)__shfl((long long)we, 0);
    fe = (uint64_t)__shfl((long long)fe, 0);
    he = (uint64_t)__shfl((long long)he, 0);
    oe = (uint64_t)__shfl((long long)oe, 0);
    if (fe == 0) fe = we;
    if (he == 0) he = fe;
    if (oe == 0) oe = he;
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&g_k1t[0], (unsigned long long)(t1 - t0));
        atomicAdd(&g_k1t[1], (unsigned long long)(we - t1));
        atomicAdd(&g_k1t[2], (unsigned long long)(t3 - we));
        atomicAdd(&g_k1t[3], (unsigned long long)(t3 - t0));
        atomicAdd(&g_k1t[4], (unsigned long long)(fe - we));
        atomicAdd(&g_k1t[5], (unsigned long long)(he - fe));
        atomicAdd(&g_k1t[6], (unsigned long long)(oe - he));
        atomicAdd(&g_k1t[8], (unsigned long long)(t3 - oe));
        atomicAdd(&g_k1t[7], 1ull);
    }
#endif
}

// ---------------------------------------------------------------- filter count
// Candidates [i0, i1) that pass F: postings headers (POST; idx order) or tile headers (slot order).
// A block reduction (a wave scan of the lanes' counts, then the waves' sums through LDS) and one
// atomic add per workgroup.
constexpr int kCountThreads = 256;
template <bool POST>
__global__ __launch_bounds__(kCountThreads) void filter_count_kernel(const uint4* __restrict__ hdr, const uint4* __restrict__ hdr1,
                                                                     const uint4* __restrict__ hdr2, int32_t i0, int32_t i1,
                                                                     CandFilter F, unsigned long long* __restrict__ count) {
    __shared__ uint32_t wsum[kCountThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t n = 0;
    for (int64_t i = (int64_t)i0 + (int64_t)blockIdx.x * kCountThreads + threadIdx.x; i < i1;
         i += (int64_t)gridDim.x * kCountThreads) {
        bool ok;
        if (POST) ok = filter_pass_post(F, hdr[2 * i], hdr[2 * i + 1]);
        else ok = filter_pass_tile(F, hdr[i], hdr1[i], hdr2[i]);
        n += ok ? 1u : 0u;
    }
    n = wave_last(wave_incl_scan(n));
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kCountThreads / 64; ++w) t += wsum[w];
        if (t) atomicAdd(count, (unsigned long long)t);
    }
}

// ---------------------------------------------------------------- launchers
hipError_t launch_filter_count(const PostStore& ps, const DevStore& st, int32_t i0, int32_t i1, const CandFilter& filt,
                               unsigned long long* count, hipStream_t s) {
    if (i1 <= i0) return hipSuccess;
    const int blocks = std::max(1, std::min(1024, (i1 - i0 + kCountThreads - 1) / kCountThreads));
    if (ps.hdr)
        hipLaunchKernelGGL(filter_count_kernel<true>, dim3(blocks), dim3(kCountThreads), 0, s, ps.hdr, (const uint4*)nullptr,
                           (const uint4*)nullptr, i0, i1, filt, count);
    else
        hipLaunchKernelGGL(filter_count_kernel<false>, dim3(blocks), dim3(kCountThreads), 0, s, st.hdr0, st.hdr1, st.hdr2, i0,
                           i1, filt, count);
    return hipGetLastError();
}

// The instantiation a launch's run-time choice names, one function per kernel template: the launch
// and the occupancy query both ask it, so they cannot disagree, and a new template parameter is one
// more dimension of its table.
using ScanKernel = decltype(&fas_scan_kernel<false, false>);
static ScanKernel scan_kernel(bool packed, bool gtab) {
    static constexpr ScanKernel tab[2][2] = {{fas_scan_kernel<false, false>, fas_scan_kernel<false, true>},
                                             {fas_scan_kernel<true, false>, fas_scan_kernel<true, true>}};
    return tab[packed][gtab];
}
using PairsKernel = decltype(&fas_pairs_kernel<false, false>);
static PairsKernel pairs_kernel(bool packed, bool gtab) {
    static constexpr PairsKernel tab[2][2] = {{fas_pairs_kernel<false, false>, fas_pairs_kernel<false, true>},
                                              {fas_pairs_kernel<true, false>, fas_pairs_kernel<true, true>}};
    return tab[packed][gtab];
}
using PostKernel = decltype(&fas_post_kernel<false, false, false, false>);
static PostKernel post_kernel(bool claimed, bool filtered, bool selected, bool windowed) {
#define PF_POST_ROW(XD, FILT, SEL) {fas_post_kernel<XD, FILT, SEL, false>, fas_post_kernel<XD, FILT, SEL, true>}
    static constexpr PostKernel tab[2][2][2][2] = {
        {{PF_POST_ROW(false, false, false), PF_POST_ROW(false, false, true)},
         {PF_POST_ROW(false, true, false), PF_POST_ROW(false, true, true)}},
        {{PF_POST_ROW(true, false, false), PF_POST_ROW(true, false, true)},
         {PF_POST_ROW(true, true, false), PF_POST_ROW(true, true, true)}}};
#undef PF_POST_ROW
    return tab[claimed][filtered][selected][windowed];
}

hipError_t launch_scan(const ScanLaunch& L) {
    if (L.nq <= 0) return hipSuccess;
    if (!extras_ok(L.x, L.nq)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_kernel(L.st.packed, L.gtab), dim3(L.blocks, L.nq), dim3(kScanThreads), L.lds, L.s, L.st, L.pool,
                       L.refs_dev, L.tile_begin, L.tile_end, L.k, L.parts, L.sync, L.out, L.out_rows, L.x.filt, L.x.sel, L.x.win, L.x.totals,
                       L.x.collect, L.x.collect_cap);
    return hipGetLastError();
}

int scan_blocks_per_cu(bool packed, bool gtab, uint32_t lds) {
    // the answer depends only on (variant, LDS bytes): cache it, the query is not free
    static thread_local uint64_t last_key = ~0ull;
    static thread_local int last_nb = 1;
    const uint64_t key = ((uint64_t)lds << 2) | ((uint64_t)packed << 1) | (uint64_t)gtab;
    if (key == last_key) return last_nb;
    int nb = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, scan_kernel(packed, gtab), kScanThreads, lds);
    last_key = key;
    last_nb = (e == hipSuccess && nb > 0) ? nb : 1;
    return last_nb;
}

// K5 dynamic LDS: QConst | fixed per-block arrays | PTok[n_tok] | PList[n_lists] | ranges[n_lists] |
// rounds[n_tok + 1] | token prefix[n_tok + 1] | set prefix[n_sets + 1] | token -> column u8[n_tok]
uint32_t post_var_lds(int n_tok, int n_lists) {
    return (uint32_t)(sizeof(PTok) * n_tok + 8 * n_lists + 8 * (n_tok + 1) + 4 * (n_tok + 1) +
                      4 * (n_lists - n_tok + 1) + n_tok + 15) & ~15u;
}
uint32_t post_lds(uint32_t var_lds) { return (uint32_t)sizeof(QConst) + kPostFixedLds + var_lds; }

#ifdef PF_K5_BLOCKLOG
// per-block times of one launch: the span, and per nbx consecutive blocks (blk / nbx: one-query
// launches claim their blocks, so these are ranges of the block index, not rounds in time) the
// blocks' start and end offsets and durations (us, from the launch's first block start)
static void blog_report(int nbx) {
    static unsigned long long t[2 * kBlogCap];
    static unsigned int meta[kBlogCap];
    unsigned int n = 0;
    hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_blog_n), sizeof n);
    n = n < kBlogCap ? n : kBlogCap;
    hipMemcpyFromSymbol(t, HIP_SYMBOL(g_blog_t), 2 * n * sizeof(unsigned long long));
    hipMemcpyFromSymbol(meta, HIP_SYMBOL(g_blog_meta), n * sizeof(unsigned));
    unsigned long long t0 = ~0ull, t1 = 0;
    for (unsigned i = 0; i < n; ++i) { t0 = t[2 * i] < t0 ? t[2 * i] : t0; t1 = t[2 * i + 1] > t1 ? t[2 * i + 1] : t1; }
    fprintf(stderr, "k5blog: %u blocks, span %.1f us\n", n, (t1 - t0) / 100.0);
    static int dumps = 0;
    if (const char* path = getenv("PF_BLOG_OUT"); path && dumps++ < 3) {  // raw rows: wg blk start end (us)
        char fn[512];
        snprintf(fn, sizeof fn, "%s.%d.csv", path, dumps);
        if (FILE* f = fopen(fn, "w")) {
            for (unsigned i = 0; i < n; ++i)
                fprintf(f, "%u,%u,%.2f,%.2f\n", meta[i] & 0xFFFFu, meta[i] >> 16, (t[2 * i] - t0) / 100.0,
                        (t[2 * i + 1] - t0) / 100.0);
            fclose(f);
        }
    }
    for (int r = 0; r < 8; ++r) {
        std::vector<double> d, st, en;
        for (unsigned i = 0; i < n; ++i) {
            const int blk = (int)(meta[i] >> 16);
            if (blk / nbx != r) continue;
            d.push_back((t[2 * i + 1] - t[2 * i]) / 100.0);
            st.push_back((t[2 * i] - t0) / 100.0);
            en.push_back((t[2 * i + 1] - t0) / 100.0);
        }
        if (d.empty()) continue;
        std::sort(d.begin(), d.end()); std::sort(st.begin(), st.end()); std::sort(en.begin(), en.end());
        auto pc = [](const std::vector<double>& v, double q) { return v[(size_t)(q * (v.size() - 1))]; };
        fprintf(stderr, "k5blog: round %d: %zu blocks, dur p10/50/90/max %.1f/%.1f/%.1f/%.1f, start min/50/max %.1f/%.1f/%.1f, end min/50/max %.1f/%.1f/%.1f\n",
                r, d.size(), pc(d, .1), pc(d, .5), pc(d, .9), d.back(), st.front(), pc(st, .5), st.back(), en.front(),
                pc(en, .5), en.back());
    }
}
#endif

hipError_t launch_post(const PostLaunch& L) {
    if (L.nq <= 0) return hipSuccess;
    // the claimed hand-out is the one-query instantiation's and nobody else's
    if (L.claimed && L.nq != 1) return hipErrorInvalidValue;
    if (!extras_ok(L.x, L.nq)) return hipErrorInvalidValue;
    // + the filter's and the window's words (fas_post_kernel)
    const uint32_t lds = post_lds(L.var_lds) + (L.x.filt.fields ? kFiltLds : 0u) + (L.x.win.fields ? kWinLds : 0u);
    // timed launches (e0, e1 given): the kernel's own start and end timestamps, taken from its
    // dispatch (hipExtLaunchKernelGGL), instead of two marker packets around it.  The filter and the field
    // selection travel in the launch's own arguments: a later pf_set_scan_filter / _select does not reach them
    hipExtLaunchKernelGGL(post_kernel(L.claimed, L.x.filt.fields != 0u, L.x.sel.on != 0u, L.x.win.fields != 0u), dim3(L.blocks, L.nq), dim3(kPostThreads),
                          lds, L.s, L.e0, L.e1, 0u, L.ps, L.pool, L.img_off, L.blk_begin, L.blk_end, L.k, L.parts, L.sync, L.out,
                          L.out_rows, L.mode, L.qconst, L.x.filt, L.x.sel, L.x.win, L.x.totals, L.x.collect, L.x.collect_cap);
#ifdef PF_K5_BLOCKLOG
    {
        static int calls = 0;
        hipStreamSynchronize(L.s);
        if (++calls % 10 == 0 && L.nq == 1) blog_report(L.blocks);
        const unsigned zero = 0;
        hipMemcpyToSymbol(HIP_SYMBOL(g_blog_n), &zero, sizeof zero);
    }
#endif
#ifdef PF_K5_TIMERS
    {
        static int calls = 0;
        unsigned long long t[16];
        hipStreamSynchronize(L.s);
        hipMemcpyFromSymbol(t, HIP_SYMBOL(g_k5t), sizeof(t));
        static const char* nm[14] = {"ranges+hdr", "barriers", "excl+sets", "fixed", "walk", "walk-bar",
                                     "slots", "place", "place-bar", "terms", "owner-add", "rounds-end", "fas+topk",
                                     "total"};
        if (++calls % 10 == 0) {
            fprintf(stderr, "k5t per wave (clock64):");
            for (int i = 0; i < 14; ++i) fprintf(stderr, " %s=%.0f", nm[i], (double)t[i] / (double)t[15]);
            fprintf(stderr, "\n");
        }
        const unsigned long long z[16] = {0};
        hipMemcpyToSymbol(HIP_SYMBOL(g_k5t), z, sizeof(z));
    }
#endif
    return hipGetLastError();
}

hipError_t k5_prune_stats_read(unsigned long long* out, bool reset) {
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_k5_prune), kPruneStats * sizeof(unsigned long long));
    if (e == hipSuccess && reset) {
        const unsigned long long z[kPruneStats] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_k5_prune), z, sizeof(z));
    }
    return e;
}

int post_blocks_per_cu(uint32_t var_lds, bool claimed, bool filtered, bool selected, bool windowed) {
    // per thread, by instantiation (the one launch_post takes for `claimed`, the filter and the
    // selection) and LDS bytes (a batch asks once per query: the occupancy API once per size)
    static thread_local std::unordered_map<uint32_t, int> memos[16];
    auto& memo = memos[8 * (int)windowed + 4 * (int)selected + 2 * (int)filtered + (int)claimed];
    auto it = memo.find(var_lds);
    if (it != memo.end()) return it->second;
    int nb = 0;
    const size_t lds = post_lds(var_lds) + (filtered ? kFiltLds : 0u) + (windowed ? kWinLds : 0u);
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, post_kernel(claimed, filtered, selected, windowed), kPostThreads, lds);
    nb =(e == hipSuccess && nb > 0) ? nb : 1;
    if (memo.size() > 4096) memo.clear();
    memo.emplace(var_lds, nb);
    return nb;
}

hipError_t launch_merge(const uint64_t* in, int nparts, int64_t part_stride, int64_t query_stride, int nq, int k,
                        uint64_t* out, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(nq), dim3(kMergeThreads), 0, s, in, nparts, part_stride, query_stride,
                       k, out, (const int32_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_pairs(const PairsLaunch& L) {
    if (L.nblocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(pairs_kernel(L.st.packed, L.gtab), dim3(L.nblocks), dim3(kPairThreads), L.max_lds, L.s, L.st, L.pool,
                       L.refs_dev, L.blocks, L.order, L.slots, L.out, L.sel);
#ifdef PF_K5_TIMERS
    {
        static int calls = 0;
        unsigned long long t[12];
        hipStreamSynchronize(L.s);
        hipMemcpyFromSymbol(t, HIP_SYMBOL(g_k1t), sizeof(t));
        if (++calls % 10 == 0 && t[7] && t[11])
            fprintf(stderr, "k1pt epilogue: fallback waves %.3f, items per lane %.2f\n", (double)t[9] / t[11],
                    (double)t[10] / (64.0 * t[11]));
        if (calls % 10 == 0 && t[7])
            fprintf(stderr,
                    "k1pt per wave (clock64): staging=%.0f walk=%.0f epilogue=%.0f (dense=%.0f assembly=%.0f "
                    "overflow=%.0f fas=%.0f) total=%.0f waves=%llu blocks=%d\n",
                    (double)t[0] / t[7], (double)t[1] / t[7], (double)t[2] / t[7], (double)t[4] / t[7],
                    (double)t[5] / t[7], (double)t[6] / t[7], (double)t[8] / t[7], (double)t[3] / t[7], t[7], L.nblocks);
        const unsigned long long z[12] = {0};
        hipMemcpyToSymbol(HIP_SYMBOL(g_k1t), z, sizeof(z));
    }
#endif
    return hipGetLastError();
}

}  // namespace pf

// ---------------------------------------------------------------- group scan (pf_recommend_group)
// fas_group_kernel and launch_group: a sibling of K1 built from the pieces above, in a file of its own
#include "pf_group_kernel.h"
