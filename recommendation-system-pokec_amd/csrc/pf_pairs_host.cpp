// pf_pairs_host.cpp — the pair kernels' host side: pairs grouped by their query (pf_pair_groups.h) go
// to the GPU in chunks, each distinct query's image built once per chunk; run_pairs scores them (K1'),
// run_pair_terms breaks them down (K1t).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <vector>

#include "pf_batch.h"
#include "pf_ctx.h"
#include "pf_host.h"
#include "pf_kernels.h"
#include "pf_store.h"
#include "pokec_fas.h"

namespace pf {

namespace {

// One chunk of pair groups as its kernel finds it: the images in c->d_pool / d_refs, the candidate
// slots in c->d_slots (group g0 + i's from gf[i]; gf[g1 - g0] = npairs) and the pair blocks in
// c->d_blocks, all queued on the context's stream.
struct PairChunk {
    size_t g0, g1;
    const std::vector<size_t>& gf;
    size_t npairs;
    const Images& im;
    int nblocks;
    pf::HpLap& hl;
};

// Pairs (A = qidx[g], B = slots[g][j]) of every group g, to the GPU in chunks (<= 4096 distinct
// queries, <= max_pairs pairs per launch); each distinct query's image is built once per chunk, on host
// threads.  A group's pairs are cut into blocks of block_pairs (a PairBlock's count).  run(chunk)
// launches the chunk's kernel, fetches its results and synchronises the stream before it returns
// (the pinned buffers are reused by the next chunk).
// pv (optional): the A side of every group is this by-value profile, not a stored user (qidx then
// only groups the pairs); its image is built by the same builder and staged in the same pool.
template <class Run>
int pair_chunks(pf_ctx* c, const std::vector<int32_t>& qidx, const std::vector<std::vector<int32_t>>& slots,
                uint32_t block_pairs, size_t max_pairs, const pf::ProfileView* pv, Run&& run) {
    size_t g0 = 0;
    while (g0 < qidx.size()) {
        // chunk [g0, g1)
        std::unordered_map<int32_t, int32_t> img_of;
        std::vector<int32_t> uq;
        size_t g1 = g0, pairs = 0;
        for (; g1 < qidx.size(); ++g1) {
            if (slots[g1].empty()) continue;
            const bool fresh = !img_of.count(qidx[g1]);
            if (g1 > g0 && ((fresh && uq.size() >= 4096) || pairs + slots[g1].size() > max_pairs)) break;
            if (fresh) {
                img_of.emplace(qidx[g1], (int32_t)uq.size());
                uq.push_back(qidx[g1]);
            }
            pairs += slots[g1].size();
        }
        if (pairs == 0) { g0 = g1; continue; }
        std::vector<pf::QImageHost> qi(uq.size());
        std::vector<uint8_t> ok(uq.size(), 1);
        pf::HpLap hl;
        {
            const int th = (int)std::min<size_t>(16, std::max<size_t>(1, uq.size() / 16));
            std::vector<std::thread> ts;
            for (int w = 0; w < th; ++w)
                ts.emplace_back([&, w]() {
                    for (size_t i = (size_t)w; i < uq.size(); i += (size_t)th)
                        ok[i] = (pv ? pf::build_query(c->hc, c->hs.packed, *pv, nullptr, qi[i])
                                    : pf::build_query(c->hc, c->hs.packed, uq[i], nullptr, qi[i])) ? 1 : 0;
                });
            for (auto& t : ts) t.join();
        }
        for (uint8_t x : ok)
            if (!x) return c->fail(PF_EUNSUPP, "query hash table too large");
        hl.lap(pf::kHpImages);
        Images im;
        std::vector<pf::PairBlock> blocks;
        const size_t pool_bytes = plan_images(im, qi);
        // per group: first block and first pair (serial, O(groups)); then the copies on threads
        std::vector<size_t> gb(g1 - g0 + 1), gf(g1 - g0 + 1);
        for (size_t g = g0; g < g1; ++g) {
            gb[g - g0 + 1] = gb[g - g0] + (slots[g].size() + block_pairs - 1) / block_pairs;
            gf[g - g0 + 1] = gf[g - g0] + slots[g].size();
        }
        const size_t npairs = gf.back();
        HIPCHK(c, c->h_pool.ensure(pool_bytes));
        HIPCHK(c, c->h_slots.ensure(npairs * sizeof(int32_t)));
        fill_images(im, qi, c->h_pool.as<uint8_t>(), pool_bytes);
        blocks.resize(gb.back());
        int32_t* flat = c->h_slots.as<int32_t>();
        par_jobs(g1 - g0, [&](size_t i) {
            const size_t g = g0 + i;
            if (slots[g].empty()) return;
            const int32_t img = img_of.at(qidx[g]);
            std::memcpy(flat + gf[i], slots[g].data(), slots[g].size() * sizeof(int32_t));
            for (size_t b = 0, x = gb[i]; b < slots[g].size(); b += block_pairs, ++x)
                blocks[x] = pf::PairBlock{img, (int32_t)(gf[i] + b), (int32_t)std::min<size_t>(block_pairs, slots[g].size() - b),
                                           (int32_t)(gf[i] + b)};
        }, 256);
        hl.lap(pf::kHpPack);
        // pinned buffers: async copies; they are reused only after this chunk's synchronize
        HIPCHK(c, c->d_pool.ensure(std::max<size_t>(pool_bytes, 16)));
        HIPCHK(c, hipMemcpyAsync(c->d_pool.p, c->h_pool.p, pool_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, upload(c, c->d_refs, im.refs));
        HIPCHK(c, upload(c, c->d_blocks, blocks));
        HIPCHK(c, c->d_slots.ensure(npairs * sizeof(int32_t)));
        HIPCHK(c, hipMemcpyAsync(c->d_slots.p, flat, npairs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        const int rc = run(PairChunk{g0, g1, gf, npairs, im, (int)blocks.size(), hl});
        if (rc != PF_OK) return rc;
        g0 = g1;
    }
    return PF_OK;
}

}  // namespace

int run_pairs(pf_ctx* c, const std::vector<int32_t>& qidx, const std::vector<std::vector<int32_t>>& slots,
              std::vector<std::vector<float>>& out, DBuf* keep, std::vector<int64_t>* goff, const pf::FieldSel& sel,
              const pf::ProfileView* pv) {
    out.assign(qidx.size(), {});
    if (keep) {
        size_t tot = 0;
        goff->assign(qidx.size(), 0);
        for (size_t g = 0; g < qidx.size(); ++g) {
            (*goff)[g] = (int64_t)tot;
            tot += slots[g].size();
        }
        HIPCHK(c, keep->ensure(std::max<size_t>(tot, 1) * sizeof(float)));
    }
    for (size_t g = 0; g < qidx.size(); ++g) out[g].assign(slots[g].size(), 0.f);
    return pair_chunks(c, qidx, slots, (uint32_t)kPairThreads, (size_t)8u << 20, pv, [&](const PairChunk& k) -> int {
        HIPCHK(c, c->h_scores.ensure(k.npairs * sizeof(float)));
        float* dsc = nullptr;
        if (keep) {
            dsc = keep->as<float>() + (*goff)[k.g0];  // groups are laid out in order, chunk after chunk
        } else {
            HIPCHK(c, c->d_scores.ensure(k.npairs * sizeof(float)));
            dsc = c->d_scores.as<float>();
        }
        HIPCHK(c, pf::launch_pairs({.st = c->ds, .pool = c->d_pool.as<uint8_t>(), .refs_dev = c->d_refs.as<pf::QImageRef>(),
                                    .max_lds = k.im.max_lds, .gtab = k.im.gtab, .blocks = c->d_blocks.as<pf::PairBlock>(),
                                    .nblocks = k.nblocks, .order = nullptr, .slots = c->d_slots.as<int32_t>(),
                                    .out = dsc, .s = c->stream, .sel = sel}));
        c->jb.n_dispatch += k.nblocks != 0;  // pf_jobs_stats.pair_dispatches counts every K1' dispatch
        const float* res = c->h_scores.as<float>();
        HIPCHK(c, hipMemcpyAsync(c->h_scores.p, dsc, k.npairs * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        k.hl.lap(pf::kHpGpu);
        par_jobs(k.g1 - k.g0, [&](size_t i) {
            const size_t g = k.g0 + i;
            if (!slots[g].empty()) std::memcpy(out[g].data(), res + k.gf[i], slots[g].size() * sizeof(float));
        }, 256);
        k.hl.lap(pf::kHpUnpack);
        return PF_OK;
    });
}

// A launch's rows are kept to 256 MB (a row is up to 71 doubles where a score is one float).
int run_pair_terms(pf_ctx* c, const std::vector<int32_t>& qidx, const std::vector<std::vector<int32_t>>& slots,
                   const std::vector<std::vector<int64_t>>& dest, pf_pair_terms_head* head, double* terms,
                   const pf::FieldSel& sel, const pf::ProfileView* pv) {
    const size_t W = (size_t)(pf::kNumFixed + c->hc.T);
    const size_t max_pairs = ((size_t)256u << 20) / (W * sizeof(double));
    return pair_chunks(c, qidx, slots, (uint32_t)pf::kTermsPairs, max_pairs, pv, [&](const PairChunk& k) -> int {
        const size_t hb = k.npairs * sizeof(pf_pair_terms_head), tb = k.npairs * W * sizeof(double);
        HIPCHK(c, c->d_thead.ensure(hb));
        HIPCHK(c, c->d_terms.ensure(tb));
        HIPCHK(c, c->h_thead.ensure(hb));
        HIPCHK(c, c->h_terms.ensure(tb));
        HIPCHK(c, pf::launch_terms({.st = c->ds, .pool = c->d_pool.as<uint8_t>(), .refs_dev = c->d_refs.as<pf::QImageRef>(),
                                    .lds = (uint32_t)sizeof(pf::QConst) + k.im.max_img, .gtab = k.im.gtab,
                                    .blocks = c->d_blocks.as<pf::PairBlock>(), .nblocks = k.nblocks,
                                    .slots = c->d_slots.as<int32_t>(), .head = c->d_thead.as<pf_pair_terms_head>(),
                                    .terms = c->d_terms.as<double>(), .s = c->stream, .sel = sel}));
        HIPCHK(c, hipMemcpyAsync(c->h_thead.p, c->d_thead.p, hb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_terms.p, c->d_terms.p, tb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        k.hl.lap(pf::kHpGpu);
        const pf_pair_terms_head* rh = c->h_thead.as<pf_pair_terms_head>();
        const double* rt = c->h_terms.as<double>();
        par_jobs(k.g1 - k.g0, [&](size_t i) {
            const size_t g = k.g0 + i;
            for (size_t j = 0; j < slots[g].size(); ++j) {
                head[dest[g][j]] = rh[k.gf[i] + j];
                std::memcpy(terms + (size_t)dest[g][j] * W, rt + (k.gf[i] + j) * W, W * sizeof(double));
            }
        }, 256);
        k.hl.lap(pf::kHpUnpack);
        return PF_OK;
    });
}

}  // namespace pf
