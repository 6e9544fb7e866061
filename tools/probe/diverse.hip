// Device check of the diverse top-k stage (pf_diverse.hip; links the product's build/pf_diverse_k.o) on
// synthetic pools and pair-score matrices, against the serial loop of the definition (pokec_fas.h,
// "Diverse top-k"):
//     v_i = (double)lambda * (double)r_i - (1.0 - (double)lambda) * (double)pen_i, three rounded operations;
//     the unpicked i with the largest v, ties to the smallest position; pen_i = max(pen_i, sim[s][i]).
// uid, r and pen must be equal by their bits, value by its 64 bits.  Built with -ffp-contract=off like
// the product.
//   diverse               the cases; one line each, a summary line "S ...", then OK
//   diverse sweep         wall time of the stage alone over M and topk
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pf_diverse.h"
#include "pf_types.h"

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__);  \
            exit(2);                                                                       \
        }                                                                                  \
    } while (0)

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

// the planted rounding-visible triple (tests/diverse_ref.py): v differs from the exact value rounded once
const float kPlantedLambda = 0x1.29207ep-13f, kPlantedR = 0x1.083a24p-1f, kPlantedPen = 0x1.da95e6p-4f;
const double kPlantedValue = -0x1.da38041f99745p-4, kPlantedOnce = -0x1.da38041f99746p-4;

struct Case {
    std::string name;
    int m = 0, topk = 0;
    int64_t stride = 0;  // >= m
    float lambda = 0.5f;
    std::vector<int32_t> uid;
    std::vector<float> rel;
    std::vector<float> sim;  // m rows of stride
    bool keys = false;       // the pool as collect keys
};

struct Picks {
    std::vector<int32_t> uid, pos;
    std::vector<float> r, pen;
    std::vector<double> value;
    int64_t ties = 0, cross_wave_ties = 0;  // picks whose maximum was shared, and shared across waves
};

// the definition, serially; transposed: sim read as a column (what a wrong kernel would do)
Picks reference(const Case& c, const std::vector<float>& rel, bool transposed = false) {
    Picks p;
    const int m = c.m;
    std::vector<float> pen((size_t)m, 0.f);
    std::vector<char> picked((size_t)m, 0);
    const double dl = (double)c.lambda, om = 1.0 - dl;
    for (int t = 0; t < std::min(c.topk, m); ++t) {
        int best = -1;
        double bv = 0.0;
        int equals = 0, last_equal = -1;
        for (int i = 0; i < m; ++i) {
            if (picked[(size_t)i]) continue;
            const double a = dl * (double)rel[(size_t)i];
            const double q = om * (double)pen[(size_t)i];
            const double v = a - q;
            if (best < 0 || v > bv) { best = i; bv = v; equals = 1; last_equal = i; }
            else if (v == bv) { ++equals; last_equal = i; }
        }
        p.ties += equals > 1;
        p.cross_wave_ties += equals > 1 && (last_equal >> 6) != (best >> 6);
        p.uid.push_back(c.uid[(size_t)best]);
        p.pos.push_back(best);
        p.r.push_back(rel[(size_t)best]);
        p.pen.push_back(pen[(size_t)best]);
        p.value.push_back(bv);
        picked[(size_t)best] = 1;
        for (int i = 0; i < m; ++i) {
            const float x = transposed ? c.sim[(size_t)i * (size_t)c.stride + (size_t)best] : c.sim[(size_t)best * (size_t)c.stride + (size_t)i];
            pen[(size_t)i] = x > pen[(size_t)i] ? x : pen[(size_t)i];
        }
    }
    return p;
}

template <class T>
T* up(const std::vector<T>& v) {
    T* p = nullptr;
    CK(hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)));
    if (!v.empty()) CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

pf::DiverseWs g_ws;
struct Totals {
    int64_t cases = 0, keys = 0, plain = 0, multi_wave = 0, ties = 0, cross_wave_ties = 0, all_equal = 0, last_pos = 0, asym = 0,
            pen_kept = 0, rounding = 0, past_m = 0, lane_ends = 0;
} g_t;

bool same_bits(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

// runs the case on the device matrix d_sim (uploaded by the caller: shared by the cases of one shape)
Picks run(const Case& c, const float* d_sim) {
    std::vector<float> rel = c.rel;
    std::vector<uint64_t> hkeys;
    if (c.keys) {
        for (int i = 0; i < c.m; ++i) {
            hkeys.push_back(pf::score_key(c.rel[(size_t)i], c.uid[(size_t)i]));
            rel[(size_t)i] = pf::key_score(hkeys.back());  // what the stage decodes (-0 becomes +0)
        }
    }
    const Picks want = reference(c, rel);
    uint64_t* d_keys = c.keys ? up(hkeys) : nullptr;
    int32_t* d_uid = c.keys ? nullptr : up(c.uid);
    float* d_rel = c.keys ? nullptr : up(c.rel);
    pf::DiverseIn in{};
    in.keys = d_keys;
    in.uid = d_uid;
    in.rel = d_rel;
    in.m = c.m;
    in.sim = d_sim;
    in.stride = c.stride;
    in.lambda = c.lambda;
    in.topk = c.topk;
    const size_t cap = (size_t)std::max(c.topk, 1);
    std::vector<int32_t> ou(cap, -7), op(cap, -7);
    std::vector<float> orr(cap, -7.f), open_(cap, -7.f);
    std::vector<double> ov(cap, -7.0);
    int32_t n = -1;
    hipError_t err = hipSuccess;
    const auto t0 = std::chrono::steady_clock::now();
    const pf::DiverseStatus st = pf::diverse_run(in, g_ws, nullptr, ou.data(), orr.data(), open_.data(), ov.data(), op.data(), &n, &err);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const size_t k = want.uid.size();
    bool ok = st == pf::kDiverseOk && n == (int32_t)k;
    ok = ok && same_bits(ou.data(), want.uid.data(), k * 4) && same_bits(op.data(), want.pos.data(), k * 4) &&
         same_bits(orr.data(), want.r.data(), k * 4) && same_bits(open_.data(), want.pen.data(), k * 4) &&
         same_bits(ov.data(), want.value.data(), k * 8);
    for (size_t i = k; ok && i < cap; ++i) ok = ou[i] == -7;  // nothing past min(topk, m)
    printf("case %s m %d topk %d lambda %a %s picks %d ties %lld ms %.3f %s\n", c.name.c_str(), c.m, c.topk, (double)c.lambda,
           c.keys ? "keys" : "plain", n, (long long)want.ties, ms, ok ? "ok" : "MISMATCH");
    if (!ok) {
        printf("  status %d hip %s; want %zu picks\n", (int)st, hipGetErrorString(err), k);
        for (size_t i = 0; i < k; ++i)
            if (ou[i] != want.uid[i] || !same_bits(&ov[i], &want.value[i], 8) || !same_bits(&open_[i], &want.pen[i], 4)) {
                printf("  [%zu] got uid %d pos %d r %a pen %a v %a want uid %d pos %d r %a pen %a v %a\n", i, ou[i], op[i], (double)orr[i],
                       (double)open_[i], ov[i], want.uid[i], want.pos[i], (double)want.r[i], (double)want.pen[i], want.value[i]);
                break;
            }
        exit(1);
    }
    ++g_t.cases;
    g_t.keys += c.keys;
    g_t.plain += !c.keys;
    g_t.multi_wave += c.m > 64;
    g_t.ties += want.ties;
    g_t.cross_wave_ties += want.cross_wave_ties;
    g_t.past_m += c.topk > c.m;
    (void)hipFree(d_keys); (void)hipFree(d_uid); (void)hipFree(d_rel);
    return want;
}

Picks run(const Case& c) {
    float* d = up(c.sim);
    const Picks p = run(c, d);
    (void)hipFree(d);
    return p;
}

// uids 10, 13, 16, ...; relevances and similarities from small sets (ties in r, in pen and in v), the
// matrix not symmetric, with a stride past m whose padding would be picked up by a wrong index
Case random_case(const std::string& name, int m, uint64_t seed) {
    Case c;
    c.name = name;
    c.m = m;
    c.stride = m + 3;
    Rng g{seed};
    for (int i = 0; i < m; ++i) {
        c.uid.push_back(10 + 3 * i);
        c.rel.push_back(0.125f * (float)(1 + g.below(7)));
    }
    c.sim.assign((size_t)m * (size_t)c.stride, 7.f);
    for (int s = 0; s < m; ++s)
        for (int i = 0; i < m; ++i) c.sim[(size_t)s * (size_t)c.stride + (size_t)i] = 0.0625f * (float)g.below(15) + (g.below(8) == 0 ? 0x1p-20f : 0.f);
    return c;
}

// relevance `lo` everywhere but `hi` at the given positions; a flat matrix
Case planted(const std::string& name, int m, float lo, float hi, std::vector<int> at) {
    Case c;
    c.name = name;
    c.m = m;
    c.stride = m;
    c.topk = (int)at.size() + 1;
    c.lambda = 0.5f;
    for (int i = 0; i < m; ++i) {
        c.uid.push_back(1000 + i);
        c.rel.push_back(lo);
    }
    for (int a : at) c.rel[(size_t)a] = hi;
    c.sim.assign((size_t)m * (size_t)m, 0.25f);
    return c;
}

void fail(const char* what) {
    printf("%s: wrong reference\n", what);
    exit(1);
}

void cases() {
    const float lambdas[] = {0.f, 1.f, 0.5f, 0.7f, kPlantedLambda};
    // every shape x topk x lambda, the pool given both ways
    for (int m : {1, 2, 63, 64, 65, 128, 1023, 1024}) {
        Case c = random_case("random_" + std::to_string(m), m, 100 + (uint64_t)m);
        float* d = up(c.sim);
        const bool sym = [&] {
            for (int s = 0; s < m; ++s)
                for (int i = 0; i < s; ++i)
                    if (c.sim[(size_t)s * (size_t)c.stride + (size_t)i] != c.sim[(size_t)i * (size_t)c.stride + (size_t)s]) return false;
            return true;
        }();
        for (int topk : {1, 2, 64, m, m + 5})
            for (float l : lambdas)
                for (bool keys : {false, true}) {
                    c.topk = topk;
                    c.lambda = l;
                    c.keys = keys;
                    const Picks p = run(c, d);
                    if (!sym && !keys && l == 0.5f && topk == m) {  // a row read as a column gives another list here
                        const Picks q = reference(c, c.rel, true);
                        g_t.asym += q.uid != p.uid || !same_bits(q.value.data(), p.value.data(), p.value.size() * 8);
                    }
                    if (l == 1.f)  // lambda = 1: the pool's prefix (the relevances tie, so position decides)
                        for (size_t i = 0; i + 1 < p.pos.size(); ++i)
                            if (p.r[i] < p.r[i + 1]) fail("lambda 1");
                }
        (void)hipFree(d);
    }
    // all-equal values, the identical-users case: positions 0, 1, 2, ...
    for (int m : {65, 1024}) {
        Case c = planted("all_equal_" + std::to_string(m), m, 0.5f, 0.5f, {});
        c.topk = m;
        c.lambda = 0.7f;
        const Picks p = run(c);
        for (int i = 0; i < m; ++i)
            if (p.pos[(size_t)i] != i) fail("all_equal");
        ++g_t.all_equal;
    }
    // equal maxima in two waves: the winner in the first wave, then in the last; in the last two waves;
    // in lanes 0 and 63 of one wave
    {
        Picks p = run(planted("tie_first_last_wave", 1024, 0.125f, 0.875f, {3, 1000}));
        if (p.pos[0] != 3 || p.pos[1] != 1000 || p.pos[2] != 0 || p.cross_wave_ties < 2) fail("tie_first_last_wave");
        p = run(planted("tie_last_waves", 1024, 0.125f, 0.875f, {900, 1023}));
        if (p.pos[0] != 900 || p.pos[1] != 1023 || p.pos[2] != 0) fail("tie_last_waves");
        g_t.last_pos += 1;
        p = run(planted("tie_lanes_0_63", 256, 0.125f, 0.875f, {128, 191}));
        if (p.pos[0] != 128 || p.pos[1] != 191 || p.pos[2] != 0 || p.ties < 2) fail("tie_lanes_0_63");
        ++g_t.lane_ends;
    }
    // the winner at position M - 1
    for (int m : {2, 64, 65, 1023, 1024}) {
        const Picks p = run(planted("last_" + std::to_string(m), m, 0.25f, 0.75f, {m - 1}));
        if (p.pos[0] != m - 1) fail("last");
        ++g_t.last_pos;
    }
    // a penalty that stays at an earlier, higher value: 0 is picked, then 1; position 2 is close to 0 and far from 1
    for (bool keys : {false, true}) {
        Case c = planted("pen_kept", 3, 0.f, 0.f, {});
        c.keys = keys;
        c.rel = {0.875f, 0.75f, 0.5f};
        c.sim = {0.f, 0.125f, 0.75f,  //
                 0.5f, 0.f, 0.0625f,  // (1, 0) differs from (0, 1): column reads would give pen_1 = 0.5
                 0.f, 0.f, 0.f};
        c.topk = 3;
        const Picks p = run(c);
        if (p.pos != std::vector<int32_t>{0, 1, 2} || p.pen[1] != 0.125f || p.pen[2] != 0.75f) fail("pen_kept");
        ++g_t.pen_kept;
    }
    // the rounding-visible triple: the second pick's value is the separately rounded one
    for (bool keys : {false, true}) {
        Case c = planted("rounding_visible", 2, 0.f, 0.f, {});
        c.keys = keys;
        c.lambda = kPlantedLambda;
        c.rel = {1.f, kPlantedR};
        c.sim = {0.f, kPlantedPen, 0.f, 0.f};
        c.topk = 2;
        const Picks p = run(c);
        if (p.pos[1] != 1 || p.pen[1] != kPlantedPen || !same_bits(&p.value[1], &kPlantedValue, 8) || same_bits(&p.value[1], &kPlantedOnce, 8))
            fail("rounding_visible");
        ++g_t.rounding;
    }
    // nobody, nothing asked
    {
        Case c = random_case("empty_pool", 5, 1);
        c.m = 0;
        c.topk = 3;
        run(c);
        Case z = random_case("topk_0", 5, 1);
        z.topk = 0;
        run(z);
    }
    printf("S cases %lld keys %lld plain %lld multi_wave %lld ties %lld cross_wave_ties %lld all_equal %lld last_pos %lld lane_ends %lld "
           "asym %lld pen_kept %lld rounding %lld past_m %lld\n",
           (long long)g_t.cases, (long long)g_t.keys, (long long)g_t.plain, (long long)g_t.multi_wave, (long long)g_t.ties,
           (long long)g_t.cross_wave_ties, (long long)g_t.all_equal, (long long)g_t.last_pos, (long long)g_t.lane_ends, (long long)g_t.asym,
           (long long)g_t.pen_kept, (long long)g_t.rounding, (long long)g_t.past_m);
}

// wall time of the stage (launch, copy of the picks, synchronisation): the median of 15 after 3 warm-ups
void sweep() {
    for (int m : {64, 100, 200, 512, 1024}) {
        Case c = random_case("sweep", m, 9);
        c.stride = m;
        c.sim.resize((size_t)m * (size_t)m);
        float* d = up(c.sim);
        int32_t* d_uid = up(c.uid);
        float* d_rel = up(c.rel);
        std::vector<int> topks{10, 20, 64};
        if (m != 64) topks.push_back(m);
        for (int topk : topks) {
            if (topk > m) continue;
            pf::DiverseIn in{nullptr, d_uid, d_rel, m, d, m, 0.7f, topk};
            std::vector<int32_t> ou((size_t)topk);
            std::vector<float> orr((size_t)topk);
            std::vector<double> ms;
            for (int it = 0; it < 18; ++it) {
                int32_t n = 0;
                hipError_t err;
                const auto t0 = std::chrono::steady_clock::now();
                if (pf::diverse_run(in, g_ws, nullptr, ou.data(), orr.data(), nullptr, nullptr, nullptr, &n, &err) != pf::kDiverseOk) {
                    printf("sweep: stage failed\n");
                    exit(1);
                }
                if (it >= 3) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            printf("sweep m %d topk %d median_ms %.4f min_ms %.4f max_ms %.4f us_per_pick %.3f\n", m, topk, ms[ms.size() / 2], ms.front(),
                   ms.back(), 1000.0 * ms[ms.size() / 2] / topk);
        }
        (void)hipFree(d); (void)hipFree(d_uid); (void)hipFree(d_rel);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "sweep") == 0) {
        sweep();
    } else {
        cases();
    }
    printf("OK\n");
    return 0;
}
