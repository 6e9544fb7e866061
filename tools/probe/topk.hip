// Device check of the primitives every ranked list goes through, each against a plain host reference
// (std::multiset, std::sort, serial loops; nothing below shares code with the headers under test,
// except score_key / key_score / key_uid, which section (b) checks on their own):
//   (a) pf_device.h topk_push / topk_insert, one wave per case, the whole list after every round;
//   (b) pf_types.h score_key / key_score / key_uid, on the device and on the host;
//   (c) pf_device.h wave_incl_scan, wave_last, wave_max_u32, lane_rev64, rdlane64, two waves per block;
//   (d) pf_block.h block_rank, block_rank2, block_scan_incl at 4 and 16 waves, each called twice in a row.
// Prints one summary line per section and OK, or the first mismatches and FAIL n.
//   hipcc --offload-arch=gfx950 -O3 -I csrc tools/probe/topk.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>
#include "pf_block.h"
#include "pf_device.h"
#include "pf_types.h"
using namespace pf;

#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FAIL %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int g_bad = 0;
#define BAD(...) do { if (g_bad++ < 20) printf(__VA_ARGS__); } while (0)

static const uint64_t NONE = ~0ull;
static std::mt19937_64 rng(20260);
static uint64_t rnd(uint64_t n) { return rng() % n; }  // [0, n)

// ================================================================ (a) topk_push
struct Case { int round0, rounds; };

__global__ void push_probe(const uint64_t* in, uint64_t* out, const Case* cases, int k) {
    const Case c = cases[blockIdx.x];
    const int lane = threadIdx.x;
    uint64_t list = ~0ull;
    for (int r = 0; r < c.rounds; ++r) {
        topk_push(list, in[(size_t)(c.round0 + r) * 64 + lane], k, lane);
        out[(size_t)(c.round0 + r) * 64 + lane] = list;
    }
}

// The reference: every key pushed so far; the list is its k smallest, ~0 where there are fewer.
struct Ref {
    std::multiset<uint64_t> all;
    std::vector<uint64_t> list(int k) const {
        std::vector<uint64_t> v;
        for (auto it = all.begin(); it != all.end() && (int)v.size() < k; ++it) v.push_back(*it);  // ascending
        v.resize(k, NONE);
        return v;
    }
    uint64_t thr(int k) const { return list(k)[k - 1]; }
    int qualifying(const uint64_t* x, int k) const {
        const uint64_t t = thr(k);
        int q = 0;
        for (int l = 0; l < 64; ++l) q += x[l] < t;
        return q;
    }
    void push(const uint64_t* x) { all.insert(x, x + 64); }
};

static const int kKs[10] = {1, 2, 3, 4, 5, 31, 32, 33, 63, 64};
static const int kQs[8] = {0, 1, 2, 3, 4, 5, 63, 64};

// The cases of one k: keys[round][64] and the rounds of each case.  want_q[round] is the number of
// qualifying lanes the round was built for (-1: not built for a count).
struct Stream {
    int k;
    std::vector<uint64_t> keys;
    std::vector<int> want_q;
    std::vector<Case> cases;
    Ref cur;  // the reference over the case being built (the q-rounds are built from its threshold)
    void begin() { cases.push_back(Case{(int)want_q.size(), 0}); cur = Ref(); }
    void round(const uint64_t* x, int q = -1) {
        keys.insert(keys.end(), x, x + 64);
        want_q.push_back(q);
        ++cases.back().rounds;
        cur.push(x);
    }
};

static uint64_t real_key() { const uint64_t v = rng(); return v == NONE ? v - 1 : v; }

// exactly q lanes below the reference's current threshold, at lanes chosen by `place`
// (0 the low lanes, 1 the high lanes, 2 scattered); the others equal to it, above it or ~0
static bool q_round(Stream& s, int q, int place) {
    const uint64_t thr = s.cur.thr(s.k);
    if (thr < (1ull << 20)) return false;  // no room left below the threshold
    int lanes[64];
    for (int l = 0; l < 64; ++l) lanes[l] = place == 1 ? 63 - l : l;
    if (place == 2) std::shuffle(lanes, lanes + 64, rng);
    uint64_t x[64];
    for (int i = 0; i < 64; ++i) {
        uint64_t v;
        if (i < q) v = thr / 2 + rnd(thr - thr / 2);  // [thr / 2, thr)
        else {
            const int kind = (int)rnd(3);
            v = kind == 0 || thr == NONE ? thr : kind == 1 ? thr + 1 + rnd(NONE - thr) : NONE;
        }
        x[lanes[i]] = v;
    }
    s.round(x, q);
    return true;
}

static Stream build_stream(int k) {
    Stream s;
    s.k = k;
    uint64_t x[64];
    // seeded random 64-bit keys
    s.begin();
    for (int r = 0; r < 48; ++r) { for (auto& v : x) v = real_key(); s.round(x); }
    // strictly descending: every lane qualifies in every round
    s.begin();
    {
        uint64_t v = NONE - 1 - rnd(1000);
        for (int r = 0; r < 16; ++r) { for (auto& y : x) { y = v; v -= 1 + rnd(1ull << 50); } s.round(x, 64); }
    }
    // strictly ascending
    s.begin();
    {
        uint64_t v = rnd(1000);
        for (int r = 0; r < 8; ++r) { for (auto& y : x) { y = v; v += 1 + rnd(1ull << 50); } s.round(x); }
    }
    // a fill round, then eight rounds of exactly q qualifying lanes
    for (int q : kQs)
        for (int place = 0; place < 3; ++place) {
            s.begin();
            for (auto& v : x) v = (1ull << 62) + rnd(3ull << 62);
            s.round(x, 64);
            for (int r = 0; r < 8; ++r)
                if (!q_round(s, q, place)) BAD("k %d q %d: threshold ran out of room\n", k, q);
        }
    // all keys equal
    s.begin();
    { const uint64_t v = real_key(); for (auto& y : x) y = v; for (int r = 0; r < 8; ++r) s.round(x, r == 0 ? 64 : 0); }
    // the current threshold and keys already in the list, repeated; every third round the threshold
    // alone (nothing qualifies, the list stays as it is)
    s.begin();
    for (auto& v : x) v = real_key();
    s.round(x, 64);
    for (int r = 1; r < 12; ++r) {
        const std::vector<uint64_t> have = s.cur.list(k);
        for (auto& v : x) v = r % 3 == 0 || rnd(2) ? have[k - 1] : rnd(8) ? have[rnd(k)] : NONE;
        s.round(x, r % 3 == 0 ? 0 : -1);
    }
    // k - 1 real keys in all, ~0 elsewhere: the tail stays ~0
    s.begin();
    {
        std::vector<uint64_t> slots(8 * 64, NONE);
        for (int i = 0; i < k - 1; ++i) slots[i] = real_key();
        std::shuffle(slots.begin(), slots.end(), rng);
        for (int r = 0; r < 8; ++r) s.round(&slots[r * 64]);
    }
    // one high word, low words on both sides of 2^31; then one low word, high words on both sides
    for (int high : {0, 1}) {
        s.begin();
        for (int r = 0; r < 8; ++r) {
            for (auto& v : x) {
                const uint32_t w = rnd(2) ? 0x80000000u + (uint32_t)rnd(64) - 32u : (uint32_t)rng();
                v = high ? ((uint64_t)w << 32) | 0x9ABCDEF0u : (0x12345678ull << 32) | w;
            }
            s.round(x);
        }
    }
    // real keys: few scores (long ties), the edge uids and dense runs
    s.begin();
    {
        const uint32_t fbits[6] = {0x00000000u, 0x3E800000u, 0x3F000000u, 0x3F400000u, 0x3F7FFFFFu, 0x3F800000u};
        const int32_t edge[4] = {0, 1, (1 << 30) - 1, INT32_MAX};
        for (int r = 0; r < 8; ++r) {
            for (int l = 0; l < 64; ++l) {
                float f;
                memcpy(&f, &fbits[rnd(6)], 4);
                x[l] = score_key(f, rnd(4) == 0 ? edge[rnd(4)] : 5000 + r * 64 + l);
            }
            s.round(x);
        }
    }
    return s;
}

static int section_topk() {
    long cases = 0, rounds = 0, qn[6] = {0, 0, 0, 0, 0, 0};  // q0 q1 q2 q3 q4plus (4..64) q64
    bool seen[10][65] = {}, wanted[10][65] = {};
    for (int ki = 0; ki < 10; ++ki) {
        const int k = kKs[ki];
        const Stream s = build_stream(k);
        const int nr = (int)s.want_q.size(), nc = (int)s.cases.size();
        for (const Case& c : s.cases)
            if (c.rounds < 8 || c.rounds > 48 || c.round0 < 0 || c.round0 + c.rounds > nr) { BAD("k %d: bad case extents\n", k); return 1; }
        uint64_t *din, *dout; Case* dc;
        CK(hipMalloc(&din, (size_t)nr * 64 * 8));
        CK(hipMalloc(&dout, (size_t)nr * 64 * 8));
        CK(hipMalloc(&dc, nc * sizeof(Case)));
        CK(hipMemcpy(din, s.keys.data(), (size_t)nr * 64 * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(dc, s.cases.data(), nc * sizeof(Case), hipMemcpyHostToDevice));
        CK(hipMemset(dout, 0x5A, (size_t)nr * 64 * 8));
        push_probe<<<nc, 64>>>(din, dout, dc, k);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        std::vector<uint64_t> got((size_t)nr * 64);
        CK(hipMemcpy(got.data(), dout, got.size() * 8, hipMemcpyDeviceToHost));
        CK(hipFree(din)); CK(hipFree(dout)); CK(hipFree(dc));
        for (int ci = 0; ci < nc; ++ci) {
            Ref ref;
            for (int r = s.cases[ci].round0; r < s.cases[ci].round0 + s.cases[ci].rounds; ++r) {
                const uint64_t* x = &s.keys[(size_t)r * 64];
                const int q = ref.qualifying(x, k);
                if (s.want_q[r] >= 0) {
                    wanted[ki][s.want_q[r]] = true;
                    if (q != s.want_q[r]) BAD("k %d case %d round %d: built for %d qualifying lanes, the reference counts %d\n", k, ci, r - s.cases[ci].round0, s.want_q[r], q);
                }
                seen[ki][q] = true;
                ++qn[q < 4 ? q : 4];
                qn[5] += q == 64;
                const std::vector<uint64_t> before = ref.list(k);
                ref.push(x);
                const std::vector<uint64_t> want = ref.list(k);
                if (q == 0 && want != before) BAD("k %d case %d: the reference changed its list in a round without qualifying keys\n", k, ci);
                for (int l = 0; l < k; ++l)
                    if (got[(size_t)r * 64 + l] != want[l]) {
                        BAD("topk k %d case %d round %d (q %d) lane %d: %016llx want %016llx\n", k, ci, r - s.cases[ci].round0, q, l,
                            (unsigned long long)got[(size_t)r * 64 + l], (unsigned long long)want[l]);
                        break;
                    }
                ++rounds;
            }
        }
        cases += nc;
    }
    printf("topk cases %ld rounds %ld q0 %ld q1 %ld q2 %ld q3 %ld q4plus %ld q64 %ld\n", cases, rounds, qn[0], qn[1], qn[2], qn[3], qn[4], qn[5]);
    int missing = 0;
    for (int ki = 0; ki < 10; ++ki)
        for (int q : kQs) {
            if (!wanted[ki][q]) { BAD("k %d q %d: no round built\n", kKs[ki], q); }
            if (!seen[ki][q]) { ++missing; BAD("topk_kq_missing k %d q %d\n", kKs[ki], q); }
        }
    printf("topk_kq_missing %d\n", missing);
    return 0;
}

// ================================================================ (b) key encoding
__global__ void key_probe(const float* f, const int32_t* u, int n, uint64_t* key, uint32_t* score_bits, int32_t* uid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = score_key(f[i], u[i]);
    key[i] = k;
    const float s = key_score(k);
    score_bits[i] = __float_as_uint(s);
    uid[i] = key_uid(k);
}

static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float float_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

static int section_keys() {
    const uint32_t fb[] = {0x00000000u, 0x80000000u,                                       // +0, -0
                           0x00000001u, 0x3E000000u, 0x3F000000u, 0x3F7FFFFFu, 0x3F800000u, 0x3F800001u,  // denormal, 2^-3, .5, 1-ulp, 1, 1+ulp
                           0x80000001u, 0xBE000000u, 0xBF800000u, 0xC2F00000u, 0x7F800000u};  // -denormal, -2^-3, -1, -120, +inf
    std::vector<int32_t> uids = {0, 1, (1 << 30) - 1, INT32_MAX};
    for (int i = 0; i < 8; ++i) uids.push_back(5000 + i);
    std::vector<float> f;
    std::vector<int32_t> u;
    for (uint32_t b : fb)
        for (int32_t id : uids) { f.push_back(float_of(b)); u.push_back(id); }
    const int n = (int)f.size();
    float* df; int32_t *du, *duid; uint64_t* dk; uint32_t* ds;
    CK(hipMalloc(&df, n * 4)); CK(hipMalloc(&du, n * 4)); CK(hipMalloc(&duid, n * 4)); CK(hipMalloc(&dk, n * 8)); CK(hipMalloc(&ds, n * 4));
    CK(hipMemcpy(df, f.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(du, u.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dk, 0x5A, n * 8)); CK(hipMemset(ds, 0x5A, n * 4)); CK(hipMemset(duid, 0x5A, n * 4));
    key_probe<<<(n + 63) / 64, 64>>>(df, du, n, dk, ds, duid);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint64_t> key(n); std::vector<uint32_t> sb(n); std::vector<int32_t> uid(n);
    CK(hipMemcpy(key.data(), dk, n * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(sb.data(), ds, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(uid.data(), duid, n * 4, hipMemcpyDeviceToHost));
    CK(hipFree(df)); CK(hipFree(du)); CK(hipFree(duid)); CK(hipFree(dk)); CK(hipFree(ds));
    for (int i = 0; i < n; ++i) {
        const uint64_t h = score_key(f[i], u[i]);
        if (key[i] != h) BAD("key %d: device %016llx host %016llx\n", i, (unsigned long long)key[i], (unsigned long long)h);
        const uint32_t want = bits_of(f[i]) == 0x80000000u ? 0u : bits_of(f[i]);  // -0 comes back as +0
        if (sb[i] != want || bits_of(key_score(h)) != want) BAD("key_score %d: device %08x host %08x want %08x\n", i, sb[i], bits_of(key_score(h)), want);
        if (uid[i] != u[i] || key_uid(h) != u[i]) BAD("key_uid %d: device %d host %d want %d\n", i, uid[i], key_uid(h), u[i]);
        if (h == NONE) BAD("key %d is the empty key\n", i);
    }
    // ascending keys == (score descending, uid ascending), -0 == +0 (float compare)
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    auto before = [&](int a, int b) { return f[a] != f[b] ? f[a] > f[b] : u[a] < u[b]; };
    std::stable_sort(order.begin(), order.end(), before);
    std::vector<uint64_t> sorted(key);
    std::sort(sorted.begin(), sorted.end());
    int ties = 0;
    for (int i = 0; i < n; ++i) {
        if (key[order[i]] != sorted[i]) BAD("key order: position %d holds %016llx, the comparator puts %016llx there\n", i, (unsigned long long)sorted[i], (unsigned long long)key[order[i]]);
        if (i == 0) continue;
        const bool lt = before(order[i - 1], order[i]);
        ties += !lt;
        if (lt ? !(sorted[i - 1] < sorted[i]) : sorted[i - 1] != sorted[i]) BAD("key order: positions %d and %d compare differently\n", i - 1, i);
    }
    printf("keys pairs %d equal_pairs %d\n", n, ties);
    return 0;
}

// ================================================================ (c) wave helpers
constexpr int kWaveProbeThreads = 128;  // two waves per block
__global__ void wave_probe(const uint32_t* in, uint32_t* scan, uint32_t* last, uint32_t* mx) {
    const size_t i = (size_t)blockIdx.x * kWaveProbeThreads + threadIdx.x;
    const uint32_t x = in[i];
    scan[i] = wave_incl_scan(x);
    last[i] = wave_last(x);
    mx[i] = wave_max_u32(x);
}
// rev[t] = lane_rev64; rd[l * 128 + t] = rdlane64(v, l)
__global__ void lane64_probe(const uint64_t* in, uint64_t* rev, uint64_t* rd) {
    const uint64_t v = in[threadIdx.x];
    rev[threadIdx.x] = lane_rev64(v);
    for (int l = 0; l < 64; ++l) rd[l * kWaveProbeThreads + threadIdx.x] = rdlane64(v, l);
}

static int section_wave() {
    const int T = kWaveProbeThreads;
    std::vector<uint32_t> in;
    auto add = [&](auto&& gen) { for (int t = 0; t < T; ++t) in.push_back(gen(t)); };
    add([](int) { return 1u; });                                                          // all ones
    for (int p = 0; p < 64; ++p) add([p](int t) { return (uint32_t)(t == p || t == 64 + (63 - p)); });  // a single 1
    for (int i = 0; i < 8; ++i) add([](int) { return (uint32_t)rnd(1u << 20); });
    add([](int) { return 0x0C000000u + (uint32_t)rnd(1u << 26); });                       // the sum wraps 2^32
    for (int p = 0; p < 64; ++p)                                                          // the maximum at each lane
        add([p](int t) { return (t & 63) == (t < 64 ? p : 63 - p) ? 0xF0000000u + (uint32_t)t : (uint32_t)rnd(0xF0000000u); });
    const int nc = (int)in.size() / T;
    const size_t n = in.size();
    uint32_t *di, *dsc, *dl, *dm;
    CK(hipMalloc(&di, n * 4)); CK(hipMalloc(&dsc, n * 4)); CK(hipMalloc(&dl, n * 4)); CK(hipMalloc(&dm, n * 4));
    CK(hipMemcpy(di, in.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dsc, 0x5A, n * 4)); CK(hipMemset(dl, 0x5A, n * 4)); CK(hipMemset(dm, 0x5A, n * 4));
    wave_probe<<<nc, T>>>(di, dsc, dl, dm);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> sc(n), la(n), mx(n);
    CK(hipMemcpy(sc.data(), dsc, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(la.data(), dl, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(mx.data(), dm, n * 4, hipMemcpyDeviceToHost));
    CK(hipFree(di)); CK(hipFree(dsc)); CK(hipFree(dl)); CK(hipFree(dm));
    int wraps = 0;
    for (size_t w0 = 0; w0 < n; w0 += 64) {  // wave by wave
        uint32_t sum = 0, top = 0;
        uint64_t wide = 0;
        for (int l = 0; l < 64; ++l) { top = std::max(top, in[w0 + l]); wide += in[w0 + l]; }
        wraps += wide > 0xFFFFFFFFull;
        for (int l = 0; l < 64; ++l) {
            sum += in[w0 + l];
            if (sc[w0 + l] != sum) BAD("wave_incl_scan case %zu thread %zu: %u want %u\n", w0 / T, w0 % T + l, sc[w0 + l], sum);
            if (la[w0 + l] != in[w0 + 63]) BAD("wave_last case %zu thread %zu: %u want %u\n", w0 / T, w0 % T + l, la[w0 + l], in[w0 + 63]);
            if (mx[w0 + l] != top) BAD("wave_max_u32 case %zu thread %zu: %u want %u\n", w0 / T, w0 % T + l, mx[w0 + l], top);
        }
    }
    if (wraps == 0) BAD("no wave sum wrapped 2^32\n");
    // 64-bit lane moves on distinct values whose halves both differ from lane to lane
    std::vector<uint64_t> v(T);
    for (int t = 0; t < T; ++t) v[t] = ((uint64_t)(0xA0000000u + 977u * t) << 32) | (0x00C0FFEEu + 131071u * t);
    uint64_t *dv, *drev, *drd;
    CK(hipMalloc(&dv, T * 8)); CK(hipMalloc(&drev, T * 8)); CK(hipMalloc(&drd, 64 * T * 8));
    CK(hipMemcpy(dv, v.data(), T * 8, hipMemcpyHostToDevice));
    CK(hipMemset(drev, 0x5A, T * 8)); CK(hipMemset(drd, 0x5A, 64 * T * 8));
    lane64_probe<<<1, T>>>(dv, drev, drd);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint64_t> rev(T), rd(64 * T);
    CK(hipMemcpy(rev.data(), drev, T * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(rd.data(), drd, 64 * T * 8, hipMemcpyDeviceToHost));
    CK(hipFree(dv)); CK(hipFree(drev)); CK(hipFree(drd));
    for (int t = 0; t < T; ++t) {
        const int w0 = t & ~63, lane = t & 63;
        if (rev[t] != v[w0 + 63 - lane]) BAD("lane_rev64 thread %d\n", t);
        for (int l = 0; l < 64; ++l)
            if (rd[l * T + t] != v[w0 + l]) BAD("rdlane64 thread %d lane %d\n", t, l);
    }
    printf("wave cases %d waves_per_block %d wrapped %d lane64 %d\n", nc, T / 64, wraps, T);
    return 0;
}

// ================================================================ (d) block helpers
// Per thread and input set s (0, 1): flags f0, f1 and a value.  Every helper runs on set 0 and at
// once again on set 1 over the same wsum.  Totals are the same in every thread of a block: the
// kernel keeps their minimum and maximum over the block, the host wants both equal to its sum.
struct BlockIn { uint16_t v[2]; uint8_t flags; };  // flags: bit 2 s + j = flag j of set s
struct BlockOut { uint16_t rank[2], r0[2], r1[2]; int32_t scan[2]; };
constexpr int kTotals = 8;  // rank s | rank2 t0 s, t1 s | scan s

template <int NW>
__global__ __launch_bounds__(NW * 64) void block_probe(const BlockIn* in, BlockOut* out, int* tmin, int* tmax) {
    __shared__ int wsum[2 * NW];
    const size_t i = (size_t)blockIdx.x * (NW * 64) + threadIdx.x;
    const BlockIn x = in[i];
    BlockOut o;
    int tot[kTotals];
    for (int s = 0; s < 2; ++s) o.rank[s] = (uint16_t)block_rank<NW>((x.flags >> (2 * s)) & 1, wsum, tot[s]);
    for (int s = 0; s < 2; ++s) {
        int r0, r1;
        block_rank2<NW>((x.flags >> (2 * s)) & 1, (x.flags >> (2 * s + 1)) & 1, wsum, r0, r1, tot[2 + 2 * s], tot[3 + 2 * s]);
        o.r0[s] = (uint16_t)r0;
        o.r1[s] = (uint16_t)r1;
    }
    for (int s = 0; s < 2; ++s) o.scan[s] = block_scan_incl<NW>(x.v[s], wsum, tot[6 + s]);
    out[i] = o;
    for (int j = 0; j < kTotals; ++j) {
        atomicMin(&tmin[blockIdx.x * kTotals + j], tot[j]);
        atomicMax(&tmax[blockIdx.x * kTotals + j], tot[j]);
    }
}

template <int NW>
static int block_cases(int& ncases) {
    const int T = NW * 64;
    std::vector<BlockIn> in;
    // f(set, flag index, thread) and v(set, thread)
    auto add = [&](auto&& f, auto&& v) {
        for (int t = 0; t < T; ++t) {
            BlockIn b;
            b.flags = 0;
            for (int s = 0; s < 2; ++s) {
                for (int j = 0; j < 2; ++j) b.flags |= (uint8_t)((f(s, j, t) ? 1 : 0) << (2 * s + j));
                b.v[s] = v(s, t);
            }
            in.push_back(b);
        }
    };
    auto rv = [](int, int) { return (int)rnd(1001); };
    add([](int s, int j, int) { return s != j; }, [](int s, int) { return s; });           // all false | all true; values 0, then 1
    add([](int s, int j, int t) { return ((t + s + j) & 1) != 0; }, rv);                   // alternating
    for (int w = 0; w < NW; ++w)  // a single thread set: the first and the last thread of every wave
        add([w](int s, int j, int t) {  // set 0: first | last of wave w; set 1: last of wave w | first of wave NW - 1 - w
            const int first = 64 * w, last = 64 * w + 63, other = 64 * (NW - 1 - w);
            return t == (s == 0 ? (j == 0 ? first : last) : (j == 0 ? last : other));
        }, rv);
    for (int d : {2, 2, 32, 5}) add([d](int, int, int) { return rnd(d) == 0; }, rv);        // seeded random
    const int nc = (int)in.size() / T;
    const size_t n = in.size();
    BlockIn* di; BlockOut* dout; int *dmin, *dmax;
    std::vector<int> tmin(nc * kTotals, INT_MAX), tmax(nc * kTotals, INT_MIN);
    CK(hipMalloc(&di, n * sizeof(BlockIn))); CK(hipMalloc(&dout, n * sizeof(BlockOut)));
    CK(hipMalloc(&dmin, tmin.size() * 4)); CK(hipMalloc(&dmax, tmax.size() * 4));
    CK(hipMemcpy(di, in.data(), n * sizeof(BlockIn), hipMemcpyHostToDevice));
    CK(hipMemcpy(dmin, tmin.data(), tmin.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dmax, tmax.data(), tmax.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dout, 0x5A, n * sizeof(BlockOut)));
    block_probe<NW><<<nc, T>>>(di, dout, dmin, dmax);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<BlockOut> out(n);
    CK(hipMemcpy(out.data(), dout, n * sizeof(BlockOut), hipMemcpyDeviceToHost));
    CK(hipMemcpy(tmin.data(), dmin, tmin.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(tmax.data(), dmax, tmax.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(di)); CK(hipFree(dout)); CK(hipFree(dmin)); CK(hipFree(dmax));
    for (int c = 0; c < nc; ++c) {
        const BlockIn* x = &in[(size_t)c * T];
        const BlockOut* o = &out[(size_t)c * T];
        int want_tot[kTotals];
        for (int s = 0; s < 2; ++s) {
            int n0 = 0, n1 = 0;
            for (int t = 0; t < T; ++t) { n0 += (x[t].flags >> (2 * s)) & 1; n1 += (x[t].flags >> (2 * s + 1)) & 1; }
            // exclusive ranks in thread order; block_rank2: every f0 item, then every f1 item
            int a = 0, b = n0, sum = 0;
            for (int t = 0; t < T; ++t) {
                if (o[t].rank[s] != a) BAD("block_rank<%d> case %d set %d thread %d: %d want %d\n", NW, c, s, t, o[t].rank[s], a);
                if (o[t].r0[s] != a || o[t].r1[s] != b) BAD("block_rank2<%d> case %d set %d thread %d: %d %d want %d %d\n", NW, c, s, t, o[t].r0[s], o[t].r1[s], a, b);
                a += (x[t].flags >> (2 * s)) & 1;
                b += (x[t].flags >> (2 * s + 1)) & 1;
                sum += x[t].v[s];
                if (o[t].scan[s] != sum) BAD("block_scan_incl<%d> case %d set %d thread %d: %d want %d\n", NW, c, s, t, o[t].scan[s], sum);
            }
            want_tot[s] = n0;
            want_tot[2 + 2 * s] = n0;
            want_tot[3 + 2 * s] = n1;
            want_tot[6 + s] = sum;
        }
        for (int j = 0; j < kTotals; ++j)
            if (tmin[c * kTotals + j] != want_tot[j] || tmax[c * kTotals + j] != want_tot[j])
                BAD("block total<%d> case %d #%d: min %d max %d want %d\n", NW, c, j, tmin[c * kTotals + j], tmax[c * kTotals + j], want_tot[j]);
    }
    ncases = nc;
    return 0;
}

static int section_block() {
    int n4 = 0, n16 = 0;
    if (block_cases<4>(n4)) return 1;
    if (block_cases<16>(n16)) return 1;
    printf("block nw4 cases %d nw16 cases %d\n", n4, n16);
    return 0;
}

int main() {
    if (section_topk() || section_keys() || section_wave() || section_block()) return 1;
    if (g_bad) printf("FAIL %d\n", g_bad); else printf("OK\n");
    return g_bad ? 1 : 0;
}
