// pf_clubsum.hip — clubs by interest, the device stage (pf_clubsum.h): own bitmap, count, place, emit,
// sort, sum, rank.  Every contribution of a club is added by one thread in ascending rank, so a club's
// double accumulator sees the adds in the order of the definition; nothing else here touches a sum.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <vector>

#include "pf_block.h"
#include "pf_clubsum.h"
#include "pf_types.h"

namespace pf {
namespace {

constexpr int kNW = kClubSumThreads / 64;

struct LongRun {
    uint32_t start, len, slot, dense;
};

// device view of one call
struct Stage {
    const uint64_t* keys;
    const int32_t* uid;
    const int64_t* club_off;
    const int32_t* club_dense;
    const int32_t* club_id;
    const uint32_t* bitmap;  // nullptr: no own list
    uint32_t used, n_users, n_club_ids, rank_bits;
    uint32_t C;              // contributions (emit and later)
    uint32_t cutover;
    uint32_t run_cap, long_cap;
};

__device__ __forceinline__ bool is_own(const Stage& st, int32_t d) {
    return st.bitmap != nullptr && ((st.bitmap[(uint32_t)d >> 5] >> ((uint32_t)d & 31u)) & 1u) != 0u;
}

// the club range of ranked neighbour r; empty when its weight is <= 0 (the reference's serial test)
// or its uid has no profile
__device__ __forceinline__ void club_range(const Stage& st, uint32_t r, int64_t& cb, int64_t& ce) {
    cb = ce = 0;
    const uint64_t key = st.keys[r];
    const double w = (double)key_score(key);
    if (w <= 0.0) return;
    const int32_t u = key_uid(key);
    uint32_t lo = 0, hi = st.n_users;
    while (lo < hi) {  // first index whose uid is >= u
        const uint32_t mid = (lo + hi) >> 1;
        if (st.uid[mid] < u) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= st.n_users || st.uid[lo] != u) return;
    cb = st.club_off[lo];
    ce = st.club_off[lo + 1];
}

__global__ __launch_bounds__(256) void own_kernel(const int32_t* __restrict__ own, uint32_t n_own, uint32_t n_club_ids,
                                                  uint32_t* __restrict__ bitmap) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_own) return;
    const uint32_t d = (uint32_t)own[i];
    if (d < n_club_ids) atomicOr(&bitmap[d >> 5], 1u << (d & 31u));
}

// cnt[r] = contributions of ranked neighbour r; btot[block] = their sum over the workgroup
__global__ __launch_bounds__(kClubSumThreads) void count_kernel(Stage st, uint32_t* __restrict__ cnt,
                                                                unsigned long long* __restrict__ btot) {
    __shared__ int wsum[kNW];
    const uint32_t r = blockIdx.x * (uint32_t)kClubSumThreads + threadIdx.x;
    int n = 0;
    if (r < st.used) {
        int64_t cb, ce;
        club_range(st, r, cb, ce);
        if (st.bitmap == nullptr) {
            n = (int)(ce - cb);
        } else {
            for (int64_t k = cb; k < ce; ++k) n += is_own(st, st.club_dense[k]) ? 0 : 1;
        }
        cnt[r] = (uint32_t)n;
    }
    int total;  // at most 256 x 65,535: an int holds it
    (void)block_scan_incl<kNW>(n, wsum, total);
    if (threadIdx.x == 0) btot[blockIdx.x] = (unsigned long long)total;
}

// one key per contribution at its place: (dense << rank_bits) | rank
__global__ __launch_bounds__(kClubSumThreads) void emit_kernel(Stage st, const uint32_t* __restrict__ cnt,
                                                               const unsigned long long* __restrict__ bbase,
                                                               uint64_t* __restrict__ ckeys) {
    __shared__ int wsum[kNW];
    const uint32_t r = blockIdx.x * (uint32_t)kClubSumThreads + threadIdx.x;
    const int n = r < st.used ? (int)cnt[r] : 0;
    int total;
    const int incl = block_scan_incl<kNW>(n, wsum, total);
    if (n == 0) return;
    uint64_t pos = (uint64_t)bbase[blockIdx.x] + (uint64_t)(incl - n);
    uint64_t end = pos + (uint64_t)n;
    if (end > (uint64_t)st.C) end = (uint64_t)st.C;  // never past the buffer
    int64_t cb, ce;
    club_range(st, r, cb, ce);
    for (int64_t k = cb; k < ce && pos < end; ++k) {
        const int32_t d = st.club_dense[k];
        if (is_own(st, d)) continue;
        ckeys[pos++] = ((uint64_t)(uint32_t)d << st.rank_bits) | (uint64_t)r;
    }
}

__device__ __forceinline__ double weight_at(const Stage& st, uint64_t ckey) {
    const uint32_t r = (uint32_t)(ckey & ((1ull << st.rank_bits) - 1ull));
    return (double)key_score(st.keys[r]);
}

// counters[0] = runs, counters[1] = long runs.  A thread on a run's first key adds the run in order
// while it is shorter than the cut-over; a run that reaches it is listed for long_kernel.
__global__ __launch_bounds__(256) void heads_kernel(Stage st, const uint64_t* __restrict__ skeys,
                                                    unsigned long long* __restrict__ counters,
                                                    uint64_t* __restrict__ rkeys, LongRun* __restrict__ longs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= st.C) return;
    const uint32_t d = (uint32_t)(skeys[i] >> st.rank_bits);
    if (i > 0 && (uint32_t)(skeys[i - 1] >> st.rank_bits) == d) return;
    const uint32_t slot = (uint32_t)atomicAdd(&counters[0], 1ull);
    if (slot >= st.run_cap) return;  // cannot happen: at most one run per club and per contribution
    double acc = 0.0;
    uint32_t j = i;
    while (j < st.C && j - i < st.cutover - 1u && (uint32_t)(skeys[j] >> st.rank_bits) == d) {
        acc += weight_at(st, skeys[j]);
        ++j;
    }
    if (j >= st.C || (uint32_t)(skeys[j] >> st.rank_bits) != d) {
        rkeys[slot] = score_key((float)acc, st.club_id[d]);
        return;
    }
    // cutover - 1 keys seen and the run goes on: its end is the first key of a later club
    uint32_t lo = j, hi = st.C;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)(skeys[mid] >> st.rank_bits) <= d) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t l = (uint32_t)atomicAdd(&counters[1], 1ull);
    if (l < st.long_cap) longs[l] = LongRun{i, lo - i, slot, d};
}

// one wave per listed run: 64 weights per step are loaded by the wave's lanes, then every lane adds the
// same 64 values in lane order (readlane with a wave-uniform index): the loads are parallel, the FP64
// add chain is serial and in rank order
__global__ __launch_bounds__(256) void long_kernel(Stage st, const uint64_t* __restrict__ skeys,
                                                   const unsigned long long* __restrict__ counters,
                                                   const LongRun* __restrict__ longs, uint64_t* __restrict__ rkeys) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long listed = counters[1];
    const uint32_t n_long = listed < (unsigned long long)st.long_cap ? (uint32_t)listed : st.long_cap;
    for (uint32_t x = blockIdx.x * 4u + wave; x < n_long; x += gridDim.x * 4u) {
        const LongRun R = longs[x];
        double acc = 0.0;
        for (uint32_t b = 0; b < R.len; b += 64u) {
            const uint32_t m = R.len - b < 64u ? R.len - b : 64u;
            const double w = lane < m ? weight_at(st, skeys[R.start + b + lane]) : 0.0;
            const int lo = __double2loint(w), hi = __double2hiint(w);
            for (uint32_t k = 0; k < m; ++k)
                acc += __hiloint2double(__builtin_amdgcn_readlane(hi, (int)k), __builtin_amdgcn_readlane(lo, (int)k));
        }
        if (lane == 0) rkeys[R.slot] = score_key((float)acc, st.club_id[R.dense]);
    }
}

int bit_width_u32(uint32_t v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// a workspace that cannot be had is reported, not fatal: the sticky error is cleared
bool grow(DBuf& b, size_t bytes) {
    if (b.ensure(std::max<size_t>(bytes, 16)) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

}  // namespace

#define CS_HIP(expr)                     \
    do {                                 \
        const hipError_t _e = (expr);    \
        if (_e != hipSuccess) {          \
            if (err) *err = _e;          \
            return kClubSumHip;          \
        }                                \
    } while (0)
#define CS_MEM(buf, bytes) \
    do {                   \
        if (!grow(buf, bytes)) return kClubSumNoMem; \
    } while (0)

ClubSumStatus clubsum_run(const ClubSumIn& in, ClubSumWs& ws, hipStream_t s, int32_t* out_club, float* out_score,
                          ClubSumOut* out, hipError_t* err) {
    *out = ClubSumOut{};
    if (err) *err = hipSuccess;
    if (in.used < 0 || in.used > (int64_t)INT32_MAX || in.n_users < 0 || in.n_club_ids < 0 || in.n_own < 0 || in.topk < 0) {
        if (err) *err = hipErrorInvalidValue;
        return kClubSumHip;
    }
    if (in.used == 0 || in.n_club_ids == 0 || in.n_users == 0) return kClubSumOk;

    Stage st{};
    st.keys = in.keys;
    st.uid = in.uid;
    st.club_off = in.club_off;
    st.club_dense = in.club_dense;
    st.club_id = in.club_id;
    st.used = (uint32_t)in.used;
    st.n_users = (uint32_t)in.n_users;
    st.n_club_ids = (uint32_t)in.n_club_ids;
    st.rank_bits = (uint32_t)std::max(1, bit_width_u32(st.used - 1u));
    st.cutover = (uint32_t)std::max(2, in.cutover > 0 ? in.cutover : kClubSumCutoverDefault);
    const int club_bits = std::max(1, bit_width_u32(st.n_club_ids - 1u));
    const uint32_t nb = (st.used + kClubSumThreads - 1u) / kClubSumThreads;

    // own bitmap
    if (in.n_own > 0) {
        const size_t words = ((size_t)st.n_club_ids + 31u) / 32u;
        CS_MEM(ws.own, (size_t)in.n_own * sizeof(int32_t));
        CS_MEM(ws.bitmap, words * sizeof(uint32_t));
        CS_HIP(hipMemcpyAsync(ws.own.p, in.own, (size_t)in.n_own * sizeof(int32_t), hipMemcpyHostToDevice, s));
        CS_HIP(hipMemsetAsync(ws.bitmap.p, 0, words * sizeof(uint32_t), s));
        hipLaunchKernelGGL(own_kernel, dim3(((uint32_t)in.n_own + 255u) / 256u), dim3(256), 0, s, ws.own.as<int32_t>(),
                           (uint32_t)in.n_own, st.n_club_ids, ws.bitmap.as<uint32_t>());
        CS_HIP(hipGetLastError());
        st.bitmap = ws.bitmap.as<uint32_t>();
    }

    // count, place
    using u64 = unsigned long long;
    CS_MEM(ws.cnt, (size_t)st.used * sizeof(uint32_t));
    CS_MEM(ws.btot, ((size_t)nb + 1) * sizeof(u64));
    CS_MEM(ws.bbase, ((size_t)nb + 1) * sizeof(u64));
    CS_MEM(ws.counters, 2 * sizeof(u64));
    CS_HIP(hipMemsetAsync(ws.btot.as<u64>() + nb, 0, sizeof(u64), s));  // the sum's last word: the total
    CS_HIP(hipMemsetAsync(ws.counters.p, 0, 2 * sizeof(u64), s));
    hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(kClubSumThreads), 0, s, st, ws.cnt.as<uint32_t>(), ws.btot.as<u64>());
    CS_HIP(hipGetLastError());
    size_t scan_b = 0;
    CS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, ws.btot.as<u64>(), ws.bbase.as<u64>(), (int)(nb + 1), s));
    CS_MEM(ws.scan_tmp, scan_b);
    CS_HIP(hipcub::DeviceScan::ExclusiveSum(ws.scan_tmp.p, scan_b, ws.btot.as<u64>(), ws.bbase.as<u64>(), (int)(nb + 1), s));
    u64 C = 0;
    CS_HIP(hipMemcpyAsync(&C, ws.bbase.as<u64>() + nb, sizeof(u64), hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    out->contributions = (int64_t)C;
    if (C > (u64)INT32_MAX) return kClubSumTooMany;
    if (C == 0) return kClubSumOk;

    // buffers of C entries, only now
    st.C = (uint32_t)C;
    st.run_cap = (uint32_t)std::min<u64>(C, st.n_club_ids);
    st.long_cap = st.C / st.cutover + 1u;
    size_t sort_b = 0, rsort_b = 0;
    {
        const uint64_t* a = nullptr;
        uint64_t* b = nullptr;
        CS_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_b, a, b, (int)st.C, 0, (int)st.rank_bits + club_bits, s));
    }
    CS_MEM(ws.ckeys, (size_t)st.C * sizeof(uint64_t));
    CS_MEM(ws.skeys, (size_t)st.C * sizeof(uint64_t));
    CS_MEM(ws.sort_tmp, sort_b);
    CS_MEM(ws.rkeys, (size_t)st.run_cap * sizeof(uint64_t));
    CS_MEM(ws.rsorted, (size_t)st.run_cap * sizeof(uint64_t));
    CS_MEM(ws.longs, (size_t)st.long_cap * sizeof(LongRun));

    hipLaunchKernelGGL(emit_kernel, dim3(nb), dim3(kClubSumThreads), 0, s, st, ws.cnt.as<uint32_t>(), ws.bbase.as<u64>(),
                       ws.ckeys.as<uint64_t>());
    CS_HIP(hipGetLastError());
    CS_HIP(hipcub::DeviceRadixSort::SortKeys(ws.sort_tmp.p, sort_b, ws.ckeys.as<uint64_t>(), ws.skeys.as<uint64_t>(), (int)st.C, 0,
                                             (int)st.rank_bits + club_bits, s));
    hipLaunchKernelGGL(heads_kernel, dim3((st.C + 255u) / 256u), dim3(256), 0, s, st, ws.skeys.as<uint64_t>(),
                       ws.counters.as<u64>(), ws.rkeys.as<uint64_t>(), ws.longs.as<LongRun>());
    CS_HIP(hipGetLastError());
    hipLaunchKernelGGL(long_kernel, dim3(std::min((st.long_cap + 3u) / 4u, 2048u)), dim3(256), 0, s, st, ws.skeys.as<uint64_t>(),
                       ws.counters.as<u64>(), ws.longs.as<LongRun>(), ws.rkeys.as<uint64_t>());
    CS_HIP(hipGetLastError());
    u64 cnts[2] = {0, 0};
    CS_HIP(hipMemcpyAsync(cnts, ws.counters.p, sizeof cnts, hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    const uint32_t R = (uint32_t)std::min<u64>(cnts[0], st.run_cap);
    out->clubs = (int64_t)R;
    out->long_runs = (int64_t)cnts[1];

    // rank
    const int32_t k = (int32_t)std::min<int64_t>(in.topk, R);
    out->count = k;
    if (k == 0) return kClubSumOk;
    {
        const uint64_t* a = nullptr;
        uint64_t* b = nullptr;
        CS_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, rsort_b, a, b, (int)R, 0, 64, s));
        CS_MEM(ws.sort_tmp, rsort_b);
    }
    CS_HIP(hipcub::DeviceRadixSort::SortKeys(ws.sort_tmp.p, rsort_b, ws.rkeys.as<uint64_t>(), ws.rsorted.as<uint64_t>(), (int)R, 0, 64, s));
    std::vector<uint64_t> top((size_t)k);
    CS_HIP(hipMemcpyAsync(top.data(), ws.rsorted.p, (size_t)k * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    for (int32_t i = 0; i < k; ++i) {
        out_club[i] = key_uid(top[(size_t)i]);
        out_score[i] = key_score(top[(size_t)i]);
    }
    return kClubSumOk;
}

}  // namespace pf
