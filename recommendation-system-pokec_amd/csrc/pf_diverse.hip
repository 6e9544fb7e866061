// pf_diverse.hip — diverse top-k, the device stage (pf_diverse.h): one workgroup picks min(topk, M)
// pool positions one after the other; each pick is a two-level argmax on (value desc, position asc)
// and one row load of the pair-score matrix.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "pf_device.h"
#include "pf_diverse.h"
#include "pf_types.h"

namespace pf {
namespace {

constexpr int kMaxWaves = kDiverseMaxPool / 64;

struct Pick {
    double value;
    int32_t uid;
    float r, pen;
    int32_t pos;
};
static_assert(sizeof(Pick) == 24, "a pick is 24 B");

// ascending key == descending double (-0 == +0, as the comparison of the definition has it)
__device__ __forceinline__ uint64_t value_key(double v) {
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if ((b << 1) == 0) b = 0;
    const uint64_t ord = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return ~ord;
}

// the smallest key among the lanes that are `in`, and the lowest lane that holds it (64: no lane is in)
__device__ __forceinline__ void wave_argmin(uint64_t key, bool in, uint64_t& best, uint32_t& at) {
    best = wave_min64(in ? key : ~0ull);
    const unsigned long long eq = __ballot(in && key == best);
    at = eq ? (uint32_t)__ffsll(eq) - 1u : 64u;
}

__global__ __launch_bounds__(kDiverseMaxPool) void diverse_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ uid,
                                                                  const float* __restrict__ rel, uint32_t m,
                                                                  const float* __restrict__ sim, uint64_t stride, float lambda,
                                                                  uint32_t picks, Pick* __restrict__ out,
                                                                  uint32_t* __restrict__ made) {
    __shared__ uint64_t wkey[2][kMaxWaves];
    __shared__ uint32_t wpos[2][kMaxWaves];
    const uint32_t i = threadIdx.x, lane = i & 63u, wave = i >> 6, nw = blockDim.x >> 6;
    const bool live = i < m;
    float r = 0.f, pen = 0.f;
    int32_t u = 0;
    if (live) {
        if (keys) {
            const uint64_t k = keys[i];
            r = key_score(k);
            u = key_uid(k);
        } else {
            r = rel[i];
            u = uid[i];
        }
    }
    bool open = live;  // in the pool and not picked yet
    const double dl = (double)lambda, om = 1.0 - dl;
    const double a = dl * (double)r;
    uint32_t t = 0;
    for (; t < picks; ++t) {
        const double p = om * (double)pen;
        const double v = a - p;
        uint64_t best;
        uint32_t at;
        wave_argmin(value_key(v), open, best, at);
        const uint32_t b = t & 1u;
        if (lane == 0) {
            wkey[b][wave] = best;
            wpos[b][wave] = wave * 64u + at;
        }
        __syncthreads();
        // every wave reduces the waves' winners for itself; slot b is written again two picks on,
        // behind the next pick's barrier
        uint64_t top;
        uint32_t w;
        wave_argmin(lane < nw ? wkey[b][lane] : ~0ull, lane < nw && wkey[b][lane] != ~0ull, top, w);
        if (w >= nw) break;  // nobody left (cannot happen while picks <= m); uniform over the workgroup
        const uint32_t s = wpos[b][w];
        if (s >= m) break;
        if (i == s) {
            out[t] = Pick{v, u, r, pen, (int32_t)s};
            open = false;
        }
        if (live) {
            const float x = sim[(uint64_t)s * stride + i];
            pen = x > pen ? x : pen;
        }
    }
    if (i == 0) *made = t;  // the records written: the host reads no more than these
}

}  // namespace

DiverseStatus diverse_run(const DiverseIn& in, DiverseWs& ws, hipStream_t s, int32_t* out_uid, float* out_r, float* out_pen,
                          double* out_value, int32_t* out_pos, int32_t* count, hipError_t* err) {
    *count = 0;
    if (err) *err = hipSuccess;
    const bool lam_ok = in.lambda >= 0.f && in.lambda <= 1.f;
    if (in.m < 0 || in.m > kDiverseMaxPool || in.topk < 0 || !lam_ok || in.stride < (int64_t)in.m ||
        (in.m > 0 && in.topk > 0 && (!in.sim || (!in.keys && (!in.uid || !in.rel))))) {
        if (err) *err = hipErrorInvalidValue;
        return kDiverseHip;
    }
    const int32_t k = std::min(in.topk, in.m);
    if (k == 0) return kDiverseOk;
    // k records, then the count of those the kernel wrote
    if (ws.picks.ensure((size_t)k * sizeof(Pick) + sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();  // reported, not fatal: the sticky error is cleared
        return kDiverseNoMem;
    }
    const uint32_t threads = ((uint32_t)in.m + 63u) / 64u * 64u;
    hipLaunchKernelGGL(diverse_kernel, dim3(1), dim3(threads), 0, s, in.keys, in.uid, in.rel, (uint32_t)in.m, in.sim,
                       (uint64_t)in.stride, in.lambda, (uint32_t)k, ws.picks.as<Pick>(),
                       reinterpret_cast<uint32_t*>(ws.picks.as<Pick>() + k));
    hipError_t e = hipGetLastError();
    std::vector<Pick> got((size_t)k + 1);  // the last entry's first word: the count
    if (e == hipSuccess)
        e = hipMemcpyAsync(got.data(), ws.picks.p, (size_t)k * sizeof(Pick) + sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    uint32_t made = 0;
    std::memcpy(&made, &got[(size_t)k], sizeof made);
    if (e == hipSuccess && made != (uint32_t)k) e = hipErrorUnknown;  // the kernel left early: no record past `made` is valid
    if (e != hipSuccess) {
        if (err) *err = e;
        return kDiverseHip;
    }
    for (int32_t j = 0; j < k; ++j) {
        out_uid[j] = got[(size_t)j].uid;
        out_r[j] = got[(size_t)j].r;
        if (out_pen) out_pen[j] = got[(size_t)j].pen;
        if (out_value) out_value[j] = got[(size_t)j].value;
        if (out_pos) out_pos[j] = got[(size_t)j].pos;
    }
    *count = k;
    return kDiverseOk;
}

}  // namespace pf
