// pf_block.h — workgroup-wide ranks and prefix sums of the job pipeline's gathers (pf_jobs.hip),
// over ballots and pf_device.h's wave_incl_scan.  NW = waves of the workgroup; wsum is LDS scratch
// of NW ints (2 * NW for block_rank2), free for re-use once a helper returns (trailing barrier).
// tools/probe/topk.hip checks the three against serial prefix sums (tests/test_gpu_topk_primitives.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_device.h"

namespace pf {

// ---------------------------------------------------------------- block helpers
// exclusive rank of `flag` among the block's threads and the block total (ballots + LDS)
template <int NW>
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    const int r = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int x = wsum[w];
        if (w < wave) before += x;
        total += x;
    }
    __syncthreads();
    return before + r;
}

// block_rank for two flags per thread whose items are ordered all-f0-items first (thread order),
// then all f1-items: one LDS exchange (wsum holds 2 * NW words)
template <int NW>
__device__ __forceinline__ void block_rank2(bool f0, bool f1, int* wsum, int& r0, int& r1, int& t0, int& t1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m0 = __ballot(f0), m1 = __ballot(f1);
    const uint64_t below = (1ull << lane) - 1ull;
    r0 = __popcll(m0 & below);
    r1 = __popcll(m1 & below);
    if (lane == 0) {
        wsum[wave] = __popcll(m0);
        wsum[NW + wave] = __popcll(m1);
    }
    __syncthreads();
    int b0 = 0, b1 = 0;
    t0 = t1 = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int x0 = wsum[w], x1 = wsum[NW + w];
        if (w < wave) { b0 += x0; b1 += x1; }
        t0 += x0;
        t1 += x1;
    }
    __syncthreads();
    r0 += b0;
    r1 += t0 + b1;
}

// inclusive prefix of v over the block; total in `total`
template <int NW>
__device__ __forceinline__ int block_scan_incl(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
    x = (int)wave_incl_scan((uint32_t)x);
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int t = wsum[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();
    return before + x;
}

}  // namespace pf
