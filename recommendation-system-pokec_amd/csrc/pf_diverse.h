// pf_diverse.h — diverse top-k (pokec_fas.h "Diverse top-k"): the selection stage between a pool of
// M <= 1024 users with float relevances, a device matrix of their pair scores, and the list of picks.
// Per pick, in the arithmetic of the definition (three separately rounded double ops, never fused:
// the build is -ffp-contract=off),
//     a = (double)lambda * (double)r_i;  p = (1.0 - (double)lambda) * (double)pen_i;  v_i = a - p
// the unpicked position with the largest v wins, ties to the smallest position; then
//     pen_i = sim[s * stride + i] > pen_i ? sim[s * stride + i] : pen_i      (row s: the pick on the A side).
// One launch of one workgroup of ceil(M / 64) waves: lane i owns position i and keeps r_i, pen_i and its
// picked flag in registers.  A pick is a wave argmax (the double's orderable 64 bits, inverted, through
// wave_min64 of pf_device.h; the lowest lane among the equals by ballot), the waves' winners in LDS, and
// the same reduction over them.  Every wave reduces the winners for itself, out of a slot that
// alternates with the pick's parity: one barrier per pick, and no broadcast to wait for.  Only row s of
// the matrix is read, one coalesced 4-byte load per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_dbuf.h"

namespace pf {

constexpr int kDiverseMaxPool = 1024;  // PF_DIVERSE_MAX_POOL: one workgroup's lanes

struct DiverseIn {
    // the pool, in its order: either ranked keys (pf_types.h score_key: r and the uid are decoded on the
    // device as pf_decode_keys decodes them) or, with keys == nullptr, plain arrays.  Device pointers.
    const uint64_t* keys;
    const int32_t* uid;
    const float* rel;
    int32_t m;           // 0 .. kDiverseMaxPool
    const float* sim;    // device: sim[s * stride + i], rows and columns in pool order
    int64_t stride;      // >= m
    float lambda;        // in [0, 1]
    int32_t topk;        // >= 0
};

// grows on demand; lives in the context
struct DiverseWs {
    DBuf picks;  // the launch's output records
    DBuf sim;    // the callers' matrix (pf_diverse_api.cpp); the stage itself never allocates it
    DBuf pool;   // a by-list call's uids and relevances
};

enum DiverseStatus { kDiverseOk = 0, kDiverseNoMem, kDiverseHip };

// Runs the stage on s and synchronises it.  out_*: host arrays of min(topk, m) entries in pick order
// (out_pos: the pool positions; it, out_pen and out_value may be nullptr); *count = entries written.
// Nothing is launched when m == 0 or topk == 0.  kDiverseNoMem: the output buffer cannot be had;
// kDiverseHip: *err holds the HIP error (hipErrorInvalidValue for arguments outside the limits above).
// The kernel also reports how many picks it made: fewer than min(topk, m) (it leaves a pick nobody can win,
// which finite values never produce) is kDiverseHip with hipErrorUnknown, not a list of stale records.
// No load goes past row m - 1 or column m - 1 of the matrix, no store past min(topk, m) records.
DiverseStatus diverse_run(const DiverseIn& in, DiverseWs& ws, hipStream_t s, int32_t* out_uid, float* out_r, float* out_pen,
                          double* out_value, int32_t* out_pos, int32_t* count, hipError_t* err);

}  // namespace pf
