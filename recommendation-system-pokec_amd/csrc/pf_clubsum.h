// pf_clubsum.h — clubs by interest (pokec_fas.h "Clubs by interest"): the stage between a collecting
// scan's ranked keys and a ranked club list.  Per club, in the order of the definition,
//     double acc = 0;  for every neighbour in rank order with w = (double)score > 0:
//                          acc += w for every occurrence of the club in its list (profile order)
// and the club's score is (float)acc.  The order of the adds is the contract (as K7's, pf_jobs.hip):
// every contribution of a club is added by ONE thread, in ascending rank.
//   own       the own-club list, as dense indices, becomes a bitmap over the dense club indices in
//             global memory (n_club_ids bits): a list of 65,535 entries is 256 KiB as words, more than a
//             workgroup's LDS, and a bitmap is one path for every size.
//   count     per ranked neighbour: its uid's profile index (binary search of the sorted uid table, on
//             the device: nothing is mapped on the host), its clubs not in `own`; 0 when w <= 0.  A
//             workgroup's counts are summed (pf_block.h) to one word per workgroup.
//   place     an exclusive sum of the workgroups' words (hipCUB): the total C reaches the host before
//             any buffer of C entries is allocated.
//   emit      the same workgroups scan their counts (pf_block.h block_scan_incl) and write one key per
//             contribution, (dense club << rank_bits) | rank: rank_bits = bit width of used - 1, so the
//             sort below sees no idle bits between the two parts.
//   sort      one hipCUB radix sort over the rank_bits + club bits in use: every club is one run,
//             ranks ascend inside it; equal keys (a club listed twice by one neighbour) are adjacent and
//             carry the same weight.
//   sum       one thread per run head adds the run in order while it is shorter than the cut-over;
//             a run that reaches the cut-over goes to a list, and one wave per listed run loads 64
//             weights at a time (coalesced keys, gathered scores) and its first lane adds them in order.
//             The weight is decoded from keys[rank]: no value array goes through the sort.
//   rank      score_key((float)acc, club id) per run, one hipCUB sort of the runs' keys (at most one per
//             club), the first topk copied out: every topk is served (the wave top-k of pf_device.h
//             stops at 64).
// The host reads three words on the way (C, the run count, the results): three synchronisations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_dbuf.h"

namespace pf {

constexpr int kClubSumThreads = 256;        // a workgroup of count / emit: its scan width
constexpr int kClubSumCutoverDefault = 32;  // runs of this length and longer take the wave path

struct ClubSumIn {
    const uint64_t* keys;        // device: ranked top-k keys (pf_types.h score_key), ascending
    int64_t used;                // the first `used` of them enter; 0 <= used <= INT32_MAX
    const int32_t* uid;          // device: [n_users] the stored uids, ascending (index = profile idx)
    int32_t n_users;
    int32_t n_club_ids;
    const int64_t* club_off;     // device: [n_users + 1]
    const int32_t* club_dense;   // device: dense club indices, per profile in profile order
    const int32_t* club_id;      // device: [n_club_ids] dense index -> club id
    const int32_t* own;          // HOST: dense indices never scored (may repeat); n_own == 0: none
    int32_t n_own;
    int32_t topk;                // >= 0
    int32_t cutover;             // <= 0: kClubSumCutoverDefault
};

// grows on demand; lives in the context
struct ClubSumWs {
    DBuf own, bitmap, cnt, btot, bbase, scan_tmp, ckeys, skeys, sort_tmp, rkeys, rsorted, longs, counters;
};

struct ClubSumOut {
    int64_t contributions = 0;   // C: adds made
    int64_t clubs = 0;           // clubs with at least one contribution
    int32_t count = 0;           // entries written: min(topk, clubs)
    int64_t long_runs = 0;       // runs that took the wave path
};

enum ClubSumStatus { kClubSumOk = 0, kClubSumTooMany, kClubSumNoMem, kClubSumHip };

// Runs the stage on s and synchronises it.  out_club / out_score: host arrays of topk entries, ranked
// (score desc, club id asc).  kClubSumTooMany: C above INT32_MAX; kClubSumNoMem: a workspace cannot be
// had; kClubSumHip: *err holds the HIP error.  No store goes past a buffer: every emit is bounded by C.
ClubSumStatus clubsum_run(const ClubSumIn& in, ClubSumWs& ws, hipStream_t s, int32_t* out_club, float* out_score,
                          ClubSumOut* out, hipError_t* err);

}  // namespace pf
