// pf_collect.h — the scans' collector (pokec_fas.h "Collect"): one scan appends every key of its score
// window to a device buffer, one device sort puts the keys in the engine's order.
//   the append   pf_kernels.hip collect_append, at the three keying points where a counted window
//                counts (K5's WIN instantiations, K1, the group kernel's last pass).  A collecting
//                launch is a counting one (kWinCollect comes with kWinCount): the total is the count
//                word, the cursor (ScanSync::ccursor) only hands out slots.
//   the finish   collect_sort below, once the host has read the total and it fits the buffer.
// The buffer and its cap travel by value with each launch, like the window (pf_scan_call.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pf {

// Temporary storage hipCUB's radix sort takes for n 64-bit keys
hipError_t collect_sort_bytes(int64_t n, size_t* bytes);
// keys[0, n) sorted ascending into sorted[0, n) on s: ascending key order is (score desc, uid asc)
// (pf_types.h score_key), and uids are unique, so the result does not depend on arrival order
hipError_t collect_sort(const uint64_t* keys, uint64_t* sorted, int64_t n, void* tmp, size_t tmp_bytes, hipStream_t s);

}  // namespace pf
