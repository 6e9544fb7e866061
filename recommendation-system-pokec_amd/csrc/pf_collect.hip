// pf_collect.hip — the collector's finish (pf_collect.h): hipCUB's radix sort over the keys a
// collecting scan appended.  The keys are top-k keys (pf_types.h score_key): all 64 bits take part.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>

#include "pf_collect.h"

namespace pf {

hipError_t collect_sort_bytes(int64_t n, size_t* bytes) {
    if (n < 0 || n > (int64_t)INT32_MAX || !bytes) return hipErrorInvalidValue;
    *bytes = 0;
    const uint64_t* in = nullptr;
    uint64_t* out = nullptr;
    return hipcub::DeviceRadixSort::SortKeys(nullptr, *bytes, in, out, (int)n, 0, 64, nullptr);
}

hipError_t collect_sort(const uint64_t* keys, uint64_t* sorted, int64_t n, void* tmp, size_t tmp_bytes, hipStream_t s) {
    if (n < 0 || n > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    return hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, keys, sorted, (int)n, 0, 64, s);
}

}  // namespace pf
