// pf_dbuf.h — a device buffer that only grows: the workspaces of the context (pf_ctx.h) and of the
// stages that keep their own (pf_clubsum.h).  Contents are not kept across a growth.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace pf {

struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes, 4096);
        want = want + want / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    // per-call workspaces: grow to twice the request (at least 1 MiB), so the sizes of
    // successive batches settle after a few calls instead of re-allocating (hipFree syncs)
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        return ensure(std::max<size_t>(2 * bytes, 1u << 20));
    }
    ~DBuf() {
        if (p) (void)hipFree(p);
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace pf
