// pf_stage.h — the byte layout of a scan launch's pinned staging buffer: a few sections, each starting
// on a 16-B boundary, sent to the device in one copy (pf_scan_host.cpp stage_send).  Plain C++ with no
// HIP include, so the CPU test (tests/cpp/stage_check.cpp) compiles it with g++; the element sizes
// (a QImageRef, a ScanSync) are the caller's arguments for the same reason.
#pragma once
#include <stddef.h>

namespace pf {

constexpr size_t stage_round(size_t x) { return (x + 15) & ~(size_t)15; }

// N sections: section i holds size[i] bytes at off[i]; total ends with the last section's last byte
template <int N>
struct StageLayout {
    size_t off[N], size[N], total;
};

template <int N>
inline StageLayout<N> stage_layout(const size_t (&bytes)[N]) {
    StageLayout<N> L{};
    size_t o = 0;
    for (int i = 0; i < N; ++i) {
        L.off[i] = stage_round(o);
        L.size[i] = bytes[i];
        o = L.off[i] + bytes[i];
    }
    L.total = o;
    return L;
}

// The three launches' buffers (sync_b = sizeof(ScanSync), ref_b = sizeof(QImageRef), both multiples of 16):
// K5: [image offsets | result rows | sync x nq | images]
inline StageLayout<4> stage_post_layout(size_t nq, size_t sync_b, size_t pool_b) {
    return stage_layout<4>({nq * 4, nq * 4, nq * sync_b, pool_b});
}
// K1: [refs x nq | result rows | sync x nq | image pool]
inline StageLayout<4> stage_stream_layout(size_t nq, size_t ref_b, size_t sync_b, size_t pool_b) {
    return stage_layout<4>({nq * ref_b, nq * 4, nq * sync_b, pool_b});
}
// the group kernel: [refs x G | carve offsets | one sync | image pool]
inline StageLayout<4> stage_group_layout(size_t G, size_t ref_b, size_t sync_b, size_t pool_b) {
    return stage_layout<4>({G * ref_b, G * 4, sync_b, pool_b});
}

}  // namespace pf
