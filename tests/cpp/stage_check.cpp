// CPU check of csrc/pf_stage.h: the byte layouts of the three staging buffers (K5, K1, the group
// kernel) for nq (or G) in {1, 3, 4, 5} and image pools of {0, 16, 40} bytes.  The expected offsets are
// written out as numbers, worked by hand from the formulas the three launchers used before they shared
// the header: K5 round16(4 nq) twice, then 4288 nq; K1 16 nq, round16(4 nq), 4288 nq; the group
// round16(16 G), round16(4 G), 4288 (sizeof(QImageRef) = 16, sizeof(ScanSync) = 4288).
#include <cstdio>

#include "pf_stage.h"

namespace {

constexpr size_t kRef = 16, kSync = 4288;
int bad = 0;

void check(const char* what, size_t n, size_t pool, const pf::StageLayout<4>& L, const size_t (&off)[4]) {
    for (int i = 0; i < 4; ++i) {
        if (L.off[i] != off[i]) {
            std::printf("%s n=%zu pool=%zu: section %d at %zu, expected %zu\n", what, n, pool, i, L.off[i], off[i]);
            ++bad;
        }
        if (L.off[i] % 16) {
            std::printf("%s n=%zu pool=%zu: section %d at %zu is not 16-B aligned\n", what, n, pool, i, L.off[i]);
            ++bad;
        }
    }
    if (L.total != off[3] + pool) {
        std::printf("%s n=%zu pool=%zu: total %zu, expected %zu\n", what, n, pool, L.total, off[3] + pool);
        ++bad;
    }
    if (L.size[3] != pool) {
        std::printf("%s n=%zu pool=%zu: pool section of %zu bytes\n", what, n, pool, L.size[3]);
        ++bad;
    }
}

}  // namespace

int main() {
    const size_t ns[4] = {1, 3, 4, 5}, pools[3] = {0, 16, 40};
    // [image offsets | rows | sync x nq | images]
    const size_t k5[4][4] = {{0, 16, 32, 4320}, {0, 16, 32, 12896}, {0, 16, 32, 17184}, {0, 32, 64, 21504}};
    // [refs x nq | rows | sync x nq | pool]
    const size_t k1[4][4] = {{0, 16, 32, 4320}, {0, 48, 64, 12928}, {0, 64, 80, 17232}, {0, 80, 112, 21552}};
    // [refs x G | offsets | sync x 1 | pool]
    const size_t gr[4][4] = {{0, 16, 32, 4320}, {0, 48, 64, 4352}, {0, 64, 80, 4368}, {0, 80, 112, 4400}};
    int cases = 0;
    for (int i = 0; i < 4; ++i)
        for (size_t pool : pools) {
            check("k5", ns[i], pool, pf::stage_post_layout(ns[i], kSync, pool), k5[i]);
            check("k1", ns[i], pool, pf::stage_stream_layout(ns[i], kRef, kSync, pool), k1[i]);
            check("group", ns[i], pool, pf::stage_group_layout(ns[i], kRef, kSync, pool), gr[i]);
            cases += 3;
        }
    // the sections' own sizes are the unrounded ones (what is copied)
    const pf::StageLayout<4> L = pf::stage_post_layout(5, kSync, 40);
    if (L.size[0] != 20 || L.size[1] != 20 || L.size[2] != 5 * kSync) {
        std::printf("k5 n=5: section sizes %zu %zu %zu\n", L.size[0], L.size[1], L.size[2]);
        ++bad;
    }
    if (bad) return 1;
    std::printf("ok %d layouts\n", cases);
    return 0;
}
