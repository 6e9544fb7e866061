// K5's theta derivation by slabs (csrc/pf_prune.h: prune_slab_bin, prune_bin_live, prune_slabs,
// prune_pick, the text the kernel's prune_derive runs) against a serial scan of the histogram from
// its top bin.  The wave is run lane by lane: per slab the 64 lanes' counts, their inclusive sums,
// the pick, the count carried to the next slab; the loop ends like the kernel's (no live slab left,
// or k reached).  A pending record (the workgroup's own, counted in registers, not yet in the
// histogram) must give what the serial scan gives with the record added.
// Expected: the serial answer (the lower edge of the bin where the count from above reaches k)
// whenever it exceeds thb, otherwise thb.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pf_prune.h"

using namespace pf;

static uint32_t serial(const std::vector<uint32_t>& h, uint32_t k, uint32_t thb) {
    uint32_t run = 0;
    for (int b = kPruneBins - 1; b >= 0; --b) {
        run += h[b];
        if (run >= k) return prune_edge(b) > thb ? prune_edge(b) : thb;
    }
    return thb;
}
static int serial_bin(const std::vector<uint32_t>& h, uint32_t k) {
    uint32_t run = 0;
    for (int b = kPruneBins - 1; b >= 0; --b) {
        run += h[b];
        if (run >= k) return b;
    }
    return -1;
}

static long g_loads = 0;  // slabs read, for the report
static uint32_t slabs(const std::vector<uint32_t>& h, uint32_t k, uint32_t thb, uint32_t rec) {
    const int ns = prune_slabs(thb), rb = rec ? prune_bin(rec) : -2;
    if (ns < 0 || ns > kPruneSlabs) { std::printf("bad slab count %d\n", ns); std::exit(1); }
    uint32_t above = 0, nt = 0;
    int picks = 0;
    for (int i = 0; i < kPruneSlabs; ++i) {
        if (!(i < ns && above < k)) continue;  // the kernel's wave-uniform guard
        ++g_loads;
        uint32_t incl = 0;
        for (int l = 0; l < kPruneSlab; ++l) {
            const int b = prune_slab_bin(i, l);
            uint32_t c = 0;
            if (prune_bin_live(b, thb)) {
                if (b < 0 || b >= kPruneBins) { std::printf("live bin %d out of range\n", b); std::exit(1); }
                c = h[b] + (b == rb ? 1u : 0u);
            }
            incl += c;
            if (prune_pick(above, incl, c, k)) { nt = prune_edge(b); ++picks; }
        }
        above += incl;
    }
    if (picks > 1) { std::printf("%d lanes picked\n", picks); std::exit(1); }
    return nt > thb ? nt : thb;
}

static long g_cases = 0;
static void one(const std::vector<uint32_t>& h, uint32_t k, uint32_t thb, uint32_t rec, const char* what) {
    std::vector<uint32_t> hr = h;
    if (rec) hr[prune_bin(rec)] += 1;
    const uint32_t want = serial(hr, k, thb), got = slabs(h, k, thb, rec);
    ++g_cases;
    if (want != got) {
        std::printf("mismatch (%s): k=%u thb=%08x rec=%08x want %08x got %08x\n", what, k, thb, rec, want, got);
        std::exit(1);
    }
}

// every thb the issue names, for one histogram and k: 0, every bin edge hit, one bin either side of the answer
static void sweep(const std::vector<uint32_t>& h, uint32_t k, const char* what) {
    one(h, k, 0u, 0u, what);
    for (int b = 0; b < kPruneBins; ++b)
        if (h[b]) one(h, k, prune_edge(b), 0u, what);
    const int a = serial_bin(h, k);
    for (int d = -1; d <= 1; ++d)
        if (a + d >= 0 && a + d < kPruneBins) one(h, k, prune_edge(a + d), 0u, what);
    one(h, k, prune_edge(kPruneBins - 1), 0u, what);  // thb in the top bin: no slab is read
    // a pending record in the answer's bin, next to it, at the top and at the bottom
    const int rbs[5] = {a, a + 1, a - 1, kPruneBins - 1, 0};
    for (int rb : rbs) {
        if (rb < 0 || rb >= kPruneBins) continue;
        const uint32_t rec = prune_edge(rb) + 5u;
        one(h, k, 0u, rec, what);
        if (a >= 0) one(h, k, prune_edge(a), rec, what);
        if (a >= 1) one(h, k, prune_edge(a - 1), rec, what);
    }
}

int main() {
    const uint32_t ks[3] = {1, 10, 64};
    std::mt19937 rng(12345);
    for (uint32_t k : ks) {
        std::vector<uint32_t> h(kPruneBins, 0u);
        sweep(h, k, "empty");
        // random histograms: sparse (a few records, as early in a launch) to dense
        for (int rep = 0; rep < 60; ++rep) {
            std::fill(h.begin(), h.end(), 0u);
            const int n = 1 + (int)(rng() % (rep < 20 ? 8 : rep < 40 ? 200 : 5000));
            const int lo = (int)(rng() % kPruneBins);
            for (int i = 0; i < n; ++i) h[lo + (int)(rng() % (uint32_t)(kPruneBins - lo))] += 1 + (rng() % 3 == 0 ? rng() % 5 : 0);
            sweep(h, k, "random");
        }
        // the count reaches k exactly at a slab boundary: at a slab's last lane, at the next one's
        // first, and k - 1 at the end of one slab with the k-th record at the start of the next
        for (int s = 0; s + 1 < kPruneSlabs; ++s) {
            const int last = prune_slab_bin(s, kPruneSlab - 1), first = prune_slab_bin(s + 1, 0);
            std::fill(h.begin(), h.end(), 0u);
            h[last] = k;
            sweep(h, k, "boundary: last lane");
            std::fill(h.begin(), h.end(), 0u);
            h[first] = k;
            sweep(h, k, "boundary: first lane");
            std::fill(h.begin(), h.end(), 0u);
            h[last] = k - 1;
            h[first] = 1;
            if (first > 0) h[first - 1] = 7;
            sweep(h, k, "boundary: straddled");
            std::fill(h.begin(), h.end(), 0u);
            h[kPruneBins - 1] = k - 1;  // spread: top bin, then the boundary
            h[last] += 1;
            h[first] += 3;
            sweep(h, k, "boundary: spread");
        }
        std::fill(h.begin(), h.end(), 0u);
        h[0] = k;  // the lowest bin, in the last (one-bin) slab
        sweep(h, k, "lowest bin");
    }
    std::printf("ok %ld cases, %ld slab reads\n", g_cases, g_loads);
    return 0;
}
