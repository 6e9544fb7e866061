// Host check of a scan call's options (csrc/pf_scan_call.h): the truth table of make_scan_call, the
// one builder of a call's ScanCall, of its accessors and of extras_ok, what every launcher asks.
// Prints "ok <cases>" or the first violation.
#include <climits>
#include <cstdio>
#include <cstring>

#include "pf_scan_call.h"

static long cases = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        ++cases;                                                     \
        if (!(cond)) {                                               \
            std::printf("line %d: %s\n", __LINE__, #cond);           \
            return 1;                                                \
        }                                                            \
    } while (0)

static bool same(const pf::ScanWindow& a, const pf::ScanWindow& b) {
    return a.lo == b.lo && a.hi == b.hi && a.theta0 == b.theta0 && a.fields == b.fields;
}

int main() {
    pf::CandFilter filt{};
    filt.fields = pf::kFiltAge;
    filt.age_min = 18;
    filt.age_max = 30;
    const pf::FieldSel sel{pf::kSelAge | pf::kSelClubs, 1u, 5ull};
    const int32_t uids[4] = {10, 20, 30, 40};
    uint64_t buf[4];
    uint32_t words[8];
    const uint32_t kBoth = pf::kWinCollect | pf::kWinCount;

    // no window, no collector: everything passes, nothing counted (the words on offer are left out)
    {
        const pf::ScanCall C = pf::make_scan_call(filt, sel, pf_scan_window{}, uids, 4, 0, buf, words);
        for (const pf::ScanWindow& W : {C.win, C.win_idx}) CHECK(W.fields == 0u && W.lo == 0ull && W.hi == ~0ull && W.theta0 == 0u);
        CHECK(C.totals == nullptr && C.collect == nullptr && C.collect_cap == 0u);
        CHECK(std::memcmp(&C.filt, &filt, sizeof filt) == 0 && std::memcmp(&C.sel, &sel, sizeof sel) == 0);
        const pf::ScanExtras x = C.k5(3);
        CHECK(x.totals == nullptr && x.collect == nullptr && x.collect_cap == 0u && x.win.fields == 0u);
        CHECK(std::memcmp(&x.filt, &filt, sizeof filt) == 0 && std::memcmp(&x.sel, &sel, sizeof sel) == 0);
        CHECK(pf::extras_ok(x, 1) && pf::extras_ok(C.k1(), 256));
    }
    // a collector over no window: the device-only bits, every key in the window, an unseeded K5
    {
        const pf::ScanCall C = pf::make_scan_call(filt, sel, pf_scan_window{}, uids, 4, 3, buf, words);
        for (const pf::ScanWindow& W : {C.win, C.win_idx}) CHECK(W.fields == kBoth && W.lo == 0ull && W.hi == ~0ull && W.theta0 == 0u);
        CHECK(C.totals == words && C.collect == buf && C.collect_cap == 3u);
        CHECK(pf::extras_ok(C.k1(), 1) && pf::extras_ok(C.k5(0), 1));
    }
    // a collector over a floor keeps the floor's hi and theta0
    {
        pf_scan_window w{};
        w.fields = PF_WIN_MIN;
        w.min_score = 0.5f;
        const pf::ScanWindow F = pf::window_make(pf::kWinMin, 0.5f, 0.f, 0);
        const pf::ScanCall C = pf::make_scan_call(filt, sel, w, uids, 4, 4, buf, words);
        CHECK(F.theta0 != 0u && F.hi != ~0ull);
        for (const pf::ScanWindow& W : {C.win, C.win_idx})
            CHECK(W.fields == (pf::kWinMin | kBoth) && W.lo == 0ull && W.hi == F.hi && W.theta0 == F.theta0);
    }
    // a cursor: K5's lo names the first idx whose uid exceeds after_uid; the uid-keyed window is window_make's
    {
        const struct { int32_t after; uint32_t first; } tab[] = {
            {20, 2u}, {25, 2u}, {5, 0u}, {40, 4u}, {41, 4u}, {INT32_MAX, 4u}, {INT32_MIN, 0u}};
        for (const auto& t : tab) {
            pf_scan_window w{};
            w.fields = PF_WIN_AFTER | PF_WIN_MIN;
            w.min_score = 0.25f;
            w.after_score = 0.75f;
            w.after_uid = t.after;
            const pf::ScanWindow U = pf::window_make(w.fields, w.min_score, w.after_score, w.after_uid);
            const pf::ScanCall C = pf::make_scan_call(filt, sel, w, uids, 4, 0, nullptr, nullptr);
            CHECK(same(C.win, U));
            CHECK(C.win_idx.lo == (((uint64_t)pf::window_score_word(0.75f) << 32) | (t.first ^ 0x80000000u)));
            CHECK(C.win_idx.hi == U.hi && C.win_idx.theta0 == U.theta0 && C.win_idx.fields == U.fields);
            // at the cursor's score exactly the users above the cursor's uid pass, in both forms
            for (uint32_t x = 0; x < 4; ++x) {
                CHECK(pf::window_pass(pf::window_key(0.75f, (int32_t)x), C.win_idx) == (uids[x] > t.after));
                CHECK(pf::window_pass(pf::window_key(0.75f, uids[x]), C.win) == (uids[x] > t.after));
            }
            CHECK(C.totals == nullptr && C.collect == nullptr);
        }
        // an empty corpus: idx 0 = n
        pf_scan_window w{};
        w.fields = PF_WIN_AFTER;
        w.after_score = 0.75f;
        w.after_uid = 7;
        const pf::ScanCall C = pf::make_scan_call(filt, sel, w, uids, 0, 0, nullptr, nullptr);
        CHECK(C.win_idx.lo == (((uint64_t)pf::window_score_word(0.75f) << 32) | 0x80000000u));
    }
    // PF_WIN_COUNT without a collector: counted, not collecting; the accessors' rows
    {
        pf_scan_window w{};
        w.fields = PF_WIN_COUNT;
        const pf::ScanCall C = pf::make_scan_call(filt, sel, w, uids, 4, 0, buf, words);
        CHECK(C.win.fields == pf::kWinCount && C.win_idx.fields == pf::kWinCount);
        CHECK(C.totals == words && C.collect == nullptr && C.collect_cap == 0u);
        CHECK(C.k5(5).totals == words + 5 && C.k5(0).totals == words && C.k5().totals == words);
        CHECK(C.k1().totals == words && C.group(2).totals == words + 2 && C.group(0).totals == words);
        CHECK(same(C.k5(5).win, C.win_idx) && same(C.k1().win, C.win) && same(C.group(2).win, C.win));
        CHECK(pf::extras_ok(C.k1(), 256) && pf::extras_ok(C.k5(5), 1));
        // ... and without its words: refused
        const pf::ScanCall N = pf::make_scan_call(filt, sel, w, uids, 4, 0, buf, nullptr);
        CHECK(N.totals == nullptr && N.k5(5).totals == nullptr);
        CHECK(!pf::extras_ok(N.k1(), 1) && !pf::extras_ok(N.k5(0), 1));
    }
    // extras_ok on a collecting launch: one query, a buffer, a cap in (0, INT32_MAX]
    {
        const pf::ScanCall C = pf::make_scan_call(filt, sel, pf_scan_window{}, uids, 4, 4, buf, words);
        pf::ScanExtras x = C.k1();
        CHECK(pf::extras_ok(x, 1) && !pf::extras_ok(x, 2) && !pf::extras_ok(x, 0));
        x.collect = nullptr;
        CHECK(!pf::extras_ok(x, 1));
        x = C.k1();
        x.collect_cap = 0u;
        CHECK(!pf::extras_ok(x, 1));
        x.collect_cap = (uint32_t)INT32_MAX;
        CHECK(pf::extras_ok(x, 1));
        x.collect_cap = (uint32_t)INT32_MAX + 1u;
        CHECK(!pf::extras_ok(x, 1));
        x = C.k1();
        x.win.fields &= ~pf::kWinCount;  // a collecting launch is a counting one
        CHECK(!pf::extras_ok(x, 1));
        x = C.k1();
        x.totals = nullptr;
        CHECK(!pf::extras_ok(x, 1));
        // a buffer without the bit
        x = C.k1();
        x.win.fields &= ~pf::kWinCollect;
        CHECK(!pf::extras_ok(x, 1));
        x.collect = nullptr;
        CHECK(pf::extras_ok(x, 1) && pf::extras_ok(x, 2));
    }
    std::printf("ok %ld scan call cases\n", cases);
    return 0;
}
