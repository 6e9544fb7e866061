// pf_scan_call.h — what an all-candidates scan carries besides its query: the options of one call
// (ScanCall) and their form in one launch's arguments (ScanExtras).  A call's options are a value,
// built once by make_scan_call and passed down the launch chain; nothing on the way reads them from
// the context.  Plain C++ with no HIP include, so the CPU test (tests/cpp/scan_call_check.cpp)
// compiles it with g++.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "pf_filter.h"
#include "pf_select.h"
#include "pf_window.h"
#include "pokec_fas.h"

namespace pf {

// One launch's share, passed by value in the kernel's arguments in this order.
struct ScanExtras {
    CandFilter filt;  // the candidate filter (pf_filter.h; fields == 0: none)
    // the field selection (pf_select.h; on == 0: none), applied to each block's staged copy of its
    // query's constants; K5 takes its SEL instantiation, which leaves the deselected lists out
    FieldSel sel;
    // the score window (pf_window.h; fields == 0: none), keyed as the kernel keys: by uid for K1 and
    // the group kernel (on the aggregate's key, in the last pass), by idx for K5 (its WIN
    // instantiation and kWinLds bytes)
    ScanWindow win;
    // a counted window (kWinCount): the device words the launch adds its counts to, query q's at
    // totals[its result row] (a one-query K5 launch and the group kernel write totals[0]); else nullptr
    uint32_t* totals;
    // a collecting window (kWinCollect, which comes with kWinCount): the device buffer the launch's
    // one query appends its in-window keys to, and its cap in keys; else nullptr / 0
    uint64_t* collect;
    uint32_t collect_cap;
};

// What every launcher asks before it launches nq queries: a counted window has its count words; a
// collecting one has one query, a count, a buffer and a cap that fits the kernels' 32-bit slots; a
// launch that does not collect carries no buffer.
inline bool extras_ok(const ScanExtras& E, int nq) {
    if ((E.win.fields & kWinCount) && !E.totals) return false;
    if (!(E.win.fields & kWinCollect)) return E.collect == nullptr;
    return nq == 1 && (E.win.fields & kWinCount) && E.collect != nullptr && E.collect_cap > 0u &&
           E.collect_cap <= (uint32_t)INT32_MAX;
}

// The options of one call.  The launches get absolute result rows and `totals`, the base of the call's
// count words.  A batch launch indexes the words by its own rows, so it takes the base (k1(), k5() with
// no row: an offset here would count twice); a launch that counts its one query into word 0 names
// that query's row (k5(row) for K5's one-query launch, group(row) for the group kernel).
struct ScanCall {
    CandFilter filt;
    FieldSel sel;
    ScanWindow win, win_idx;  // uid-keyed (K1, the group kernel) and idx-keyed (K5)
    uint32_t* totals;         // nullptr: not counted
    uint64_t* collect;        // nullptr / 0: not collecting
    uint32_t collect_cap;
    ScanExtras k1() const { return group(0); }
    ScanExtras group(int32_t row) const { return {filt, sel, win, totals ? totals + row : nullptr, collect, collect_cap}; }
    ScanExtras k5(int32_t row = 0) const { return {filt, sel, win_idx, totals ? totals + row : nullptr, collect, collect_cap}; }
};

// A call's options from the sticky filter and selection, the public window (validated: known bits, no
// NaN; fields == 0: none), the corpus's uids in idx order, the collector's cap in keys with its
// device buffer (cap 0: none), and the call's zeroed count words (kept only by a counted call).
// The one place that sets the device-only bits of a collecting call, and the one that turns the
// cursor's uid into K5's idx bound: the first idx whose uid exceeds it, n when none does.  No heap
// allocation, and no search without a cursor: the asynchronous one-query path builds one per call.
inline ScanCall make_scan_call(const CandFilter& filt, const FieldSel& sel, const pf_scan_window& w, const int32_t* uids,
                               size_t n_uids, int64_t cap, uint64_t* buf, uint32_t* totals) {
    ScanCall C{filt, sel, window_make(w.fields, w.min_score, w.after_score, w.after_uid), {}, nullptr, nullptr, 0u};
    if (cap > 0) {
        C.win.fields |= kWinCollect | kWinCount;
        C.collect = buf;
        C.collect_cap = (uint32_t)cap;
    }
    if (C.win.fields & kWinCount) C.totals = totals;
    C.win_idx = C.win;
    if (C.win.fields & kWinAfter)
        C.win_idx = window_for_idx(C.win, w.after_score, (uint32_t)(std::upper_bound(uids, uids + n_uids, w.after_uid) - uids));
    return C;
}

}  // namespace pf
