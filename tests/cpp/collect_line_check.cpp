// collect_line_check.cpp — the collector's word all=<cap> of the api_cli's MATCH and GROUP lines
// (csrc/match_line.h), without an engine: it parses on MATCH (parse_match_line) and as GROUP's words
// (parse_collect_word next to parse_window_word, as csrc/api_cli.cpp walks them), malformed values are
// refused, and a line without the word parses to the struct it parsed to before.  Prints "ok <checks>".
// Test infrastructure only (tests/test_scan_collect_cpu.py).
#include <cstdio>
#include <cstring>
#include <string>

#include "match_line.h"

static int checks = 0;
static bool expect(bool ok, const char* what) {
    if (!ok) std::printf("mismatch: %s\n", what);
    ++checks;
    return ok;
}

static bool same_but_collect(const pokec::MatchLine& a, const pokec::MatchLine& b) {
    return a.topk == b.topk && a.pub == b.pub && a.gen == b.gen && a.comp == b.comp && a.age == b.age &&
           std::memcmp(a.reg, b.reg, sizeof a.reg) == 0 && a.clubs == b.clubs && a.friends == b.friends && a.exclude == b.exclude &&
           std::memcmp(&a.window, &b.window, sizeof a.window) == 0 && a.cols == b.cols;
}

int main() {
    using namespace pokec;
    bool ok = true;
    MatchLine m, p;
    std::string why;
    const std::string base = " 7 public=1 gender=0 age=25 region=3,,27 clubs=4,9 exclude=11,12 c0=5:2,6:1 min=0.25 count";
    // MATCH: the word is taken wherever it stands, the rest of the struct is what it was
    ok &= expect(parse_match_line(base, 3, p, why) && p.collect == 0, "a line without the word");
    ok &= expect(p.window.fields == (PF_WIN_MIN | PF_WIN_COUNT) && p.window.min_score == 0.25f && p.topk == 7, "the plain line's struct");
    ok &= expect(parse_match_line(base + " all=5000", 3, m, why) && m.collect == 5000 && same_but_collect(m, p), "all= at the end");
    ok &= expect(parse_match_line(" 7 all=1 public=1 gender=0 age=25 region=3,,27 clubs=4,9 exclude=11,12 c0=5:2,6:1 min=0.25 count", 3, m, why) &&
                 m.collect == 1 && same_but_collect(m, p), "all= first");
    ok &= expect(parse_match_line(" 0 all=2147483647", 3, m, why) && m.collect == 2147483647LL && m.topk == 0 && m.window.fields == 0u,
                 "the largest cap, no window");
    ok &= expect(parse_match_line(" 7 all=3 all=9", 3, m, why) && m.collect == 9, "the last all= holds");
    for (const char* bad : {"all=", "all=0", "all=-1", "all=+5", "all=2147483648", "all=1e3", "all=12x", "all=0x10", "all= 5", "all=5,6"}) {
        const bool parsed = parse_match_line(std::string(" 7 ") + bad, 3, m, why);
        // ("all= 5" is two words: "all=" is malformed whatever follows)
        ok &= expect(!parsed && why.find("all=") != std::string::npos, bad);
    }
    ok &= expect(!parse_match_line(" 7 al=5", 3, m, why) && !parse_match_line(" 7 ALL=5", 3, m, why), "other keys stay unknown");
    // GROUP's walk: every word goes to parse_window_word first, then to parse_collect_word
    {
        pf_scan_window win{};
        int64_t cap = 0;
        int taken = 0, bad = 0, other = 0;
        for (const char* w : {"101", "min=0.3", "all=640", "noadj", "102", "count", "exclude=7,8"}) {
            const int ww = parse_window_word(w, win);
            const int cw = ww == 0 ? parse_collect_word(w, cap) : 0;
            taken += ww > 0 || cw > 0;
            bad += ww < 0 || cw < 0;
            other += ww == 0 && cw == 0;
        }
        ok &= expect(taken == 3 && bad == 0 && other == 4 && cap == 640 && win.fields == (PF_WIN_MIN | PF_WIN_COUNT), "GROUP's words");
        int64_t keep = 77;
        ok &= expect(parse_collect_word("all=0", keep) == -1 && keep == 77 && parse_collect_word("all=abc", keep) == -1 &&
                     parse_collect_word("alls=5", keep) == 0 && parse_collect_word("count", keep) == 0 && keep == 77,
                     "a malformed or foreign word leaves the cap alone");
        pf_scan_window w2{};
        ok &= expect(parse_window_word("all=5", w2) == 0 && w2.fields == 0u, "all= is no window word");
    }
    if (!ok) return 1;
    std::printf("ok %d\n", checks);
    return 0;
}
