// clubs_line_check.cpp — the clubs-by-interest words topclubs=<topk> and m=<M> of the api_cli's MATCH and
// GROUP lines (csrc/match_line.h), without an engine: they parse on MATCH (parse_match_line) and as
// GROUP's words (parse_clubs_word after parse_window_word and parse_collect_word, as csrc/api_cli.cpp
// walks them), malformed values are refused, MATCH's clubs=<id,..> is still the profile's club list, and a
// line without the words parses to the struct it parsed to before.  Prints "ok <checks>".
// Test infrastructure only (tests/test_club_interest_cpu.py).
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

static bool same_but_clubs(const pokec::MatchLine& a, const pokec::MatchLine& b) {
    return a.topk == b.topk && a.pub == b.pub && a.gen == b.gen && a.comp == b.comp && a.age == b.age &&
           std::memcmp(a.reg, b.reg, sizeof a.reg) == 0 && a.clubs == b.clubs && a.friends == b.friends && a.exclude == b.exclude &&
           std::memcmp(&a.window, &b.window, sizeof a.window) == 0 && a.cols == b.cols && a.collect == b.collect;
}

int main() {
    using namespace pokec;
    bool ok = true;
    MatchLine m, p;
    std::string why;
    const std::string base = " 7 public=1 gender=0 age=25 region=3,,27 clubs=4,9 exclude=11,12 c0=5:2,6:1 min=0.25 all=900";
    ok &= expect(parse_match_line(base, 3, p, why) && p.club_topk == 0 && p.club_m == -1, "a line without the words");
    ok &= expect(p.clubs.size() == 2 && p.clubs[0] == 4u && p.clubs[1] == 9u && p.collect == 900, "clubs= is the profile's list");
    ok &= expect(parse_match_line(base + " topclubs=5", 3, m, why) && m.club_topk == 5 && m.club_m == -1 && same_but_clubs(m, p),
                 "topclubs= at the end");
    ok &= expect(parse_match_line(" 7 m=64 topclubs=1048576 public=1 gender=0 age=25 region=3,,27 clubs=4,9 exclude=11,12 c0=5:2,6:1 min=0.25 all=900",
                                  3, m, why) && m.club_topk == (1 << 20) && m.club_m == 64 && same_but_clubs(m, p), "m= before topclubs=, first");
    ok &= expect(parse_match_line(" 0 topclubs=3 m=0", 3, m, why) && m.club_topk == 3 && m.club_m == 0 && m.topk == 0, "m=0: the whole window");
    ok &= expect(parse_match_line(" 0 topclubs=3 m=2147483647 topclubs=9", 3, m, why) && m.club_topk == 9 && m.club_m == 2147483647,
                 "the largest m; the last topclubs= holds");
    ok &= expect(!parse_match_line(" 7 m=5", 3, m, why) && why.find("topclubs") != std::string::npos, "m= without topclubs=");
    for (const char* bad : {"topclubs=", "topclubs=0", "topclubs=-1", "topclubs=+5", "topclubs=1048577", "topclubs=1e3", "topclubs=4,9",
                            "topclubs=5 m=", "topclubs=5 m=-1", "topclubs=5 m=2147483648", "topclubs=5 m=+1", "topclubs=5 m=1x"}) {
        const bool parsed = parse_match_line(std::string(" 7 ") + bad, 3, m, why);
        ok &= expect(!parsed && why.find("bad value") != std::string::npos, bad);
    }
    ok &= expect(!parse_match_line(" 7 topclub=5", 3, m, why) && !parse_match_line(" 7 M=5 topclubs=2", 3, m, why), "other keys stay unknown");
    // GROUP's walk
    {
        pf_scan_window win{};
        int64_t cap = 0;
        int32_t topk = 0, mm = -1;
        int taken = 0, bad = 0, other = 0;
        for (const char* w : {"101", "min=0.3", "all=640", "topclubs=12", "noadj", "102", "m=65", "exclude=7,8"}) {
            const int ww = parse_window_word(w, win);
            const int cw = ww == 0 ? parse_collect_word(w, cap) : 0;
            const int kw = ww == 0 && cw == 0 ? parse_clubs_word(w, topk, mm) : 0;
            taken += ww > 0 || cw > 0 || kw > 0;
            bad += ww < 0 || cw < 0 || kw < 0;
            other += ww == 0 && cw == 0 && kw == 0;
        }
        ok &= expect(taken == 4 && bad == 0 && other == 4 && cap == 640 && topk == 12 && mm == 65 && win.fields == PF_WIN_MIN, "GROUP's words");
        int32_t keep_t = 77, keep_m = 5;
        ok &= expect(parse_clubs_word("topclubs=0", keep_t, keep_m) == -1 && parse_clubs_word("m=x", keep_t, keep_m) == -1 && keep_t == 77 &&
                     keep_m == 5 && parse_clubs_word("min=0.5", keep_t, keep_m) == 0 && parse_clubs_word("mean", keep_t, keep_m) == 0 &&
                     parse_clubs_word("max", keep_t, keep_m) == 0, "a malformed word changes nothing; min= / mean / max are not club words");
    }
    if (!ok) return 1;
    std::printf("ok %d\n", checks);
    return 0;
}
