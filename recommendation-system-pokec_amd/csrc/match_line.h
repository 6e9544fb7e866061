// match_line.h — the api_cli's MATCH command line (csrc/api_cli.cpp): a profile given by value on one
// line, for a person who is not a user of the corpus (pokec_fas.h pf_query_profile).
//
//   MATCH <topk> [public=N] [gender=N] [completion=N] [age=N] [region=a,b,c] [clubs=id,id,..]
//         [friends=id,id,..] [exclude=uid,uid,..] [c<t>=tid:tf,tid:tf,..]...
//
// and the score window's words (pokec_fas.h pf_scan_window), which GROUP takes as well:
//         [min=<float>] [after=<8 hex digits of the score's float bits>:<uid>] [count]
// The cursor token carries the float's bits because printed decimal scores lose them; a reply to a
// line with one of these words ends with "next":"<hex>:<uid>", the last result's cursor.
// A window-like word of both commands asks for the WHOLE window (pokec_fas.h "Collect"):
//         [all=<cap>]      1 <= cap <= 2147483647
// The reply's list is then every candidate of the window, ranked, whatever topk is, and the reply ends
// with "total":N; when N > cap the list is empty and "overflow":true follows.
// The words of clubs by interest (pokec_fas.h "Clubs by interest"), on both commands:
//         [topclubs=<topk>] [m=<M>]      1 <= topk <= 1048576, 0 <= M <= 2147483647
// topclubs adds a "clubs" list to the reply: the clubs of the window's first M neighbours (m=0 or no m:
// the whole window), scored by the neighbours' scores, with names.  (MATCH's clubs=<id,..> is the
// profile's own club list, so the new word cannot be spelt clubs=.)  m without topclubs is malformed.
// The words of diverse top-k (pokec_fas.h "Diverse top-k"), on both commands and on DIVERSE:
//         [diverse=<lambda>] [pool=<M>]      0 <= lambda <= 1, 1 <= M <= 1024 (default 200)
// diverse makes the reply's list the diverse one: the window's first M candidates re-ranked by maximal
// marginal relevance, topk of them, each item with its "pen", and the reply ends with "total" and "pool"
// (so count adds nothing, and no "next" follows: a diverse list has no next page).  pool without diverse
// is malformed, and so is diverse together with all=, topclubs= or m=: the reply holds one list.
//
// A field that is not given is missing; an empty region part ("region=3,,27") is missing; c<t> is
// text column t of the engine's list, as token ids (the text -> id ETL is not part of the engine).
// Engine-free, so the parser is tested without a GPU.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "pokec_fas.h"

namespace pokec {

struct MatchLine {
    int topk = 0;
    int32_t pub = -1, gen = -1, comp = 0, age = 0, reg[3] = {-1, -1, -1};
    std::vector<uint32_t> clubs, friends;
    std::vector<int32_t> exclude;
    pf_scan_window window{};  // fields == 0: the line has none of the window's words
    int64_t collect = 0;      // all=<cap>; 0: the line has no such word
    int32_t club_topk = 0;    // topclubs=<topk>; 0: the line has no such word
    int32_t club_m = -1;      // m=<M>; -1: the line has no such word
    float diverse = -1.f;     // diverse=<lambda>; below 0: the line has no such word
    int32_t diverse_pool = 0; // pool=<M>; 0: the line has no such word
    std::vector<std::vector<std::pair<int32_t, int32_t>>> cols;  // [n_cols] (tid, tf) in the line's order
    // the C struct over this object's arrays (valid while the object lives and is not changed)
    std::vector<int64_t> off;
    std::vector<int32_t> tid, tf;
    pf_query_profile profile() {
        off.assign(1, 0);
        tid.clear();
        tf.clear();
        for (const auto& c : cols) {
            for (const auto& kv : c) { tid.push_back(kv.first); tf.push_back(kv.second); }
            off.push_back((int64_t)tid.size());
        }
        pf_query_profile q{};
        q.public_flag = pub; q.gender = gen; q.completion = comp; q.age = age;
        for (int k = 0; k < 3; ++k) q.region[k] = reg[k];
        q.club_ids = clubs.data(); q.n_clubs = (int32_t)clubs.size();
        q.friend_ids = friends.data(); q.n_friends = (int32_t)friends.size();
        q.tok_off = off.data(); q.tok_tid = tid.data(); q.tok_tf = tf.data();
        q.exclude_uid = exclude.data(); q.n_exclude = (int32_t)exclude.size();
        return q;
    }
};

namespace match_detail {
inline bool to_int(const std::string& s, long long lo, long long hi, long long& v) {
    if (s.empty()) return false;
    char* end = nullptr;
    v = std::strtoll(s.c_str(), &end, 10);
    return *end == '\0' && v >= lo && v <= hi;
}
inline std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out(1);
    for (char c : s) {
        if (c == sep) out.emplace_back();
        else out.back() += c;
    }
    return out;
}
}  // namespace match_detail

// One word of a MATCH / GROUP line as a word of the score window: 1 = taken into `win`, 0 = not a
// window word, -1 = a window word with a malformed value.
inline int parse_window_word(const std::string& w, pf_scan_window& win) {
    if (w == "count") {
        win.fields |= PF_WIN_COUNT;
        return 1;
    }
    if (w.rfind("min=", 0) == 0) {
        const std::string val = w.substr(4);
        char* end = nullptr;
        const float f = std::strtof(val.c_str(), &end);
        if (val.empty() || *end != '\0' || f != f) return -1;
        win.fields |= PF_WIN_MIN;
        win.min_score = f;
        return 1;
    }
    if (w.rfind("after=", 0) == 0) {
        const std::string val = w.substr(6);
        long long uid = 0;
        if (val.size() < 10 || val[8] != ':' || !match_detail::to_int(val.substr(9), INT32_MIN, INT32_MAX, uid)) return -1;
        uint32_t bits = 0;
        for (int i = 0; i < 8; ++i) {
            const char ch = val[(size_t)i];
            const int d = ch >= '0' && ch <= '9' ? ch - '0' : (ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : (ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1));
            if (d < 0) return -1;
            bits = bits << 4 | (uint32_t)d;
        }
        float f;
        std::memcpy(&f, &bits, sizeof f);
        if (f != f) return -1;
        win.fields |= PF_WIN_AFTER;
        win.after_score = f;
        win.after_uid = (int32_t)uid;
        return 1;
    }
    return 0;
}
// One word of a MATCH / GROUP line as the collector's word all=<cap>: 1 = taken into `cap`, 0 = another
// word, -1 = malformed (not a number, below 1, above INT32_MAX)
inline int parse_collect_word(const std::string& w, int64_t& cap) {
    if (w.rfind("all=", 0) != 0) return 0;
    long long v = 0;
    const std::string val = w.substr(4);
    if (val.empty() || val[0] == '+' || val[0] == '-' || !match_detail::to_int(val, 1, INT32_MAX, v)) return -1;
    cap = (int64_t)v;
    return 1;
}
// One word of a MATCH / GROUP / CLUBS line as a word of clubs by interest: 1 = taken, 0 = another word,
// -1 = malformed (not a number, topclubs below 1 or above 2^20, m below 0 or above INT32_MAX)
inline int parse_clubs_word(const std::string& w, int32_t& topk, int32_t& m) {
    const bool is_top = w.rfind("topclubs=", 0) == 0;
    if (!is_top && w.rfind("m=", 0) != 0) return 0;
    const std::string val = w.substr(is_top ? 9 : 2);
    long long v = 0;
    if (val.empty() || val[0] == '+' || val[0] == '-' || !match_detail::to_int(val, is_top ? 1 : 0, is_top ? (1 << 20) : INT32_MAX, v))
        return -1;
    (is_top ? topk : m) = (int32_t)v;
    return 1;
}
// One word of a MATCH / GROUP / DIVERSE line as a word of diverse top-k: 1 = taken, 0 = another word,
// -1 = malformed (lambda not a number in [0, 1], pool not a number in 1 .. PF_DIVERSE_MAX_POOL)
inline int parse_diverse_word(const std::string& w, float& lambda, int32_t& pool) {
    if (w.rfind("diverse=", 0) == 0) {
        const std::string val = w.substr(8);
        char* end = nullptr;
        const float f = std::strtof(val.c_str(), &end);
        if (val.empty() || *end != '\0' || !(f >= 0.f && f <= 1.f)) return -1;
        lambda = f;
        return 1;
    }
    if (w.rfind("pool=", 0) != 0) return 0;
    const std::string val = w.substr(5);
    long long v = 0;
    if (val.empty() || val[0] == '+' || val[0] == '-' || !match_detail::to_int(val, 1, PF_DIVERSE_MAX_POOL, v)) return -1;
    pool = (int32_t)v;
    return 1;
}
// whether the diverse words of a line go together: pool needs diverse, diverse excludes all= and the
// clubs words
inline bool diverse_words_ok(float lambda, int32_t pool, int64_t collect, int32_t club_topk, int32_t club_m) {
    return lambda >= 0.f ? collect == 0 && club_topk == 0 && club_m < 0 : pool == 0;
}
constexpr int32_t kDiversePoolDefault = 200;
// the cursor token of a result: its score's float bits and its uid
inline std::string window_cursor(float score, int32_t uid) {
    uint32_t bits = 0;
    std::memcpy(&bits, &score, sizeof bits);
    char buf[32];
    std::snprintf(buf, sizeof buf, "%08x:%d", bits, uid);
    return buf;
}

// Parses the words after "MATCH" for an engine of n_cols text columns; false with `why` on a
// malformed line (an unknown key, a value that is not a number, a column outside the engine's list).
inline bool parse_match_line(const std::string& rest, int n_cols, MatchLine& m, std::string& why) {
    using namespace match_detail;
    m = MatchLine{};
    m.cols.assign((size_t)n_cols, {});
    std::istringstream iss(rest);
    std::string w;
    long long v = 0;
    if (!(iss >> w) || !to_int(w, 0, 1 << 20, v)) { why = "topk"; return false; }
    m.topk = (int)v;
    const long long i32lo = INT32_MIN, i32hi = INT32_MAX;
    while (iss >> w) {
        const int ww = parse_window_word(w, m.window);
        if (ww < 0) { why = "bad value: " + w; return false; }
        if (ww > 0) continue;
        const int cw = parse_collect_word(w, m.collect);
        if (cw < 0) { why = "bad value: " + w; return false; }
        if (cw > 0) continue;
        const int kw = parse_clubs_word(w, m.club_topk, m.club_m);
        if (kw < 0) { why = "bad value: " + w; return false; }
        if (kw > 0) continue;
        const int dw = parse_diverse_word(w, m.diverse, m.diverse_pool);
        if (dw < 0) { why = "bad value: " + w; return false; }
        if (dw > 0) continue;
        const size_t eq = w.find('=');
        if (eq == std::string::npos || eq == 0) { why = "not key=value: " + w; return false; }
        const std::string key = w.substr(0, eq), val = w.substr(eq + 1);
        auto scalar = [&](int32_t& dst) {
            if (!to_int(val, i32lo, i32hi, v)) return false;
            dst = (int32_t)v;
            return true;
        };
        bool ok = true;
        if (key == "public") ok = scalar(m.pub);
        else if (key == "gender") ok = scalar(m.gen);
        else if (key == "completion") ok = scalar(m.comp);
        else if (key == "age") ok = scalar(m.age);
        else if (key == "region") {
            const auto parts = split(val, ',');
            ok = parts.size() <= 3;
            for (size_t k = 0; ok && k < parts.size(); ++k) {
                if (parts[k].empty()) continue;  // a missing part
                ok = to_int(parts[k], i32lo, i32hi, v);
                m.reg[k] = (int32_t)v;
            }
        } else if (key == "clubs" || key == "friends") {
            auto& dst = key == "clubs" ? m.clubs : m.friends;
            for (const auto& p : split(val, ',')) {
                if (val.empty()) break;
                if (!(ok = to_int(p, 0, 0xFFFFFFFFll, v))) break;
                dst.push_back((uint32_t)v);
            }
        } else if (key == "exclude") {
            for (const auto& p : split(val, ',')) {
                if (val.empty()) break;
                if (!(ok = to_int(p, i32lo, i32hi, v))) break;
                m.exclude.push_back((int32_t)v);
            }
        } else if (key.size() > 1 && key[0] == 'c' && to_int(key.substr(1), 0, 1 << 20, v)) {
            if (v >= n_cols) { why = "column outside the engine's list: " + key; return false; }
            auto& dst = m.cols[(size_t)v];
            for (const auto& p : split(val, ',')) {
                if (val.empty()) break;
                const size_t c = p.find(':');
                long long a = 0, b = 0;
                if (!(ok = c != std::string::npos && to_int(p.substr(0, c), i32lo, i32hi, a) && to_int(p.substr(c + 1), i32lo, i32hi, b))) break;
                dst.emplace_back((int32_t)a, (int32_t)b);
            }
        } else {
            why = "unknown key: " + key;
            return false;
        }
        if (!ok) { why = "bad value: " + w; return false; }
    }
    if (m.club_m >= 0 && m.club_topk == 0) { why = "m= without topclubs="; return false; }
    if (!diverse_words_ok(m.diverse, m.diverse_pool, m.collect, m.club_topk, m.club_m)) {
        why = "pool= without diverse=, or diverse= with all= / topclubs= / m=";
        return false;
    }
    return true;
}

}  // namespace pokec
