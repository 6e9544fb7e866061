// match_line.h — the api_cli's MATCH command line (csrc/api_cli.cpp): a profile given by value on one
// line, for a person who is not a user of the corpus (pokec_fas.h pf_query_profile).
//
//   MATCH <topk> [public=N] [gender=N] [completion=N] [age=N] [region=a,b,c] [clubs=id,id,..]
//         [friends=id,id,..] [exclude=uid,uid,..] [c<t>=tid:tf,tid:tf,..]...
//
// A field that is not given is missing; an empty region part ("region=3,,27") is missing; c<t> is
// text column t of the engine's list, as token ids (the text -> id ETL is not part of the engine).
// Engine-free, so the parser is tested without a GPU.
#pragma once
#include <cstdint>
#include <cstdlib>
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
    return true;
}

}  // namespace pokec
