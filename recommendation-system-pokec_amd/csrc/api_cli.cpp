// api_cli.cpp — the reference's stdin/JSON front end (src/api_cli.cpp:86-258) over the
// MI355X engine.  Same files (cwd-relative data/ + config/), same stdout protocol:
// loader progress lines, READY, then one JSON line per input line.  The four
// recommenders run through the C ABI (pokec_fas.h); start-up uses pokec_io.h.
// One command is the engine's own: EXPLAIN <a> <b> prints the breakdown of FAS(a, b)
// (pf_fas_pairs_terms): {"a":A,"b":B,"score":S,"used":U,"possible":7+T,"terms":{name:term,...}},
// the present slots in slot order, doubles with max_digits10 digits (a JSON parse gives them back).
// Another is MATCH <topk> [key=value]... (csrc/match_line.h): the all-candidates top-k for a profile
// given on the line, for a person who is not a user of the corpus (pf_recommend_interest_profile).
// It answers {"recommendations":{"interest":[{"id":..,"score":..},..]}}, USER's list format, or
// {"error":"bad request","detail":..} / {"error":"engine failure","detail":..}.
// GROUP <topk> <mean|min|max> <uid> <uid> ... [noadj] [exclude=<uid,uid,...>] is the group query
// (pf_recommend_group): the users most similar to the listed seed users as a group; noadj also drops
// every seed's adj_list row.  It answers {"recommendations":{"group":[..]}} or the same two errors.
// MATCH and GROUP take topclubs=<topk> [m=<M>] (match_line.h): the reply's "recommendations" gain a
// "clubs" list with names, the clubs of the line's window scored by its neighbours
// (pf_recommend_clubs_profile / _group).  CLUBS <topk> <uid> [min=<float>] [m=<M>] [cap=<n>] is the same
// for a stored user (pf_recommend_clubs_interest): {"recommendations":{"clubs":[..]},"total":N,"used":U}
// and "overflow":true when the window holds more than cap (default 1048576) candidates.
// MATCH and GROUP also take diverse=<lambda> [pool=<M>] (match_line.h): the reply's list is then the
// diverse top-k of the line's window (pf_recommend_diverse_profile / _group), each item with its "pen",
// and the reply ends with "total":N,"pool":M; not together with all=, topclubs= or m=.  DIVERSE <topk> <uid> <lambda> [pool=<M>] [min=<float>]
// [cap=<n>] is the same for a stored user (pf_recommend_diverse_interest):
// {"recommendations":{"interest":[{"id":..,"score":..,"pen":..},..]},"total":N,"pool":M} and
// "overflow":true when the window holds more than cap (default 1048576) candidates.
//
//   pokec_api_cli [load_users] [--root DIR] [--device N] [--no-cap] [--cache PATH]
//
// load_users is parsed and ignored exactly like the reference (the loader's cap is
// fixed at 100000 lines, user_loader.cpp:34); --no-cap lifts it for full corpora.
// Differences: no vocabulary/adjacency ETL when tokens.csv / adjacency.csv are missing
// (out of scope): a missing adjacency.csv is an error, a missing
// tokens.csv only drops club names.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "match_line.h"
#include "pokec_io.h"

namespace {

// api_cli.cpp:28-47
std::string json_escape(const std::string& s) {
    std::string out;
    for (char c : s) {
        switch (c) {
            case '\\': out += "\\\\"; break;
            case '"': out += "\\\""; break;
            case '\b': out += "\\b"; break;
            case '\f': out += "\\f"; break;
            case '\n': out += "\\n"; break;
            case '\r': out += "\\r"; break;
            case '\t': out += "\\t"; break;
            default:
                if ((unsigned char)c < 0x20) {
                    char buf[8];
                    snprintf(buf, sizeof(buf), "\\u%04x", (int)c);
                    out += buf;
                } else {
                    out += c;
                }
        }
    }
    return out;
}

struct List {
    std::vector<int32_t> id;
    std::vector<float> score;
    int32_t n = 0;
    explicit List(int k) : id(k), score(k) {}
};

void write_list(std::ostringstream& os, const char* name, const List& l, const pf_dataset* clubs) {
    os << "\"" << name << "\":[";
    for (int i = 0; i < l.n; ++i) {
        if (i) os << ",";
        os << "{\"id\":" << l.id[i] << ",\"score\":" << std::fixed << std::setprecision(6) << l.score[i];
        if (clubs) {
            const char* nm = pf_dataset_club_name(clubs, l.id[i]);
            if (nm) os << ",\"name\":\"" << json_escape(nm) << "\"";
        }
        os << "}";
    }
    os << "]";
}

// a diverse list: write_list's items with the penalty each was picked at
void write_diverse_list(std::ostringstream& os, const char* name, const List& l, const std::vector<float>& pen) {
    os << "\"" << name << "\":[";
    for (int i = 0; i < l.n; ++i)
        os << (i ? "," : "") << "{\"id\":" << l.id[i] << ",\"score\":" << std::fixed << std::setprecision(6) << l.score[i] << ",\"pen\":"
           << pen[(size_t)i] << "}";
    os << "]";
}

// The diverse list of a MATCH / GROUP / DIVERSE line: call(q, topk, ids, scores, pen, n, info) is the
// engine call; the reply, or the engine-failure line.
template <class Call>
std::string diverse_reply(pf_ctx* ctx, const char* name, int topk, float lambda, int32_t pool, const pf_scan_window& win, int64_t cap,
                          Call call) {
    pf_scan_window w = win;
    w.fields &= ~PF_WIN_COUNT;  // the reply carries the total anyway
    pf_diverse_query q{};
    q.cap = cap;
    q.pool = pool > 0 ? pool : pokec::kDiversePoolDefault;
    q.lambda = lambda;
    q.window = w.fields ? &w : nullptr;
    List r(topk > 0 ? topk : 1);
    std::vector<float> pen((size_t)(topk > 0 ? topk : 1));
    pf_diverse_info di{};
    if (call(&q, (int32_t)topk, r.id.data(), r.score.data(), pen.data(), &r.n, &di) != PF_OK) {
        std::cerr << "[api_cli] engine: " << pf_last_error(ctx) << "\n";
        return "{\"error\":\"engine failure\",\"detail\":\"" + json_escape(pf_last_error(ctx)) + "\"}";
    }
    std::ostringstream os;
    os << "{\"recommendations\":{";
    write_diverse_list(os, name, r, pen);
    os << "},\"total\":" << di.total << ",\"pool\":" << di.pool << (di.total > q.cap ? ",\"overflow\":true" : "") << "}";
    return os.str();
}

// The score window of one MATCH / GROUP line (match_line.h: min=, after=, count): set for the span of
// the call, cleared on the way out.  A line without those words touches nothing and its reply is the
// line it always was; with one, tail() adds the last result's cursor and, under `count`, the total.
struct WindowScope {
    pf_ctx* ctx;
    pf_scan_window w;
    bool ok = true;
    WindowScope(pf_ctx* c, const pf_scan_window& win) : ctx(c), w(win) {
        if (w.fields) ok = pf_set_scan_window(ctx, &w) == PF_OK;
    }
    ~WindowScope() {
        if (w.fields) pf_set_scan_window(ctx, nullptr);
    }
    std::string tail(const List& r, int topk) const {
        if (!w.fields) return "";
        std::ostringstream os;
        if (r.n > 0) os << ",\"next\":\"" << pokec::window_cursor(r.score[(size_t)r.n - 1], r.id[(size_t)r.n - 1]) << "\"";
        else os << ",\"next\":null";
        if ((w.fields & PF_WIN_COUNT) && topk > 0) {  // (topk = 0 scans nothing and counts nothing)
            int64_t total = 0;
            int32_t n = 0;
            if (pf_scan_window_totals(ctx, &total, 1, &n) == PF_OK) os << ",\"total\":" << total;
        }
        return os.str();
    }
};

// The collector of one MATCH / GROUP line (match_line.h: all=<cap>): set for the span of the call,
// cleared on the way out.  whole() replaces the call's list by the whole window and gives the reply's
// tail: "total":N, and "overflow":true with an empty list when N > cap.
struct CollectScope {
    pf_ctx* ctx;
    int64_t cap;
    bool ok = true;
    CollectScope(pf_ctx* c, int64_t k) : ctx(c), cap(k) {
        if (cap > 0) ok = pf_set_scan_collect(ctx, cap) == PF_OK;
    }
    ~CollectScope() {
        if (cap > 0) pf_set_scan_collect(ctx, 0);
    }
    bool whole(List& r, std::string& tail) const {
        int64_t n = 0, total = 0;
        if (pf_scan_collected(ctx, nullptr, nullptr, 0, &n, &total) != PF_OK) return false;
        r.id.assign((size_t)n + 1, 0);
        r.score.assign((size_t)n + 1, 0.f);
        if (n > 0 && pf_scan_collected(ctx, r.id.data(), r.score.data(), n, &n, &total) != PF_OK) return false;
        r.n = (int32_t)n;
        tail = ",\"total\":" + std::to_string(total) + (total > cap ? ",\"overflow\":true" : "");
        return true;
    }
};

// The "clubs" list of a MATCH / GROUP line with topclubs=: the line's window (its count word plays no
// part), its all=<cap> as the cap when given
pf_clubs_query clubs_query(const pf_scan_window& win, int64_t collect, int32_t m) {
    pf_clubs_query q{};
    q.cap = collect > 0 ? collect : (int64_t)1 << 20;
    q.neighbours = m > 0 ? m : 0;
    q.window = win.fields ? &win : nullptr;
    return q;
}

}  // namespace

int main(int argc, char** argv) {
    std::ios::sync_with_stdio(true);
    std::cin.tie(nullptr);
    std::string root = ".";
    int device = 0;
    int64_t cap = PF_LOAD_REFERENCE_CAP;
    std::string cache;  // --cache PATH: binary cache of the CSV parse (F2), off by default
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--root" && i + 1 < argc) root = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
        else if (a == "--no-cap") cap = 0;
        else if (a == "--cache" && i + 1 < argc) cache = argv[++i];
        else {
            try { (void)std::stoi(a); } catch (...) {}  // load_users: no effect, as in the reference
        }
    }
    pf_dataset* ds = nullptr;
    if (pf_dataset_load_cached(root.c_str(), cap, cache.empty() ? nullptr : cache.c_str(), nullptr, &ds) != PF_OK) {
        std::cerr << "[api_cli] " << pf_last_error(nullptr) << "\n";
        return 1;
    }
    pf_dataset_info info{};
    pf_dataset_info_get(ds, &info);
    // load_users_encoded progress lines (user_loader.cpp:35-38,94)
    for (int64_t c = 0; c < info.lines_read; c += 10000) std::cout << "Loaded " << c << " users " << std::endl;
    std::cout << "Loaded " << info.n_profiles << " users total" << std::endl;
    std::cerr << "[api_cli] " << (info.vocab_loaded ? "vocab loaded from data" : "vocab not found (no club names)")
              << "\n[api_cli] adjacency loaded from data/adjacency.csv\n[api_cli] loaded profiles: "
              << info.n_profiles << "\n";
    const std::string median_path = root + "/data/median_age.txt";
    if (info.median_loaded) {
        std::cerr << "[api_cli] loaded median_age=" << info.median_age << " from " << median_path << "\n";
    } else if (info.median_age > 0) {
        std::ofstream out(median_path);  // save_median_age (user_loader.cpp:123-129)
        if (out.is_open()) out << info.median_age << "\n";
        std::cerr << "[api_cli] computed median_age=" << info.median_age << " and saved to " << median_path << "\n";
    } else {
        std::cerr << "[api_cli] computed median_age=0\n";
    }
    std::cerr << "[api_cli] replaced " << info.ages_replaced << " zero-ages with median_age=" << info.median_age
              << "\n";
    if (info.n_normalizers)
        std::cerr << "[api_cli] loaded column normalizers (" << info.n_normalizers << " entries)\n";
    else
        std::cerr << "[api_cli] column_normalizers.csv not found or invalid\n";

    pf_ctx* ctx = nullptr;
    if (pf_open(pf_dataset_desc(ds), device, &ctx) != PF_OK) {
        std::cerr << "[api_cli] engine: " << pf_last_error(nullptr) << "\n";
        pf_dataset_free(ds);
        return 1;
    }

    std::cout << "READY" << std::endl;
    std::cout.flush();
    constexpr int kTop = 20, kLimit = 5000;  // api_cli.cpp:213-234
    std::string line;
    std::vector<char> pj(1 << 16);
    while (std::getline(std::cin, line)) {
        if (line.empty()) {
            std::cout << "{}" << std::endl;
            continue;
        }
        std::string cmd;
        int uid = -1, xa = -1, xb = -1;
        {
            std::istringstream iss(line);
            iss >> cmd;
            if (cmd == "USER") iss >> uid;
            if (cmd == "EXPLAIN" && !(iss >> xa >> xb)) xa = xb = -1;
        }
        if (cmd == "PING") {
            std::cout << "{\"ok\":true}" << std::endl;
            continue;
        }
        if (cmd == "EXIT") {
            std::cout << "{\"ok\":true, \"exiting\":true}" << std::endl;
            break;
        }
        if (cmd == "USER" && uid >= 0) {
            int64_t len = 0;
            int rc = pf_dataset_profile_json(ds, uid, pj.data(), (int64_t)pj.size(), &len);
            if (rc == PF_ENOTFOUND) {
                std::cout << "{\"error\":\"not found\",\"user_id\":" << uid << "}" << std::endl;
                continue;
            }
            if (len + 1 > (int64_t)pj.size()) {
                pj.resize(len + 1);
                pf_dataset_profile_json(ds, uid, pj.data(), (int64_t)pj.size(), &len);
            }
            const int32_t q = uid;
            List g(kTop), c(kTop), cl(kTop);
            rc = pf_recommend_interest(ctx, &q, 1, kTop, PF_MODE_FOF, kLimit, g.id.data(), g.score.data(), &g.n);
            if (rc == PF_OK) rc = pf_recommend_collab(ctx, &q, 1, kTop, kLimit, c.id.data(), c.score.data(), &c.n);
            if (rc == PF_OK) rc = pf_recommend_clubs(ctx, &q, 1, kTop, kLimit, cl.id.data(), cl.score.data(), &cl.n);
            if (rc != PF_OK) {
                std::cerr << "[api_cli] engine: " << pf_last_error(ctx) << "\n";
                std::cout << "{\"error\":\"engine failure\",\"user_id\":" << uid << "}" << std::endl;
                continue;
            }
            std::ostringstream os;
            os << "{\"profile\":" << pj.data() << ",\"recommendations\":{";
            write_list(os, "graph", g, nullptr);
            os << ",";
            write_list(os, "collaborative", c, nullptr);
            os << ",";
            write_list(os, "interest", g, nullptr);  // recommend_by_interest == graph (recommender_graph.cpp:224-227)
            os << ",";
            write_list(os, "clubs", cl, ds);
            os << "}}";
            std::cout << os.str() << std::endl;
            continue;
        }
        if (cmd == "MATCH") {
            pokec::MatchLine m;
            std::string why;
            if (!pokec::parse_match_line(line.substr(line.find("MATCH") + 5), pf_num_cols(ctx), m, why)) {
                std::cout << "{\"error\":\"bad request\",\"detail\":\"" << json_escape(why) << "\"}" << std::endl;
                continue;
            }
            const pf_query_profile q = m.profile();
            if (m.diverse >= 0.f) {
                std::cout << diverse_reply(ctx, "interest", m.topk, m.diverse, m.diverse_pool, m.window, (int64_t)1 << 20,
                                           [&](const pf_diverse_query* dq, int32_t k, int32_t* ou, float* os_, float* op, int32_t* n, pf_diverse_info* di) {
                                               return pf_recommend_diverse_profile(ctx, &q, dq, k, ou, os_, op, nullptr, n, di);
                                           })
                          << std::endl;
                continue;
            }
            List r(m.topk > 0 ? m.topk : 1);
            const WindowScope ws(ctx, m.window);
            const CollectScope cs(ctx, m.collect);
            if (m.collect > 0 && m.topk < 1) m.topk = 1;  // (topk = 0 scans nothing; the list is the window anyway)
            std::string tail;
            if (!ws.ok || !cs.ok || pf_recommend_interest_profile(ctx, &q, 1, m.topk, r.id.data(), r.score.data(), &r.n) != PF_OK ||
                (m.collect > 0 && !cs.whole(r, tail))) {
                std::cerr << "[api_cli] engine: " << pf_last_error(ctx) << "\n";
                std::cout << "{\"error\":\"engine failure\",\"detail\":\"" << json_escape(pf_last_error(ctx)) << "\"}" << std::endl;
                continue;
            }
            List cl(m.club_topk > 0 ? m.club_topk : 1);
            if (m.club_topk > 0) {
                const pf_clubs_query cq = clubs_query(m.window, m.collect, m.club_m);
                if (pf_recommend_clubs_profile(ctx, &q, &cq, m.club_topk, cl.id.data(), cl.score.data(), &cl.n, nullptr) != PF_OK) {
                    std::cerr << "[api_cli] engine: " << pf_last_error(ctx) << "\n";
                    std::cout << "{\"error\":\"engine failure\",\"detail\":\"" << json_escape(pf_last_error(ctx)) << "\"}" << std::endl;
                    continue;
                }
            }
            std::ostringstream os;
            os << "{\"recommendations\":{";
            write_list(os, "interest", r, nullptr);
            if (m.club_topk > 0) {
                os << ",";
                write_list(os, "clubs", cl, ds);
            }
            os << "}" << (m.collect > 0 ? tail : ws.tail(r, m.topk)) << "}";
            std::cout << os.str() << std::endl;
            continue;
        }
        if (cmd == "GROUP") {
            // GROUP <topk> <mean|min|max> <uid> <uid> ... [noadj] [exclude=<uid,uid,...>] and the window's
            // words (match_line.h): [min=<float>] [after=<hex>:<uid>] [count] [all=<cap>]
            std::istringstream iss(line);
            std::string w, agg;
            int topk = -1;
            iss >> w >> topk >> agg;
            std::vector<int32_t> seeds, excl;
            pf_scan_window win{};
            int64_t collect = 0;
            int32_t club_topk = 0, club_m = -1, dpool = 0;
            float dlam = -1.f;
            uint32_t flags = 0;
            bool ok = !iss.fail() && topk >= 0 && (agg == "mean" || agg == "min" || agg == "max");
            auto number = [](const std::string& t, int32_t& v) {
                if (t.empty() || t.size() > 10) return false;
                for (char ch : t)
                    if (ch < '0' || ch > '9') return false;
                const long long x = atoll(t.c_str());
                v = (int32_t)x;
                return x <= 2147483647LL;
            };
            while (ok && iss >> w) {
                int32_t v = 0;
                const int ww = pokec::parse_window_word(w, win);
                const int cw = ww == 0 ? pokec::parse_collect_word(w, collect) : 0;
                const int kw = ww == 0 && cw == 0 ? pokec::parse_clubs_word(w, club_topk, club_m) : 0;
                const int dw = ww == 0 && cw == 0 && kw == 0 ? pokec::parse_diverse_word(w, dlam, dpool) : 0;
                if (dw != 0) {
                    ok = dw > 0;
                } else if (ww != 0) {
                    ok = ww > 0;
                } else if (cw != 0) {
                    ok = cw > 0;
                } else if (kw != 0) {
                    ok = kw > 0;
                } else if (w == "noadj") {
                    flags |= PF_GROUP_EXCLUDE_ADJ;
                } else if (w.rfind("exclude=", 0) == 0) {
                    std::istringstream es(w.substr(8));
                    std::string t;
                    while (ok && std::getline(es, t, ',')) {
                        ok = number(t, v);
                        excl.push_back(v);
                    }
                } else {
                    ok = number(w, v);
                    seeds.push_back(v);
                }
            }
            if (!ok || seeds.empty() || (club_m >= 0 && club_topk == 0) || !pokec::diverse_words_ok(dlam, dpool, collect, club_topk, club_m)) {
                std::cout << "{\"error\":\"bad request\",\"detail\":\"GROUP <topk> <mean|min|max> <uid>... [noadj] [exclude=<uid,...>] [min=<float>] [after=<hex>:<uid>] [count] [all=<cap>]"
                          << (club_topk > 0 || club_m >= 0 ? " [topclubs=<topk>] [m=<M>]" : "")
                          << (dlam >= 0.f || dpool > 0 ? " [diverse=<lambda>] [pool=<M>]" : "") << "\"}"
                          << std::endl;
                continue;
            }
            const pf_group_query q{seeds.data(), (int32_t)seeds.size(), agg == "mean" ? PF_GROUP_MEAN : (agg == "min" ? PF_GROUP_MIN : PF_GROUP_MAX),
                                   flags, excl.empty() ? nullptr : excl.data(), (int32_t)excl.size()};
            if (dlam >= 0.f) {
                std::cout << diverse_reply(ctx, "group", topk, dlam, dpool, win, (int64_t)1 << 20,
                                           [&](const pf_diverse_query* dq, int32_t k, int32_t* ou, float* os_, float* op, int32_t* n, pf_diverse_info* di) {
                                               return pf_recommend_diverse_group(ctx, &q, dq, k, ou, os_, op, nullptr, n, di);
                                           })
                          << std::endl;
                continue;
            }
            List r(topk > 0 ? topk : 1);
            const WindowScope ws(ctx, win);
            const CollectScope cs(ctx, collect);
            if (collect > 0 && topk < 1) topk = 1;  // (topk = 0 scans nothing; the list is the window anyway)
            std::string tail;
            if (!ws.ok || !cs.ok || pf_recommend_group(ctx, &q, 1, topk, r.id.data(), r.score.data(), &r.n) != PF_OK ||
                (collect > 0 && !cs.whole(r, tail))) {
                std::cerr << "[api_cli] engine: " << pf_last_error(ctx) << "\n";
                std::cout << "{\"error\":\"engine failure\",\"detail\":\"" << json_escape(pf_last_error(ctx)) << "\"}" << std::endl;
                continue;
            }
            List cl(club_topk > 0 ? club_topk : 1);
            if (club_topk > 0) {
                const pf_clubs_query cq = clubs_query(win, collect, club_m);
                if (pf_recommend_clubs_group(ctx, &q, &cq, club_topk, cl.id.data(), cl.score.data(), &cl.n, nullptr) != PF_OK) {
                    std::cerr << "[api_cli] engine: " << pf_last_error(ctx) << "\n";
                    std::cout << "{\"error\":\"engine failure\",\"detail\":\"" << json_escape(pf_last_error(ctx)) << "\"}" << std::endl;
                    continue;
                }
            }
            std::ostringstream os;
            os << "{\"recommendations\":{";
            write_list(os, "group", r, nullptr);
            if (club_topk > 0) {
                os << ",";
                write_list(os, "clubs", cl, ds);
            }
            os << "}" << (collect > 0 ? tail : ws.tail(r, topk)) << "}";
            std::cout << os.str() << std::endl;
            continue;
        }
        if (cmd == "CLUBS") {
            // CLUBS <topk> <uid> [min=<float>] [m=<M>] [cap=<n>]
            std::istringstream iss(line);
            std::string w;
            long long topk = -1, cu = -1, capv = (long long)1 << 20;
            iss >> w >> topk >> cu;
            pf_scan_window win{};
            int32_t unused_topk = 0, cm = -1;
            bool ok = !iss.fail() && topk >= 0 && topk <= (1 << 20) && cu >= 0 && cu <= 2147483647LL;
            while (ok && iss >> w) {
                if (w.rfind("min=", 0) == 0) ok = pokec::parse_window_word(w, win) > 0;
                else if (w.rfind("m=", 0) == 0) ok = pokec::parse_clubs_word(w, unused_topk, cm) > 0;
                else if (w.rfind("cap=", 0) == 0) ok = w.size() > 4 && w[4] != '+' && w[4] != '-' && pokec::match_detail::to_int(w.substr(4), 1, 2147483647LL, capv);
                else ok = false;
            }
            if (!ok) {
                std::cout << "{\"error\":\"bad request\",\"detail\":\"CLUBS <topk> <uid> [min=<float>] [m=<M>] [cap=<n>]\"}" << std::endl;
                continue;
            }
            pf_clubs_query cq{};
            cq.cap = (int64_t)capv;
            cq.neighbours = cm > 0 ? cm : 0;
            cq.window = win.fields ? &win : nullptr;
            List cl(topk > 0 ? (int)topk : 1);
            pf_clubs_info ci{};
            if (pf_recommend_clubs_interest(ctx, (int32_t)cu, &cq, (int32_t)topk, cl.id.data(), cl.score.data(), &cl.n, &ci) != PF_OK) {
                std::cerr << "[api_cli] engine: " << pf_last_error(ctx) << "\n";
                std::cout << "{\"error\":\"engine failure\",\"detail\":\"" << json_escape(pf_last_error(ctx)) << "\"}" << std::endl;
                continue;
            }
            std::ostringstream os;
            os << "{\"recommendations\":{";
            write_list(os, "clubs", cl, ds);
            os << "},\"total\":" << ci.total << ",\"used\":" << ci.used << (ci.total > cq.cap ? ",\"overflow\":true" : "") << "}";
            std::cout << os.str() << std::endl;
            continue;
        }
        if (cmd == "DIVERSE") {
            // DIVERSE <topk> <uid> <lambda> [pool=<M>] [min=<float>] [cap=<n>]
            std::istringstream iss(line);
            std::string w, lam;
            long long topk = -1, cu = -1, capv = (long long)1 << 20;
            iss >> w >> topk >> cu >> lam;
            pf_scan_window win{};
            float dlam = -1.f;
            int32_t dpool = 0;
            bool ok = !iss.fail() && topk >= 0 && topk <= (1 << 20) && cu >= 0 && cu <= 2147483647LL &&
                      pokec::parse_diverse_word("diverse=" + lam, dlam, dpool) > 0;
            while (ok && iss >> w) {
                if (w.rfind("min=", 0) == 0) ok = pokec::parse_window_word(w, win) > 0;
                else if (w.rfind("pool=", 0) == 0) ok = pokec::parse_diverse_word(w, dlam, dpool) > 0;
                else if (w.rfind("cap=", 0) == 0) ok = w.size() > 4 && w[4] != '+' && w[4] != '-' && pokec::match_detail::to_int(w.substr(4), 1, 2147483647LL, capv);
                else ok = false;
            }
            if (!ok) {
                std::cout << "{\"error\":\"bad request\",\"detail\":\"DIVERSE <topk> <uid> <lambda> [pool=<M>] [min=<float>] [cap=<n>]\"}" << std::endl;
                continue;
            }
            std::cout << diverse_reply(ctx, "interest", (int)topk, dlam, dpool, win, (int64_t)capv,
                                       [&](const pf_diverse_query* dq, int32_t k, int32_t* ou, float* os_, float* op, int32_t* n, pf_diverse_info* di) {
                                           return pf_recommend_diverse_interest(ctx, (int32_t)cu, dq, k, ou, os_, op, nullptr, n, di);
                                       })
                      << std::endl;
            continue;
        }
        if (cmd == "EXPLAIN" && xa >= 0 && xb >= 0) {
            static const char* const kFixedNames[PF_NUM_FIXED] = {"public", "gender", "completion", "age", "region", "clubs", "friends"};
            const int32_t a = xa, b = xb;
            const int W = PF_NUM_FIXED + pf_num_cols(ctx);
            pf_pair_terms_head h{};
            std::vector<double> row((size_t)W);
            if (pf_fas_pairs_terms(ctx, &a, &b, 1, nullptr, &h, row.data()) != PF_OK) {
                std::cerr << "[api_cli] engine: " << pf_last_error(ctx) << "\n";
                std::cout << "{\"error\":\"engine failure\",\"user_id\":" << xa << "}" << std::endl;
                continue;
            }
            if (h.score != h.score) {  // NaN: one of the two has no profile
                int64_t len = 0;
                const bool a_known = pf_dataset_profile_json(ds, xa, nullptr, 0, &len) != PF_ENOTFOUND;
                std::cout << "{\"error\":\"not found\",\"user_id\":" << (a_known ? xb : xa) << "}" << std::endl;
                continue;
            }
            std::ostringstream os;
            int used = 0;
            for (int s = 0; s < W; ++s)
                used += s < PF_NUM_FIXED ? (int)((h.fixed >> s) & 1u) : (int)((h.cols >> (s - PF_NUM_FIXED)) & 1ull);
            os << "{\"a\":" << xa << ",\"b\":" << xb << ",\"score\":" << std::setprecision(std::numeric_limits<float>::max_digits10)
               << h.score << ",\"used\":" << used << ",\"possible\":" << W << ",\"terms\":{"
               << std::setprecision(std::numeric_limits<double>::max_digits10);
            bool first = true;
            for (int s = 0; s < W; ++s) {
                const bool on = s < PF_NUM_FIXED ? ((h.fixed >> s) & 1u) != 0 : ((h.cols >> (s - PF_NUM_FIXED)) & 1ull) != 0;
                if (!on) continue;
                const char* nm = s < PF_NUM_FIXED ? kFixedNames[s] : pf_dataset_column(ds, s - PF_NUM_FIXED);
                os << (first ? "" : ",") << "\"" << json_escape(nm ? nm : "") << "\":" << row[(size_t)s];
                first = false;
            }
            os << "}}";
            std::cout << os.str() << std::endl;
            continue;
        }
        std::cout << "{\"error\":\"unknown command\"}" << std::endl;
    }
    pf_close(ctx);
    pf_dataset_free(ds);
    return 0;
}
