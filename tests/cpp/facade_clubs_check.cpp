// facade_clubs_check.cpp — test driver for the clubs-by-interest methods of the C++ facade
// (include/pokec/recommender.h): recommend_clubs_by_interest, recommend_clubs_by_profile and
// recommend_clubs_for_group against the definition computed on the host from the facade's collected
// rankings and the map's club lists (a double per club, added in rank order, cast to float), and against
// the C call on the facade's own engine.  Builds the reference-shaped maps from a data directory through
// pokec_io.h and wires a pokec::Recommender like api_cli.cpp:155-163.  Prints "ok <checks>" or the first
// difference.  Test infrastructure only (tests/test_gpu_club_front.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <map>
#include <set>
#include <iostream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "pokec/recommender.h"
#include "pokec_io.h"

using Ranked = pokec::Recommender::Ranked;

static int bad(const char* what) {
    std::printf("mismatch: %s\n", what);
    return 1;
}

static bool same(const Ranked& a, const std::vector<int32_t>& ids, const std::vector<float>& sc) {
    if (a.size() != ids.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].first != ids[i] || std::memcmp(&a[i].second, &sc[i], 4) != 0) return false;
    return true;
}

static bool ranked(const Ranked& r) {
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i - 1].second < r[i].second || (r[i - 1].second == r[i].second && r[i - 1].first >= r[i].first)) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::cerr << "usage: facade_clubs_check <root>\n"; return 2; }
    pf_dataset* ds = nullptr;
    if (pf_dataset_load(argv[1], PF_LOAD_REFERENCE_CAP, &ds) != PF_OK) { std::cerr << pf_last_error(nullptr) << "\n"; return 1; }
    const pf_corpus_desc* d = pf_dataset_desc(ds);
    const int T = d->n_cols;
    std::vector<std::string> cols;
    for (int t = 0; t < T; ++t) cols.push_back(pf_dataset_column(ds, t));
    std::unordered_map<int, pokec::UserProfile> profiles;
    for (int i = 0; i < d->n_users; ++i) {
        pokec::UserProfile p;
        p.user_id = d->user_id[i]; p.public_flag = d->public_flag[i]; p.completion_percentage = d->completion[i];
        p.gender = d->gender[i]; p.age = d->age[i];
        for (int k = 0; k < 3; ++k) p.region_parts[k] = d->region[3 * i + k];
        p.clubs.assign(d->club_ids + d->club_off[i], d->club_ids + d->club_off[i + 1]);
        p.friends.assign(d->friend_ids + d->friend_off[i], d->friend_ids + d->friend_off[i + 1]);
        p.token_cols.resize(T);
        for (int t = 0; t < T; ++t)
            for (int64_t k = d->tok_off[(int64_t)i * T + t]; k < d->tok_off[(int64_t)i * T + t + 1]; ++k)
                p.token_cols[t][d->tok_tid[k]] = d->tok_tf[k];
        profiles[p.user_id] = std::move(p);
    }
    pokec::AdjMap adj;
    for (int i = 0; i < d->n_adj; ++i) adj[d->adj_uid[i]].assign(d->adj_nbr + d->adj_off[i], d->adj_nbr + d->adj_off[i + 1]);
    pokec::NormMap norms;
    const char* keys[PF_NUM_FIXED] = {"public", "gender", "completion", "age", "region", "clubs", "friends"};
    for (int k = 0; k < PF_NUM_FIXED + T; ++k)
        if (d->norm_present[k]) norms[k < PF_NUM_FIXED ? keys[k] : cols[k - PF_NUM_FIXED]] = {d->norm_mean[k], d->norm_sd[k]};
    pokec::Recommender rec(&profiles, &adj);
    rec.set_field_normalizers(norms);
    rec.set_column_normalizers(norms);
    rec.compute_idf_from_profiles(cols);
    rec.set_text_columns(cols);
    if (d->n_users < 1000) return bad("the corpus is too small");
    // u: the edge corpus's user 441 (edge_corpus.uid_of(441)), one of its identical users: its clubs are its nearest neighbours'
    const int u = 4088, v = d->user_id[1];
    if (!profiles.count(u)) return bad("uid 4088 is not in the corpus");
    const float floor = 0.125f;
    int checks = 0;

    // the definition on the host: the facade's own collected ranking (checked against the oracle by the
    // collect tests) and the map's club lists, a double per club in rank order, cast to float
    auto host = [&](const Ranked& nb, size_t m, const std::set<unsigned>& own, size_t topk, pf_clubs_info* hi) {
        std::map<unsigned, double> acc;
        const size_t used = m && m < nb.size() ? m : nb.size();
        int64_t adds = 0;
        for (size_t i = 0; i < used; ++i) {
            const double w = (double)nb[i].second;
            if (w <= 0.0) continue;
            for (unsigned cl : profiles.at(nb[i].first).clubs) {
                if (own.count(cl)) continue;
                acc[cl] += w;
                ++adds;
            }
        }
        Ranked r;
        for (auto& kv : acc) r.emplace_back((int)kv.first, (float)kv.second);
        std::sort(r.begin(), r.end(), [](const std::pair<int, float>& a, const std::pair<int, float>& b) {
            return a.second == b.second ? a.first < b.first : a.second > b.second;
        });
        *hi = pf_clubs_info{(int64_t)nb.size(), (int64_t)used, adds, (int64_t)r.size()};
        if (r.size() > topk) r.resize(topk);
        return r;
    };
    auto same_info = [](const pf_clubs_info& a, const pf_clubs_info& b) {
        return a.total == b.total && a.used == b.used && a.contributions == b.contributions && a.clubs == b.clubs;
    };
    auto bits_equal = [](const Ranked& a, const Ranked& b) {
        if (a.size() != b.size()) return false;
        for (size_t i = 0; i < a.size(); ++i)
            if (a[i].first != b[i].first || std::memcmp(&a[i].second, &b[i].second, 4) != 0) return false;
        return true;
    };
    const std::set<unsigned> own_u(profiles.at(u).clubs.begin(), profiles.at(u).clubs.end());
    if (own_u.empty()) return bad("user 441 has no clubs");
    pf_clubs_info gi{}, hi{};

    // by uid: under a floor with M = 65, and the whole ranking
    const Ranked nb = rec.collect_interest_all(u, pokec::ScoreWindow::floor(floor), 4096);
    pf_ctx* c = rec.engine();
    if (!c) return bad("no engine");
    // (u's 65 nearest neighbours are its identical users: every club they hold is u's own, so that list is empty)
    Ranked none = rec.recommend_clubs_by_interest(u, 10, 65, pokec::ScoreWindow::floor(floor), 4096, false, &gi);
    if (!bits_equal(none, host(nb, 65, own_u, 10, &hi)) || !same_info(gi, hi) || gi.used != 65) return bad("recommend_clubs_by_interest, M = 65");
    Ranked a = rec.recommend_clubs_by_interest(u, 10, 0, pokec::ScoreWindow::floor(floor), 4096, false, &gi);
    if (!bits_equal(a, host(nb, 0, own_u, 10, &hi)) || !same_info(gi, hi) || a.empty() || !ranked(a)) return bad("recommend_clubs_by_interest under a floor");
    ++checks;
    const Ranked everyone = rec.collect_interest_all(u);
    Ranked all = rec.recommend_clubs_by_interest(u, 1 << 20, 0, pokec::ScoreWindow(), 1 << 20, false, &gi);
    if (!bits_equal(all, host(everyone, 0, own_u, 1 << 20, &hi)) || !same_info(gi, hi) || all.size() < 20) return bad("recommend_clubs_by_interest, everyone");
    for (auto& pr : all)
        if (own_u.count((unsigned)pr.first)) return bad("an own club in the list");
    ++checks;
    Ranked kept = rec.recommend_clubs_by_interest(u, 10, 0, pokec::ScoreWindow(), 1 << 20, true, &gi);
    if (!bits_equal(kept, host(everyone, 0, {}, 10, &hi)) || !same_info(gi, hi) || !own_u.count((unsigned)kept[0].first))
        return bad("keep_own: the own clubs do not lead the list");
    ++checks;
    // against the C call on the same engine
    {
        pf_scan_window w{};
        w.fields = PF_WIN_MIN;
        w.min_score = floor;
        const pf_clubs_query q{4096, 0, 0u, &w};
        std::vector<int32_t> ids(10);
        std::vector<float> sc(10);
        int32_t n = 0;
        pf_clubs_info ci{};
        if (pf_recommend_clubs_interest(c, u, &q, 10, ids.data(), sc.data(), &n, &ci) != PF_OK || !same(a, std::vector<int32_t>(ids.begin(), ids.begin() + n),
                                                                                                      std::vector<float>(sc.begin(), sc.begin() + n)))
            return bad("recommend_clubs_by_interest vs the C call");
    }
    ++checks;
    // overflow throws, and names the total
    try {
        (void)rec.recommend_clubs_by_interest(u, 10, 0, pokec::ScoreWindow::floor(floor), 10);
        return bad("no exception on overflow");
    } catch (const std::length_error& e) {
        if (std::string(e.what()).find(std::to_string(nb.size())) == std::string::npos) return bad("the exception does not name the total");
    }
    ++checks;
    // by profile: u's own profile by value, excluding what the by-uid scan excludes
    std::vector<int> ex = adj.count(u) ? adj[u] : std::vector<int>();
    ex.push_back(u);
    Ranked b = rec.recommend_clubs_by_profile(profiles[u], 10, 0, pokec::ScoreWindow::floor(floor), 4096, false, ex, &gi);
    if (!bits_equal(b, a)) return bad("recommend_clubs_by_profile vs recommend_clubs_by_interest of the same user");
    ++checks;
    // a group: the seeds' clubs are the own clubs
    const std::vector<int> seeds{u, v, d->user_id[600]};
    std::set<unsigned> own_g;
    for (int s : seeds) own_g.insert(profiles.at(s).clubs.begin(), profiles.at(s).clubs.end());
    const Ranked gnb = rec.collect_for_group(seeds, pokec::GroupAgg::Mean, pokec::ScoreWindow::floor(0.1f), 4096, true);
    Ranked g = rec.recommend_clubs_for_group(seeds, 12, pokec::GroupAgg::Mean, 0, pokec::ScoreWindow::floor(0.1f), 4096, false, true, {}, &gi);
    if (!bits_equal(g, host(gnb, 0, own_g, 12, &hi)) || !same_info(gi, hi) || g.empty()) return bad("recommend_clubs_for_group");
    ++checks;
    if (!rec.recommend_clubs_for_group({}, 5).empty() || !rec.recommend_clubs_by_interest(5, 5).empty()) return bad("no seeds / an unknown user");
    // the facade keeps nothing in force: a two-query call is not refused, and no window applies
    {
        int32_t q[2] = {u, v}, out[2], n[2];
        float s[2];
        if (pf_recommend_interest(c, q, 2, 1, PF_MODE_ALL, 0, out, s, n) != PF_OK || out[0] != everyone[0].first) return bad("state stayed in force");
    }
    ++checks;
    if (!rec.last_error().empty()) { std::cerr << rec.last_error() << "\n"; return 1; }
    std::printf("ok %d\n", checks);
    pf_dataset_free(ds);
    return 0;
}
