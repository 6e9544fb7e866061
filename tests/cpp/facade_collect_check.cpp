// facade_collect_check.cpp — test driver for the collect methods of the C++ facade
// (include/pokec/recommender.h): collect_interest_all, collect_by_profile and collect_for_group against
// the C calls (pf_set_scan_collect + the scan call + pf_scan_collected) on the facade's own engine.
// Builds the reference-shaped maps from a data directory through pokec_io.h and wires a
// pokec::Recommender like api_cli.cpp:155-163.  Prints "ok <checks>" or the first difference.  Test
// infrastructure only (tests/test_gpu_scan_collect.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// the engine's last collected list, by the C call
static bool collected(pf_ctx* c, std::vector<int32_t>& ids, std::vector<float>& sc, int64_t& total) {
    int64_t n = 0;
    if (pf_scan_collected(c, nullptr, nullptr, 0, &n, &total) != PF_OK) return false;
    ids.assign((size_t)n, 0);
    sc.assign((size_t)n, 0.f);
    return n == 0 || pf_scan_collected(c, ids.data(), sc.data(), n, &n, &total) == PF_OK;
}

static bool ranked(const Ranked& r) {
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i - 1].second < r[i].second || (r[i - 1].second == r[i].second && r[i - 1].first >= r[i].first)) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::cerr << "usage: facade_collect_check <root>\n"; return 2; }
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
    const int u = d->user_id[441], v = d->user_id[1];
    const float floor = 0.125f;
    int checks = 0;
    std::vector<int32_t> ids;
    std::vector<float> sc;
    int64_t total = 0;

    // by uid: under a floor and with no window, against the C calls on the same engine
    Ranked a = rec.collect_interest_all(u, pokec::ScoreWindow::floor(floor), 4096);
    pf_ctx* c = rec.engine();
    if (!c) return bad("no engine");
    if (!collected(c, ids, sc, total) || !same(a, ids, sc) || total != (int64_t)a.size()) return bad("collect_interest_all vs pf_scan_collected");
    if (a.size() <= 64 || a.size() >= (size_t)d->n_users - 1 || !ranked(a) || a.back().second < floor) return bad("collect_interest_all under a floor");
    {
        pf_scan_window w{};
        w.fields = PF_WIN_MIN;
        w.min_score = floor;
        int32_t q = u, one = 0, n = 0;
        float s = 0.f;
        if (pf_set_scan_window(c, &w) != PF_OK || pf_set_scan_collect(c, 4096) != PF_OK ||
            pf_recommend_interest(c, &q, 1, 1, PF_MODE_ALL, 0, &one, &s, &n) != PF_OK || !collected(c, ids, sc, total))
            return bad("the C calls by uid");
        (void)pf_set_scan_collect(c, 0);
        (void)pf_set_scan_window(c, nullptr);
        if (!same(a, ids, sc) || n != 1 || one != a[0].first) return bad("collect_interest_all vs the C calls");
    }
    ++checks;
    Ranked everyone = rec.collect_interest_all(u);
    if (!collected(c, ids, sc, total) || !same(everyone, ids, sc) || everyone.size() <= a.size() || !ranked(everyone))
        return bad("collect_interest_all without a window");
    if (!std::equal(a.begin(), a.end(), everyone.begin())) return bad("the floored list is not the head of the whole one");
    ++checks;
    // overflow throws, and names the total
    try {
        (void)rec.collect_interest_all(u, pokec::ScoreWindow::floor(floor), 10);
        return bad("no exception on overflow");
    } catch (const std::length_error& e) {
        if (std::string(e.what()).find(std::to_string(a.size())) == std::string::npos) return bad("the exception does not name the total");
    }
    ++checks;
    // a cursor: the rest of the floored list after its 100th entry
    Ranked rest = rec.collect_interest_all(u, pokec::ScoreWindow::after(a[99].second, a[99].first).with_floor(floor), 4096);
    if (rest.size() != a.size() - 100 || !std::equal(rest.begin(), rest.end(), a.begin() + 100)) return bad("collect_interest_all under a cursor");
    ++checks;
    // by profile: u's own profile by value, excluding what the by-uid scan excludes
    std::vector<int> ex = adj.count(u) ? adj[u] : std::vector<int>();
    ex.push_back(u);
    Ranked b = rec.collect_by_profile(profiles[u], pokec::ScoreWindow::floor(floor), 4096, ex);
    if (!collected(c, ids, sc, total) || !same(b, ids, sc)) return bad("collect_by_profile vs pf_scan_collected");
    if (b != a) return bad("collect_by_profile vs collect_interest_all of the same user");
    ++checks;
    // a group: against pf_recommend_group with a collector
    const std::vector<int> seeds{u, v, d->user_id[600]};
    Ranked g = rec.collect_for_group(seeds, pokec::GroupAgg::Mean, pokec::ScoreWindow::floor(0.1f), 4096, true);
    if (!collected(c, ids, sc, total) || !same(g, ids, sc) || g.size() <= 64 || !ranked(g)) return bad("collect_for_group vs pf_scan_collected");
    {
        pf_scan_window w{};
        w.fields = PF_WIN_MIN;
        w.min_score = 0.1f;
        const std::vector<int32_t> sd(seeds.begin(), seeds.end());
        const pf_group_query q{sd.data(), (int32_t)sd.size(), (int32_t)pokec::GroupAgg::Mean, PF_GROUP_EXCLUDE_ADJ, nullptr, 0};
        int32_t one = 0, n = 0;
        float s = 0.f;
        if (pf_set_scan_window(c, &w) != PF_OK || pf_set_scan_collect(c, 4096) != PF_OK ||
            pf_recommend_group(c, &q, 1, 1, &one, &s, &n) != PF_OK || !collected(c, ids, sc, total))
            return bad("the C calls for a group");
        (void)pf_set_scan_collect(c, 0);
        (void)pf_set_scan_window(c, nullptr);
        if (!same(g, ids, sc)) return bad("collect_for_group vs the C calls");
    }
    for (auto& pr : g)
        if (pr.first == u || pr.first == v) return bad("a seed in its group's audience");
    ++checks;
    // the facade keeps no collector in force: a two-query call is not refused
    {
        int32_t q[2] = {u, v}, out[2], n[2];
        float s[2];
        if (pf_recommend_interest(c, q, 2, 1, PF_MODE_ALL, 0, out, s, n) != PF_OK) return bad("a collector stayed in force");
    }
    ++checks;
    if (!rec.last_error().empty()) { std::cerr << rec.last_error() << "\n"; return 1; }
    std::printf("ok %d\n", checks);
    pf_dataset_free(ds);
    return 0;
}
