// facade_diverse_check.cpp — test driver for the diverse top-k methods of the C++ facade
// (include/pokec/recommender.h): diversify, recommend_diverse_by_interest, recommend_diverse_by_profile and
// recommend_diverse_for_group.  Builds the reference-shaped maps from a data directory through pokec_io.h,
// wires a pokec::Recommender like api_cli.cpp:155-163 and prints one line per call, "<name> <id>:<the
// score's float bits as 8 hex digits> ...", which tests/test_gpu_diverse_front.py compares with the Python
// binding's results; "users", "info" and "overflow" lines beside them, then "ok".  Test infrastructure only.
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

static void show(const char* name, const Ranked& r) {
    std::printf("%s", name);
    for (const auto& p : r) {
        uint32_t b;
        std::memcpy(&b, &p.second, 4);
        std::printf(" %d:%08x", p.first, b);
    }
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { std::cerr << "usage: facade_diverse_check <root>\n"; return 2; }
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
    // u: the edge corpus's user 441 (edge_corpus.uid_of(441)); v: its user 1
    const int u = 4088, v = d->user_id[1];
    if (!profiles.count(u)) { std::printf("uid 4088 is not in the corpus\n"); return 1; }
    std::printf("users %d %d %d\n", u, v, d->user_id[600]);  // the users the lines below are about
    pf_diverse_info di{};
    show("interest", rec.recommend_diverse_by_interest(u, 12, 0.7f, 200, pokec::ScoreWindow(), 1 << 20, &di));
    std::printf("info %lld %lld %lld %lld\n", (long long)di.total, (long long)di.pool, (long long)di.pairs, (long long)di.picked);
    show("interest_floor", rec.recommend_diverse_by_interest(v, 10, 0.5f, 65, pokec::ScoreWindow::floor(0.125f)));
    std::vector<int> ex = adj.count(u) ? adj[u] : std::vector<int>();
    ex.push_back(u);
    show("profile", rec.recommend_diverse_by_profile(profiles[u], 12, 0.7f, 200, pokec::ScoreWindow(), 1 << 20, nullptr, ex));
    const std::vector<int> seeds{u, v, d->user_id[600]};
    show("group", rec.recommend_diverse_for_group(seeds, 9, 0.3f, 1024, pokec::ScoreWindow::floor(0.1f), 4096, &di, pokec::GroupAgg::Min, true));
    std::printf("info %lld %lld %lld %lld\n", (long long)di.total, (long long)di.pool, (long long)di.pairs, (long long)di.picked);
    const Ranked head = rec.recommend_interest_all(u, 64);
    show("diversify", rec.diversify(head, 10, 0.6f));
    try {
        (void)rec.recommend_diverse_by_interest(u, 10, 0.7f, 200, pokec::ScoreWindow::floor(0.125f), 10);
        std::printf("no exception on overflow\n");
        return 1;
    } catch (const std::length_error& e) {
        std::printf("overflow %s\n", e.what());
    }
    if (!rec.recommend_diverse_for_group({}, 5).empty() || !rec.recommend_diverse_by_interest(5, 5).empty() || !rec.diversify({}, 5, 0.5f).empty()) {
        std::printf("no seeds / an unknown user / an empty list\n");
        return 1;
    }
    if (!rec.recommend_diverse_by_interest(u, 5, 1.5f).empty() || rec.last_error().empty()) {
        std::printf("lambda 1.5 was served\n");
        return 1;
    }
    std::printf("ok\n");
    pf_dataset_free(ds);
    return 0;
}
