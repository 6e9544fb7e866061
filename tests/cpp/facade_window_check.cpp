// facade_window_check.cpp — test driver for the ScoreWindow overloads of the C++ facade
// (include/pokec/recommender.h).  Builds the reference-shaped maps from a data directory through
// pokec_io.h, wires a pokec::Recommender like api_cli.cpp:155-163, and answers stdin queries:
//   "floor uid topk min"            recommend_interest_all under a counted floor
//   "pages uid k n"                 n pages of k of recommend_interest_all, chained by the cursor
//   "gpages k n seed seed ..."      the same of recommend_for_group (mean, exclude_adj)
//   "plain uid topk"                the overload without a window
// each as "total id:hex ..." (total -1 where nothing was counted).  Test infrastructure only
// (tests/test_gpu_window_front.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "pokec/recommender.h"
#include "pokec_io.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::cerr << "usage: facade_window_check <root>\n"; return 2; }
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
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream iss(line);
        std::string tag;
        iss >> tag;
        pokec::Recommender::Ranked r;
        int64_t total = -1;
        if (tag == "floor") {
            int uid = 0, k = 0;
            float mn = 0.f;
            iss >> uid >> k >> mn;
            r = rec.recommend_interest_all(uid, k, pokec::ScoreWindow::floor(mn).with_count(), &total);
        } else if (tag == "pages" || tag == "gpages") {
            int uid = 0, k = 0, n = 0;
            if (tag == "pages") iss >> uid;
            iss >> k >> n;
            std::vector<int> seeds;
            for (int s; iss >> s;) seeds.push_back(s);
            pokec::ScoreWindow w;  // page 1: no window words at all
            for (int p = 0; p < n; ++p) {
                pokec::Recommender::Ranked page;
                if (tag == "pages") page = p == 0 ? rec.recommend_interest_all(uid, k) : rec.recommend_interest_all(uid, k, w);
                else page = p == 0 ? rec.recommend_for_group(seeds, k, pokec::GroupAgg::Mean, true)
                                   : rec.recommend_for_group(seeds, k, pokec::GroupAgg::Mean, true, {}, w);
                if (page.empty()) break;
                w = pokec::ScoreWindow::after(page.back().second, page.back().first);
                r.insert(r.end(), page.begin(), page.end());
            }
        } else {
            int uid = 0, k = 0;
            iss >> uid >> k;
            r = rec.recommend_interest_all(uid, k);
        }
        std::printf("%lld", (long long)total);
        for (auto& pr : r) {
            unsigned u;
            std::memcpy(&u, &pr.second, 4);
            std::printf(" %d:%08x", pr.first, u);
        }
        std::printf("\n");
    }
    if (!rec.last_error().empty()) std::cerr << rec.last_error() << "\n";
    pf_dataset_free(ds);
    return rec.last_error().empty() ? 0 : 1;
}
