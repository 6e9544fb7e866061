// facade_group_check.cpp — test driver for the group calls of the C++ facade
// (include/pokec/recommender.h: recommend_for_group, group_similarity).  Builds the reference-shaped
// maps from a data directory through pokec_io.h and wires a pokec::Recommender like api_cli.cpp:155-163.
// Every stdin line is one group: <mean|min|max> <topk> <exclude_adj 0|1> <n_exclude> <exclude uids...>
// <seed uids...>.  For each it prints "list <id>:<score bits hex> ..." (recommend_for_group), then
// "fit <bits> ..." (group_similarity of the first three results), and checks itself that one seed with
// exclude_adj gives recommend_interest_all's list and that group_similarity of a profile outside the
// map is NaN.  Prints "ok <n>" last and exits 0, or the first mismatch and exits 1.
// Test infrastructure only (tests/test_gpu_group_front.py).
#include <cmath>
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

static unsigned hex(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::cerr << "usage: facade_group_check <root>\n"; return 2; }
    pf_dataset* ds = nullptr;
    if (pf_dataset_load(argv[1], PF_LOAD_REFERENCE_CAP, &ds) != PF_OK) { std::cerr << pf_last_error(nullptr) << "\n"; return 1; }
    const pf_corpus_desc* d = pf_dataset_desc(ds);
    const int T = d->n_cols;
    std::vector<std::string> cols;
    for (int t = 0; t < T; ++t) cols.push_back(pf_dataset_column(ds, t));
    std::unordered_map<int, pokec::UserProfile> profiles;
    std::vector<int> order;
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
        order.push_back(p.user_id);
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
    int n = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string agg;
        int topk = 0, ea = 0, nex = 0, x = 0;
        if (!(is >> agg >> topk >> ea >> nex)) continue;
        std::vector<int> excl, seeds;
        for (int i = 0; i < nex && (is >> x); ++i) excl.push_back(x);
        while (is >> x) seeds.push_back(x);
        const pokec::GroupAgg a = agg == "mean" ? pokec::GroupAgg::Mean : (agg == "min" ? pokec::GroupAgg::Min : pokec::GroupAgg::Max);
        const auto got = rec.recommend_for_group(seeds, topk, a, ea != 0, excl);
        std::printf("list");
        for (const auto& p : got) std::printf(" %d:%08x", p.first, hex(p.second));
        std::printf("\nfit");
        for (size_t i = 0; i < got.size() && i < 3; ++i)
            std::printf(" %08x", hex(rec.group_similarity(seeds, profiles.at(got[i].first), a)));
        std::printf("\n");
        // one seed, its adjacency row excluded: the by-uid all-candidates list
        const int u = seeds.front();
        if (profiles.count(u)) {
            const auto want = rec.recommend_interest_all(u, 20);
            const auto one = rec.recommend_for_group({u}, 20, a, true);
            if (want.empty() || one != want) { std::printf("one seed %d: %zu vs %zu entries\n", u, one.size(), want.size()); return 1; }
            pokec::UserProfile S = profiles.at(u);
            S.user_id = -12345;
            if (!std::isnan(rec.group_similarity(seeds, S, a))) { std::printf("a profile outside the map scored\n"); return 1; }
        }
        ++n;
    }
    if (!rec.recommend_for_group({order[0], order[1]}, 65).empty() || rec.last_error().find("topk") == std::string::npos) {
        std::printf("topk 65 was not refused: %s\n", rec.last_error().c_str());
        return 1;
    }
    std::printf("ok %d\n", n);
    pf_dataset_free(ds);
    return 0;
}
