// facade_profile_check.cpp — test driver for the by-profile calls of the C++ facade
// (include/pokec/recommender.h: recommend_by_profile, profile_similarity_adhoc,
// profile_similarity_terms_adhoc).  Builds the reference-shaped maps from a data directory through
// pokec_io.h, wires a pokec::Recommender like api_cli.cpp:155-163, and checks, for every uid on
// stdin (one per line), with A a copy of the map's profile:
//   - recommend_by_profile(A, 20, adj[uid] + {uid}) == recommend_interest_all(uid, 20), ids and bits;
//   - profile_similarity_adhoc(A, B) has the bits of profile_similarity(A, B) for a spread of B,
//     with and without a field selection, and profile_similarity_terms_adhoc the same row;
//   - with A's user_id changed to one the map does not hold, profile_similarity gives NaN and
//     profile_similarity_adhoc the same finite bits as before.
// Prints "ok <n>" and exits 0, or the first mismatch and exits 1.
// Test infrastructure only (tests/test_gpu_query_profile.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
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
    if (argc < 2) { std::cerr << "usage: facade_profile_check <root>\n"; return 2; }
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
    pokec::FieldSelect sel;
    sel.fixed = PF_SEL_FIXED_ALL & ~(1u << PF_F_AGE);
    sel.cols = ~(1ull << 8);
    int n = 0, uid = 0;
    while (std::cin >> uid) {
        const pokec::UserProfile& X = profiles.at(uid);
        pokec::UserProfile A = X;  // by value
        std::vector<int> excl;
        auto it = adj.find(uid);
        if (it != adj.end()) excl = it->second;
        excl.push_back(uid);
        const auto want = rec.recommend_interest_all(uid, 20);
        const auto got = rec.recommend_by_profile(A, 20, excl);
        if (want.empty() || got.size() != want.size()) { std::printf("list size %d: %zu vs %zu\n", uid, got.size(), want.size()); return 1; }
        for (size_t i = 0; i < want.size(); ++i)
            if (got[i].first != want[i].first || hex(got[i].second) != hex(want[i].second)) {
                std::printf("list %d at %zu: %d %08x vs %d %08x\n", uid, i, got[i].first, hex(got[i].second), want[i].first, hex(want[i].second));
                return 1;
            }
        pokec::UserProfile S = X;  // the same profile under an id the map does not hold
        S.user_id = -12345;
        for (size_t j = (size_t)(uid % 7); j < order.size(); j += 97) {
            const pokec::UserProfile& B = profiles.at(order[j]);
            const float p0 = rec.profile_similarity(X, B), p1 = rec.profile_similarity_adhoc(A, B);
            const float s0 = rec.profile_similarity(X, B, sel), s1 = rec.profile_similarity_adhoc(A, B, sel);
            if (hex(p0) != hex(p1) || hex(s0) != hex(s1)) { std::printf("pair %d %d: %08x %08x / %08x %08x\n", uid, B.user_id, hex(p0), hex(p1), hex(s0), hex(s1)); return 1; }
            const float nan = rec.profile_similarity(S, B), fin = rec.profile_similarity_adhoc(S, B);
            if (!std::isnan(nan) || !std::isfinite(fin) || hex(fin) != hex(p0)) { std::printf("stranger %d %d: %08x %08x\n", uid, B.user_id, hex(nan), hex(fin)); return 1; }
            const pokec::ScoreTerms t0 = rec.profile_similarity_terms(X, B, sel), t1 = rec.profile_similarity_terms_adhoc(S, B, sel);
            if (hex(t0.score) != hex(t1.score) || t0.fixed != t1.fixed || t0.cols != t1.cols || t0.terms.size() != t1.terms.size() ||
                std::memcmp(t0.terms.data(), t1.terms.data(), t0.terms.size() * sizeof(double)) != 0) {
                std::printf("terms %d %d\n", uid, B.user_id);
                return 1;
            }
            ++n;
        }
    }
    if (!rec.last_error().empty()) { std::cerr << rec.last_error() << "\n"; return 1; }
    std::printf("ok %d\n", n);
    pf_dataset_free(ds);
    return 0;
}
