// facade_terms_check.cpp — test driver for the score breakdown of the C++ facade
// (include/pokec/recommender.h: profile_similarity_terms(A, B[, FieldSelect])).
// Builds the reference-shaped maps from a data directory through pokec_io.h, wires a
// pokec::Recommender like api_cli.cpp:155-163, and answers stdin queries:
//   "terms a b"             -> profile_similarity_terms(A, B)
//   "termsel a b fixed cols" -> the selected overload (fixed / cols in hex)
//       each as "tag score-hex sim-hex fixed-hex cols-hex n term-hex ..." (sim = profile_similarity
//       of the same arguments; terms as the doubles' 64 bits)
//   "stranger a"            -> a profile that is not of the map against a: "stranger score-hex fixed cols n"
// Test infrastructure only (tests/test_gpu_pair_terms.py).
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
    if (argc < 2) { std::cerr << "usage: facade_terms_check <root>\n"; return 2; }
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
    auto hex = [](float f) {
        unsigned u;
        std::memcpy(&u, &f, 4);
        return u;
    };
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream iss(line);
        std::string tag;
        int a = 0, b = 0;
        iss >> tag >> a;
        if (tag == "stranger") {
            pokec::UserProfile s;
            s.user_id = -12345;
            const pokec::ScoreTerms st = rec.profile_similarity_terms(s, profiles.at(a));
            std::printf("stranger %08x %x %llx %zu\n", hex(st.score), st.fixed, (unsigned long long)st.cols, st.terms.size());
            continue;
        }
        iss >> b;
        pokec::ScoreTerms st;
        float sim;
        if (tag == "termsel") {
            pokec::FieldSelect s;
            iss >> std::hex >> s.fixed >> s.cols >> std::dec;
            st = rec.profile_similarity_terms(profiles.at(a), profiles.at(b), s);
            sim = rec.profile_similarity(profiles.at(a), profiles.at(b), s);
        } else {
            st = rec.profile_similarity_terms(profiles.at(a), profiles.at(b));
            sim = rec.profile_similarity(profiles.at(a), profiles.at(b));
        }
        std::printf("%s %08x %08x %x %llx %zu", tag.c_str(), hex(st.score), hex(sim), st.fixed, (unsigned long long)st.cols,
                    st.terms.size());
        for (double t : st.terms) {
            unsigned long long u;
            std::memcpy(&u, &t, 8);
            std::printf(" %016llx", u);
        }
        std::printf("\n");
    }
    if (!rec.last_error().empty()) std::cerr << rec.last_error() << "\n";
    pf_dataset_free(ds);
    return rec.last_error().empty() ? 0 : 1;
}
