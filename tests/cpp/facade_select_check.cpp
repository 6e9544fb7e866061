// facade_select_check.cpp — test driver for the field-selection overloads of the C++ facade
// (include/pokec/recommender.h: recommend_interest_all(user, topk, FieldSelect[, CandidateFilter]),
// profile_similarity(A, B, FieldSelect) and profile_similarity(A, B, a prefix of the text columns)).
// Builds the reference-shaped maps from a data directory through pokec_io.h, wires a
// pokec::Recommender like api_cli.cpp:155-163, and answers stdin queries:
//   "all uid topk"                                    -> the unselected overload
//   "sel uid topk fixed cols"                         -> the selected one (fixed / cols in hex)
//   "selfilt uid topk fixed cols gender public amin amax cmin cmax r0 r1 r2 keep" -> with a filter
//       each as "tag uid topk n id:hex ..."
//   "simsel a b fixed cols"                           -> profile_similarity(A, B, FieldSelect) as "tag hex"
//   "simprefix a b n"                                 -> profile_similarity(A, B, the first n columns)
//   "engines"                                         -> "engines <engines in the facade's registry>"
// Test infrastructure only (tests/test_gpu_field_select.py).
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
    if (argc < 2) { std::cerr << "usage: facade_select_check <root>\n"; return 2; }
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
        iss >> tag;
        if (tag == "engines") {
            std::printf("engines %zu\n", pokec::detail::registry().engines.size());
            continue;
        }
        if (tag == "simsel" || tag == "simprefix") {
            int a = 0, b = 0;
            iss >> a >> b;
            float f;
            if (tag == "simsel") {
                pokec::FieldSelect s;
                iss >> std::hex >> s.fixed >> s.cols >> std::dec;
                f = rec.profile_similarity(profiles.at(a), profiles.at(b), s);
            } else {
                int n = 0;
                iss >> n;
                f = rec.profile_similarity(profiles.at(a), profiles.at(b), std::vector<std::string>(cols.begin(), cols.begin() + n));
            }
            std::printf("%s %08x\n", tag.c_str(), hex(f));
            continue;
        }
        int uid = 0, k = 0;
        iss >> uid >> k;
        pokec::Recommender::Ranked r;
        if (tag == "sel" || tag == "selfilt") {
            pokec::FieldSelect s;
            iss >> std::hex >> s.fixed >> s.cols >> std::dec;
            if (tag == "selfilt") {
                pokec::CandidateFilter f;
                int keep = 0;
                iss >> f.gender >> f.public_flag >> f.age_min >> f.age_max >> f.completion_min >> f.completion_max >>
                    f.region[0] >> f.region[1] >> f.region[2] >> keep;
                f.keep_missing = keep != 0;
                r = rec.recommend_interest_all(uid, k, s, f);
            } else {
                r = rec.recommend_interest_all(uid, k, s);
            }
        } else {
            r = rec.recommend_interest_all(uid, k);
        }
        std::printf("%s %d %d %zu", tag.c_str(), uid, k, r.size());
        for (auto& pr : r) std::printf(" %d:%08x", pr.first, hex(pr.second));
        std::printf("\n");
    }
    if (!rec.last_error().empty()) std::cerr << rec.last_error() << "\n";
    pf_dataset_free(ds);
    return rec.last_error().empty() ? 0 : 1;
}
