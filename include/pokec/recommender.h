// pokec/recommender.h — C++ drop-in for the reference's `Recommender` class
// (include/recommender.h:17-71) over the MI355X engine's C ABI (pokec_fas.h).
//
// Same construction (non-owning pointers to the profiles map and adj_list), same
// setters, same public data members, same recommender signatures and results
// (bit-identical scores, same order); the scoring runs on the GPU.  Header-only; link
// libpokec_fas.so.
//
// The class is a template over the profile type, pokec::BasicRecommender<Profile>; any
// struct with the reference's UserProfile fields (include/user_profile.h:10-20) works.
//   - pokec::Recommender = BasicRecommender<pokec::UserProfile> (this header's twin struct);
//   - drop-in mode: a translation unit that includes the reference's user_profile.h and
//     defines POKEC_DROP_IN before this header gets ::Recommender =
//     BasicRecommender<::UserProfile>, so the reference's own call sites (api_cli.cpp:155-234,
//     test.cpp:35-75, recommendation_tests.cpp:111-140) compile and behave unchanged.
//
// How it keeps the reference's behaviour:
//   - adj_list is read live, as the reference reads *adj_list: before every recommender call
//     the rows that call reads (the user's row and its friends' rows, recommender_graph.cpp:
//     10-31,114-125, recommender_clubs.cpp:47-58) are compared with the engine's copy and the
//     changed ones are pushed with pf_set_adj.  That is O(sum of those rows), the order of the
//     reference's own walk, so a caller that mutates its adj_mod between calls (test.cpp:73) or
//     builds a fresh Recommender over a fresh adj_mod per user (recommendation_tests.cpp:111-116)
//     needs no extra call.
//   - One engine context (a full HBM replica, pf_open) is shared by every Recommender over the
//     same profiles map, device, text columns, normalisers and idf values, whatever adjacency
//     map each one reads: constructing a Recommender costs a lookup, not a pf_open.  Engines stay
//     open for reuse (at most kMaxEngines idle ones) until release_engines().
//   - compute_idf_from_profiles fills the public idf_per_col on the host with the reference's
//     float32 logf (recommender.cpp:43-66), so callers that copy it (test.cpp:40,
//     recommendation_tests.cpp:120: set_tfidf_index(base_rec.idf_per_col)) see the reference's
//     map; an explicit map equal to the computed one shares the computed engine.
//   - The recommenders are const and may be called from several threads at once on one object
//     or on objects sharing an engine: the engine's calls are serialised by its mutex, and the
//     lazy open is guarded.
//
// Differences a caller must know:
//   - The profiles map (and the normalisers and idf values) are snapshotted when an engine is
//     opened for them; the reference reads *profiles live, but none of its callers mutates the
//     profiles after construction.
//   - profile_similarity(A, B[, text_columns]) scores two profiles OF THE MAP (by user_id), which
//     is how every reference caller uses it.  It returns NaN otherwise.  A text_columns list other
//     than set_text_columns' uses the engine for that list; a proper prefix of set_text_columns'
//     list is scored on the one engine through a field selection (no second engine is opened).
//     A profile that is NOT of the map (a visitor, an edited copy) is scored by value through
//     profile_similarity_adhoc(A, B) / profile_similarity_terms_adhoc(A, B), with B of the map, and
//     ranked against every profile of the map by recommend_by_profile(A, topk, exclude): the
//     reference's profile_similarity(A, B) for a corpus that also held A, under this engine's idf
//     and normalisers (pokec_fas.h "Query by profile").
//   - The legacy user_feats constructor and recommend_from_supernodes
//     (recommender_clubs.cpp:75-...) are not provided: no live caller uses them
//     (SURVEY.md §8 A12).
//   - No exceptions cross it either: an engine failure yields an empty result,
//     and last_error() says why.
#ifndef POKEC_RECOMMENDER_H
#define POKEC_RECOMMENDER_H

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <list>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "pokec_fas.h"

namespace pokec {

// include/user_profile.h:10-20
struct UserProfile {
    int user_id = -1;
    int public_flag = -1;
    int completion_percentage = -1;
    int gender = -1;
    int age = 0;
    std::vector<uint32_t> clubs;
    std::vector<uint32_t> friends;
    std::vector<std::unordered_map<int, int>> token_cols;
    std::array<int, 3> region_parts = {-1, -1, -1};
};

using NormMap = std::unordered_map<std::string, std::pair<float, float>>;
using IdfMap = std::unordered_map<std::string, std::unordered_map<int, float>>;
using AdjMap = std::unordered_map<int, std::vector<int>>;

// Which candidates recommend_interest_all ranks (pokec_fas.h pf_cand_filter): every member set is
// one test, all of them must pass.  gender / public_flag: the value to equal (< 0: not tested);
// age / completion: an inclusive range (max < min: not tested; ages as the profiles hold them);
// region: each part >= 0 must equal the candidate's part, -1 = any.  A candidate whose tested field
// is missing (value < 0, age / completion <= 0) fails unless keep_missing.
struct CandidateFilter {
    int gender = -1;
    int public_flag = -1;
    int age_min = 1, age_max = 0;
    int completion_min = 1, completion_max = 0;
    std::array<int, 3> region = {-1, -1, -1};
    bool keep_missing = false;

    pf_cand_filter c_form() const {
        pf_cand_filter f{};
        if (gender >= 0) { f.fields |= PF_FILT_GENDER; f.gender = gender; }
        if (public_flag >= 0) { f.fields |= PF_FILT_PUBLIC; f.public_flag = public_flag; }
        if (age_max >= age_min) { f.fields |= PF_FILT_AGE; f.age_min = age_min; f.age_max = age_max; }
        if (completion_max >= completion_min) {
            f.fields |= PF_FILT_COMPLETION;
            f.completion_min = completion_min;
            f.completion_max = completion_max;
        }
        for (int i = 0; i < 3; ++i) f.region[i] = region[(size_t)i] >= 0 ? region[(size_t)i] : -1;
        if (region[0] >= 0 || region[1] >= 0 || region[2] >= 0) f.fields |= PF_FILT_REGION;
        if (keep_missing) f.flags |= PF_FILT_KEEP_MISSING;
        return f;
    }
};

// Which fields FAS is computed over (pokec_fas.h pf_field_select): `fixed` bit k = PF_F_* (public,
// gender, completion, age, region, clubs, friends), `cols` bit t = column t of set_text_columns'
// list (bits past the list are ignored).  A deselected fixed field counts as missing on the user's
// side; the denominator is 7 + (selected columns), the reference's own for that column list, so
// scores under different selections are not comparable with each other.
struct FieldSelect {
    uint32_t fixed = PF_SEL_FIXED_ALL;
    uint64_t cols = ~0ull;

    pf_field_select c_form() const {
        pf_field_select s{};
        s.fixed = fixed;
        s.cols = cols;
        return s;
    }
};

// Which part of the ranked order an all-candidates call returns (pokec_fas.h pf_scan_window): a
// floor (results score >= min_score), a paging cursor (results rank strictly after (after_score,
// after_uid): pass a page's last result to get the next page) and, with `count`, the number of
// candidates in the window, returned through the call's `total` argument.  Under a window topk is
// at most 64: the cursor is the way deeper.
struct ScoreWindow {
    bool has_min = false, has_after = false, count = false;
    float min_score = 0.f, after_score = 0.f;
    int after_uid = 0;

    static ScoreWindow floor(float s) { ScoreWindow w; w.has_min = true; w.min_score = s; return w; }
    static ScoreWindow after(float score, int uid) {
        ScoreWindow w;
        w.has_after = true;
        w.after_score = score;
        w.after_uid = uid;
        return w;
    }
    ScoreWindow with_floor(float s) const { ScoreWindow w = *this; w.has_min = true; w.min_score = s; return w; }
    ScoreWindow with_count() const { ScoreWindow w = *this; w.count = true; return w; }

    pf_scan_window c_form() const {
        pf_scan_window w{};
        if (has_min) { w.fields |= PF_WIN_MIN; w.min_score = min_score; }
        if (has_after) { w.fields |= PF_WIN_AFTER; w.after_score = after_score; w.after_uid = after_uid; }
        if (count) w.fields |= PF_WIN_COUNT;
        return w;
    }
};

// The breakdown of a pair's FAS (pokec_fas.h pf_fas_pairs_terms): the per-field sigmoid terms the
// reference adds to sum_Si.  terms has 7 + (set_text_columns' list) doubles, slot k < 7 the fixed
// field PF_F_*, slot 7 + t column t; a slot is present where its mask bit is set (`fixed` bit k,
// `cols` bit t) and holds 0.0 otherwise.  score is profile_similarity's float.  For a profile that
// is not of the map the score is NaN, the masks are 0 and terms is empty.
struct ScoreTerms {
    float score = NAN;
    uint32_t fixed = 0;
    uint64_t cols = 0;
    std::vector<double> terms;
};

namespace detail {

// One engine context and the adjacency rows it currently holds.
struct Engine {
    pf_ctx* ctx = nullptr;
    std::mutex mu;  // pokec_fas.h: calls on one context are serialised
    AdjMap rows;    // the engine's adj_list (the open-time rows plus every pf_set_adj since)
    pf_cand_filter scan_filter{};  // the scan filter in force between calls (fields == 0: none)
    pf_field_select scan_select{};  // the scan selection in force between calls, when has_scan_select
    bool has_scan_select = false;
    int64_t n_users = 0, n_club_entries = 0;
    Engine() = default;
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    ~Engine() {
        if (ctx) pf_close(ctx);
    }
};

// What an engine was opened for; idf = the values it scores with, compared by content.
struct EngineKey {
    const void* profiles = nullptr;
    size_t n_profiles = 0;
    uint64_t fingerprint = 0;  // a content sample of the map (a recycled address is not reused blindly)
    int device = 0;
    std::vector<std::string> cols;
    NormMap field, column;
    std::shared_ptr<const IdfMap> idf;
    bool same(const EngineKey& o) const {
        return profiles == o.profiles && n_profiles == o.n_profiles && fingerprint == o.fingerprint &&
               device == o.device && cols == o.cols &&
               field == o.field && column == o.column && (idf == o.idf || *idf == *o.idf);
    }
};

// FNV-1a over the first (up to) 64 profiles in the map's iteration order: ids, scalar fields and
// list sizes. O(64) per engine lookup; tells a profiles map destroyed and re-created at the same
// address with the same size from the one the engine was opened for.
template <class Map>
uint64_t profiles_fingerprint(const Map& m) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](int64_t v) {
        for (int i = 0; i < 8; ++i) { h ^= (uint64_t)(v >> (8 * i)) & 0xFFu; h *= 1099511628211ull; }
    };
    int n = 0;
    for (auto it = m.begin(); it != m.end() && n < 64; ++it, ++n) {
        const auto& p = it->second;
        mix(it->first); mix(p.public_flag); mix(p.completion_percentage); mix(p.gender); mix(p.age);
        mix((int64_t)p.clubs.size()); mix((int64_t)p.friends.size()); mix((int64_t)p.token_cols.size());
        for (const auto& c : p.token_cols) mix((int64_t)c.size());
    }
    return h;
}

struct Registry {
    std::mutex mu;
    std::list<std::pair<EngineKey, std::shared_ptr<Engine>>> engines;  // most recent first
};
// never destroyed: engines still registered at exit are not closed during static destruction
// (the HIP runtime may be gone by then); the OS reclaims them
inline Registry& registry() {
    static Registry* r = new Registry();
    return *r;
}

}  // namespace detail

// Engines no Recommender holds are kept for reuse, at most this many.
constexpr int kMaxEngines = 4;

// Closes every engine no Recommender holds (their HBM replicas are freed).
inline void release_engines() {
    auto& R = detail::registry();
    std::lock_guard<std::mutex> g(R.mu);
    R.engines.remove_if([](const std::pair<detail::EngineKey, std::shared_ptr<detail::Engine>>& e) {
        return e.second.use_count() == 1;
    });
}

// How a group query combines a candidate's scores against the seeds (pokec_fas.h PF_GROUP_*)
enum class GroupAgg { Mean = PF_GROUP_MEAN, Min = PF_GROUP_MIN, Max = PF_GROUP_MAX };

template <class Profile>
class BasicRecommender {
public:
    using Ranked = std::vector<std::pair<int, float>>;
    using NormMap = pokec::NormMap;
    using IdfMap = pokec::IdfMap;

    BasicRecommender(const std::unordered_map<int, Profile>* profiles_in, const AdjMap* al, int device = 0)
        : profiles(profiles_in), adj_list(al), device_(device) {
        total_users = profiles ? profiles->size() : 0;
    }
    BasicRecommender(const BasicRecommender&) = delete;
    BasicRecommender& operator=(const BasicRecommender&) = delete;

    // recommender.cpp:27-41
    void set_field_normalizers(const NormMap& m) { field_normalizers = m; reset_(); }
    void set_column_normalizers(const NormMap& m) { column_normalizers = m; reset_(); }
    void set_text_columns(const std::vector<std::string>& cols) { text_columns_internal_ = cols; reset_(); }
    void set_tfidf_index(const IdfMap& idf_map) {
        idf_per_col = idf_map;
        idf_computed_ = false;
        reset_();
    }
    // recommender.cpp:43-66: df per column over the profiles, idf = logf(1 + N / (1 + df)) in
    // float32, N = |profiles|; the map the reference's callers copy (test.cpp:40)
    void compute_idf_from_profiles(const std::vector<std::string>& text_columns) {
        idf_per_col.clear();
        total_users = profiles ? profiles->size() : 0;
        if (profiles) compute_idf_(text_columns, idf_per_col);
        idf_cols_ = text_columns;
        idf_computed_ = true;
        reset_();
    }

    // recommender_graph.cpp:33-103,224-227
    Ranked recommend_graph_registration(int user, int topk, int candidate_limit = 10000) const {
        return run_(0, user, topk, candidate_limit);
    }
    Ranked recommend_by_interest(int user, int topk, int candidate_limit = 10000) const {
        return run_(0, user, topk, candidate_limit);
    }
    // recommender_graph.cpp:105-222
    Ranked recommend_collaborative(int user, int topk, int candidate_limit = 10000) const {
        return run_(1, user, topk, candidate_limit);
    }
    // recommender_clubs.cpp:10-73 (ids are club ids)
    Ranked recommend_clubs_collab(int user, int topk, int candidate_limit = 10000) const {
        return run_(2, user, topk, candidate_limit);
    }
    // recommender_graph.cpp:229-237
    Ranked recommend_friends_graph(int user, int topk, int candidate_limit = 10000) const {
        return recommend_graph_registration(user, topk, candidate_limit);
    }
    Ranked recommend_friends_collab(int user, int topk, int candidate_limit = 10000) const {
        return recommend_collaborative(user, topk, candidate_limit);
    }
    Ranked recommend_friends_by_interest(int user, int topk, int candidate_limit = 10000) const {
        return recommend_by_interest(user, topk, candidate_limit);
    }
    // Build-defined all-candidates interest scan: every profile but the
    // user and its adj_list row, one GPU pass.
    Ranked recommend_interest_all(int user, int topk) const { return run_(3, user, topk, 0); }
    // The same over the candidates that pass `filter` only (on top of the user's own exclusions);
    // the engine's filter is set for this call and put back afterwards, under the engine's lock.
    Ranked recommend_interest_all(int user, int topk, const CandidateFilter& filter) const {
        const pf_cand_filter f = filter.c_form();
        return run_(3, user, topk, 0, &f);
    }
    // The same scored over the selected fields only ("similar in what respect"); the engine's
    // selection (and filter) are set for this call and put back afterwards, under the engine's lock.
    Ranked recommend_interest_all(int user, int topk, const FieldSelect& select) const {
        const pf_field_select s = select.c_form();
        return run_(3, user, topk, 0, nullptr, &s);
    }
    Ranked recommend_interest_all(int user, int topk, const FieldSelect& select, const CandidateFilter& filter) const {
        const pf_cand_filter f = filter.c_form();
        const pf_field_select s = select.c_form();
        return run_(3, user, topk, 0, &f, &s);
    }

    // The same inside a score window (a floor, a paging cursor, a count): the engine's window is set
    // for this call and cleared afterwards, under the engine's lock.  total (optional) receives the
    // number of candidates in the window when window.count is set.  The cursor of page n + 1 is page
    // n's last result; a page shorter than topk ends the ranking.
    Ranked recommend_interest_all(int user, int topk, const ScoreWindow& window, int64_t* total = nullptr) const {
        const pf_scan_window w = window.c_form();
        return run_(3, user, topk, 0, nullptr, nullptr, &w, total);
    }
    Ranked recommend_interest_all(int user, int topk, const ScoreWindow& window, const CandidateFilter& filter,
                                  int64_t* total = nullptr) const {
        const pf_cand_filter f = filter.c_form();
        const pf_scan_window w = window.c_form();
        return run_(3, user, topk, 0, &f, nullptr, &w, total);
    }

    // recommender_similarity.cpp:10-124,126-128, for two profiles of the map
    float profile_similarity(const Profile& A, const Profile& B) const {
        return pair_(engine_(), A.user_id, B.user_id);
    }
    // recommender_similarity.cpp:10-124 over a caller-given column list (include/recommender.h:41):
    // its names pick the normalisers and idf maps, its length the columns compared and F's
    // denominator.
    // A proper prefix of set_text_columns' list (the only other list whose position t reads
    // token_cols[t] of the same column) is a selection of the first columns on the one engine.
    float profile_similarity(const Profile& A, const Profile& B, const std::vector<std::string>& text_columns) const {
        if (text_columns == text_columns_internal_) return profile_similarity(A, B);
        if (text_columns.size() < text_columns_internal_.size() && text_columns_internal_.size() <= 64 &&
            std::equal(text_columns.begin(), text_columns.end(), text_columns_internal_.begin())) {
            FieldSelect s;
            s.cols = ((uint64_t)1 << text_columns.size()) - 1;  // (size < 64 here)
            return profile_similarity(A, B, s);
        }
        return pair_(open_for_(text_columns), A.user_id, B.user_id);
    }
    // FAS over the selected fields only, for two profiles of the map (pf_fas_pairs_select)
    float profile_similarity(const Profile& A, const Profile& B, const FieldSelect& select) const {
        const pf_field_select s = select.c_form();
        return pair_(engine_(), A.user_id, B.user_id, &s);
    }

    // profile_similarity(A, B) with its per-field terms, for two profiles of the map; the overload
    // over the selected fields only (a deselected slot is not present)
    ScoreTerms profile_similarity_terms(const Profile& A, const Profile& B) const {
        return pair_terms_(engine_(), A.user_id, B.user_id, nullptr);
    }
    ScoreTerms profile_similarity_terms(const Profile& A, const Profile& B, const FieldSelect& select) const {
        const pf_field_select s = select.c_form();
        return pair_terms_(engine_(), A.user_id, B.user_id, &s);
    }

    // Query by profile (pokec_fas.h pf_query_profile): A is taken by value and need not be of the
    // map; its user_id plays no part.  The all-candidates top-k over every profile of the map but
    // those in `exclude` (nothing is excluded implicitly: pass A's own id and friends to leave them out).
    Ranked recommend_by_profile(const Profile& A, int topk, const std::vector<int>& exclude = {}) const {
        return by_profile_(A, topk, exclude, nullptr, nullptr);
    }
    // ... inside a score window (ScoreWindow: the cursor takes a profile query past result 64)
    Ranked recommend_by_profile(const Profile& A, int topk, const std::vector<int>& exclude, const ScoreWindow& window,
                                int64_t* total = nullptr) const {
        const pf_scan_window w = window.c_form();
        return by_profile_(A, topk, exclude, &w, total);
    }
    // profile_similarity(A, B) with A by value and B of the map (NaN when B is not); the overload over
    // the selected fields only
    float profile_similarity_adhoc(const Profile& A, const Profile& B) const { return adhoc_(A, B.user_id, nullptr); }
    float profile_similarity_adhoc(const Profile& A, const Profile& B, const FieldSelect& select) const {
        const pf_field_select s = select.c_form();
        return adhoc_(A, B.user_id, &s);
    }
    ScoreTerms profile_similarity_terms_adhoc(const Profile& A, const Profile& B) const {
        return adhoc_terms_(A, B.user_id, nullptr);
    }
    ScoreTerms profile_similarity_terms_adhoc(const Profile& A, const Profile& B, const FieldSelect& select) const {
        const pf_field_select s = select.c_form();
        return adhoc_terms_(A, B.user_id, &s);
    }

    // Group query (pokec_fas.h pf_group_query): the top-k profiles of the map most similar to the
    // seed users as a group, by the mean, the minimum ("similar to every seed") or the maximum
    // ("similar to any seed") of the per-seed scores.  Seeds not of the map are dropped; the seeds
    // and `exclude` are never returned; exclude_adj also drops every seed's adj_list row, as the
    // caller's adj_list holds it now.  topk above 64 is refused (an empty list, last_error says why).
    Ranked recommend_for_group(const std::vector<int>& seeds, int topk, GroupAgg agg = GroupAgg::Mean,
                               bool exclude_adj = false, const std::vector<int>& exclude = {}) const {
        return for_group_(seeds, topk, agg, exclude_adj, exclude, nullptr, nullptr);
    }
    // ... inside a score window (ScoreWindow: the cursor takes a group query past result 64)
    Ranked recommend_for_group(const std::vector<int>& seeds, int topk, GroupAgg agg, bool exclude_adj,
                               const std::vector<int>& exclude, const ScoreWindow& window, int64_t* total = nullptr) const {
        const pf_scan_window w = window.c_form();
        return for_group_(seeds, topk, agg, exclude_adj, exclude, &w, total);
    }
    // Collect (pokec_fas.h "Collect"): EVERY candidate of the window, ranked (score desc, uid asc), in
    // one scan and one device sort: everyone at least this similar to a user, to a profile given by
    // value, or to a group (its look-alike audience).  window: a floor, a cursor or neither (everybody
    // rankable); cap: the most entries the caller will take.  A window that holds more than cap throws
    // std::length_error (its what() names the total: raise the floor or the cap); any other failure
    // returns an empty list and last_error says why.  The engine's collector is set for this call and
    // cleared afterwards, under the engine's lock.
    Ranked collect_interest_all(int user, const ScoreWindow& window = ScoreWindow(), int64_t cap = 1 << 20) const {
        const pf_scan_window w = window.c_form();
        Collect col{cap};
        run_(3, user, 1, 0, nullptr, nullptr, &w, nullptr, &col);
        return col.take();
    }
    Ranked collect_by_profile(const Profile& A, const ScoreWindow& window = ScoreWindow(), int64_t cap = 1 << 20,
                              const std::vector<int>& exclude = {}) const {
        const pf_scan_window w = window.c_form();
        Collect col{cap};
        by_profile_(A, 1, exclude, &w, nullptr, &col);
        return col.take();
    }
    Ranked collect_for_group(const std::vector<int>& seeds, GroupAgg agg = GroupAgg::Mean, const ScoreWindow& window = ScoreWindow(),
                             int64_t cap = 1 << 20, bool exclude_adj = false, const std::vector<int>& exclude = {}) const {
        const pf_scan_window w = window.c_form();
        Collect col{cap};
        for_group_(seeds, 1, agg, exclude_adj, exclude, &w, nullptr, &col);
        return col.take();
    }

    // Clubs by interest (pokec_fas.h "Clubs by interest"): club recommendations from the NEIGHBOURS of a
    // user, of a profile given by value or of a group: the candidates of `window` in the all-candidates
    // ranking (the first `neighbours` of them; 0 = all), each adding its score to every club it lists, in
    // rank order; (club id, score) ranked (score desc, id asc).  No adj_list row is needed.  The query's
    // own clubs (the seeds' clubs for a group) are left out unless keep_own.  A window that holds more
    // than cap candidates throws std::length_error like collect_*; any other failure returns an empty
    // list and last_error says why.  info (optional) receives the call's pf_clubs_info.
    Ranked recommend_clubs_by_interest(int user, int topk, int neighbours = 0, const ScoreWindow& window = ScoreWindow(),
                                       int64_t cap = 1 << 20, bool keep_own = false, pf_clubs_info* info = nullptr) const {
        return clubs_(topk, neighbours, window, cap, keep_own, info, [&](detail::Engine& e, const pf_clubs_query* q, int k, int32_t* oc,
                                                                       float* os, int32_t* n, pf_clubs_info* ci) {
            return pf_recommend_clubs_interest(e.ctx, user, q, k, oc, os, n, ci);
        });
    }
    Ranked recommend_clubs_by_profile(const Profile& A, int topk, int neighbours = 0, const ScoreWindow& window = ScoreWindow(),
                                      int64_t cap = 1 << 20, bool keep_own = false, const std::vector<int>& exclude = {},
                                      pf_clubs_info* info = nullptr) const {
        return clubs_(topk, neighbours, window, cap, keep_own, info, [&](detail::Engine& e, const pf_clubs_query* q, int k, int32_t* oc,
                                                                       float* os, int32_t* n, pf_clubs_info* ci) {
            QueryHold h;
            const pf_query_profile qp = query_of_(e.ctx, A, exclude, h);
            return pf_recommend_clubs_profile(e.ctx, &qp, q, k, oc, os, n, ci);
        });
    }
    Ranked recommend_clubs_for_group(const std::vector<int>& seeds, int topk, GroupAgg agg = GroupAgg::Mean, int neighbours = 0,
                                     const ScoreWindow& window = ScoreWindow(), int64_t cap = 1 << 20, bool keep_own = false,
                                     bool exclude_adj = false, const std::vector<int>& exclude = {}, pf_clubs_info* info = nullptr) const {
        if (seeds.empty()) return Ranked();
        return clubs_(topk, neighbours, window, cap, keep_own, info, [&](detail::Engine& e, const pf_clubs_query* q, int k, int32_t* oc,
                                                                       float* os, int32_t* n, pf_clubs_info* ci) {
            if (exclude_adj && adj_list)
                for (int s : seeds) {
                    const int rc = sync_row_(e, s);
                    if (rc != PF_OK) return rc;
                }
            const std::vector<int32_t> sd(seeds.begin(), seeds.end()), ex(exclude.begin(), exclude.end());
            const pf_group_query g{sd.data(), (int32_t)sd.size(), (int32_t)agg, exclude_adj ? PF_GROUP_EXCLUDE_ADJ : 0u,
                                   ex.empty() ? nullptr : ex.data(), (int32_t)ex.size()};
            return pf_recommend_clubs_group(e.ctx, &g, q, k, oc, os, n, ci);
        });
    }

    // Diverse top-k (pokec_fas.h "Diverse top-k"): a ranking re-ranked by maximal marginal relevance.  Each
    // pick maximises lambda * score - (1 - lambda) * (its highest FAS with anything picked before); ties go to
    // the earlier entry.  diversify re-ranks a list the caller holds (unknown ids are dropped, of a repeated
    // id the first entry counts, at most PF_DIVERSE_MAX_POOL entries).  The recommend_diverse_* calls take
    // the first `pool` candidates of `window` in the all-candidates ranking as the pool; a window that holds
    // more than cap candidates throws std::length_error like clubs by interest; any other failure returns
    // an empty list and last_error says why.  info (optional) receives the call's pf_diverse_info.  The
    // pairs keep their relevance: (id, score) in pick order.
    Ranked diversify(const Ranked& list, int topk, float lambda) const {
        Ranked out;
        if (!profiles || topk <= 0 || list.empty()) return out;
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return out;
        std::lock_guard<std::mutex> g(e->mu);
        std::vector<int32_t> u, ids((size_t)std::min<size_t>((size_t)topk, list.size()));
        std::vector<float> s, sc(ids.size());
        for (const auto& p : list) {
            u.push_back(p.first);
            s.push_back(p.second);
        }
        int32_t n = 0;
        if (pf_diverse_rerank(e->ctx, u.data(), s.data(), (int64_t)u.size(), lambda, (int32_t)ids.size(), nullptr, ids.data(), sc.data(),
                              nullptr, nullptr, &n) != PF_OK)
            return fail_(e->ctx, out);
        for (int i = 0; i < n; ++i) out.emplace_back(ids[i], sc[i]);
        return out;
    }
    Ranked recommend_diverse_by_interest(int user, int topk, float lambda = 0.7f, int pool = 200, const ScoreWindow& window = ScoreWindow(),
                                         int64_t cap = 1 << 20, pf_diverse_info* info = nullptr) const {
        return diverse_(topk, lambda, pool, window, cap, info, [&](detail::Engine& e, const pf_diverse_query* q, int k, int32_t* ou,
                                                                  float* os, int32_t* n, pf_diverse_info* di) {
            if (adj_list) {  // the row the scan excludes, as the caller's adj_list holds it now
                const int rc = sync_row_(e, user);
                if (rc != PF_OK) return rc;
            }
            return pf_recommend_diverse_interest(e.ctx, user, q, k, ou, os, nullptr, nullptr, n, di);
        });
    }
    Ranked recommend_diverse_by_profile(const Profile& A, int topk, float lambda = 0.7f, int pool = 200,
                                        const ScoreWindow& window = ScoreWindow(), int64_t cap = 1 << 20,
                                        pf_diverse_info* info = nullptr, const std::vector<int>& exclude = {}) const {
        return diverse_(topk, lambda, pool, window, cap, info, [&](detail::Engine& e, const pf_diverse_query* q, int k, int32_t* ou,
                                                                  float* os, int32_t* n, pf_diverse_info* di) {
            QueryHold h;
            const pf_query_profile qp = query_of_(e.ctx, A, exclude, h);
            return pf_recommend_diverse_profile(e.ctx, &qp, q, k, ou, os, nullptr, nullptr, n, di);
        });
    }
    Ranked recommend_diverse_for_group(const std::vector<int>& seeds, int topk, float lambda = 0.7f, int pool = 200,
                                       const ScoreWindow& window = ScoreWindow(), int64_t cap = 1 << 20, pf_diverse_info* info = nullptr,
                                       GroupAgg agg = GroupAgg::Mean, bool exclude_adj = false, const std::vector<int>& exclude = {}) const {
        if (seeds.empty()) return Ranked();
        return diverse_(topk, lambda, pool, window, cap, info, [&](detail::Engine& e, const pf_diverse_query* q, int k, int32_t* ou,
                                                                  float* os, int32_t* n, pf_diverse_info* di) {
            if (exclude_adj && adj_list)
                for (int s : seeds) {
                    const int rc = sync_row_(e, s);
                    if (rc != PF_OK) return rc;
                }
            const std::vector<int32_t> sd(seeds.begin(), seeds.end()), ex(exclude.begin(), exclude.end());
            const pf_group_query g{sd.data(), (int32_t)sd.size(), (int32_t)agg, exclude_adj ? PF_GROUP_EXCLUDE_ADJ : 0u,
                                   ex.empty() ? nullptr : ex.data(), (int32_t)ex.size()};
            return pf_recommend_diverse_group(e.ctx, &g, q, k, ou, os, nullptr, nullptr, n, di);
        });
    }

    // The group's aggregate score of B, a profile of the map (NaN when B or every seed is not): how
    // well B fits the group.  No exclusion applies: a seed is scored like anyone else.
    float group_similarity(const std::vector<int>& seeds, const Profile& B, GroupAgg agg = GroupAgg::Mean) const {
        float out = NAN;
        if (!profiles || seeds.empty()) return out;
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return out;
        std::lock_guard<std::mutex> g(e->mu);
        const std::vector<int32_t> sd(seeds.begin(), seeds.end());
        const pf_group_query q{sd.data(), (int32_t)sd.size(), (int32_t)agg, 0u, nullptr, 0};
        const int32_t b = B.user_id;
        return pf_group_scores(e->ctx, &q, &b, 1, nullptr, &out) == PF_OK ? out : NAN;
    }

    // Push adj_list row `uid` to the engine now.  Never needed for correctness (every call
    // re-reads the rows it uses); kept for callers of the earlier facade.
    int sync_adjacency(int uid) const {
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e || !adj_list) return PF_ENODEV;
        std::lock_guard<std::mutex> g(e->mu);
        return sync_row_(*e, uid);
    }

    const std::string& last_error() const {
        std::lock_guard<std::mutex> g(err_mu_);
        return err_;
    }
    pf_ctx* engine() const {
        std::shared_ptr<detail::Engine> e = engine_();
        return e ? e->ctx : nullptr;
    }

    // the reference's public data members (include/recommender.h:49-60)
    const std::unordered_map<int, Profile>* profiles = nullptr;
    const AdjMap* adj_list = nullptr;
    NormMap field_normalizers;
    NormMap column_normalizers;
    IdfMap idf_per_col;
    size_t total_users = 0;

private:
    // The engine's score window for the span of one call (set here, cleared on the way out: the facade
    // keeps none in force between calls); total() reads the call's count when the window counts.
    struct WindowScope {
        pf_ctx* ctx;
        const pf_scan_window* w;
        int rc = PF_OK;
        WindowScope(pf_ctx* c, const pf_scan_window* win) : ctx(c), w(win) {
            if (w) rc = pf_set_scan_window(ctx, w);
        }
        ~WindowScope() {
            if (w) (void)pf_set_scan_window(ctx, nullptr);
        }
        bool total(int64_t* out) const {
            if (!w || !out || !(w->fields & PF_WIN_COUNT)) return true;
            int32_t n = 0;
            *out = 0;
            return pf_scan_window_totals(ctx, out, 1, &n) == PF_OK;
        }
    };

    // A collecting call's request and result: the engine's collector for the span of one call (set by
    // begin, cleared by end: the facade keeps none in force between calls), then the whole window.
    struct Collect {
        int64_t cap;
        Ranked all;
        int64_t total = 0;
        bool overflow = false;
        pf_ctx* ctx = nullptr;
        explicit Collect(int64_t c) : cap(c) {}
        int begin(pf_ctx* c) {
            const int rc = pf_set_scan_collect(c, cap > 0 ? cap : -1);
            if (rc == PF_OK) ctx = c;
            return rc;
        }
        // after the call: clears the collector and, when the call succeeded, reads its result
        int end(int rc) {
            if (!ctx) return rc;
            (void)pf_set_scan_collect(ctx, 0);
            if (rc != PF_OK) return rc;
            int64_t n = 0;
            if ((rc = pf_scan_collected(ctx, nullptr, nullptr, 0, &n, &total)) != PF_OK) return rc;
            overflow = total > cap;
            std::vector<int32_t> ids((size_t)n);
            std::vector<float> sc((size_t)n);
            if (n && (rc = pf_scan_collected(ctx, ids.data(), sc.data(), n, &n, &total)) != PF_OK) return rc;
            all.reserve((size_t)n);
            for (int64_t i = 0; i < n; ++i) all.emplace_back(ids[(size_t)i], sc[(size_t)i]);
            return PF_OK;
        }
        Ranked take() {
            if (overflow)
                throw std::length_error("collect: the window holds " + std::to_string(total) + " candidates, above the cap of " +
                                        std::to_string(cap));
            return std::move(all);
        }
    };

    // the three clubs-by-interest calls: call(engine, query, topk, out_club, out_score, out_count, info) -> rc
    template <class Call>
    Ranked clubs_(int topk, int neighbours, const ScoreWindow& window, int64_t cap, bool keep_own, pf_clubs_info* info, Call call) const {
        Ranked out;
        if (info) *info = pf_clubs_info{0, 0, 0, 0};
        if (!profiles || topk <= 0) return out;
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return out;
        pf_clubs_info ci{0, 0, 0, 0};
        {
            std::lock_guard<std::mutex> g(e->mu);
            const pf_scan_window w = window.c_form();
            const pf_clubs_query q{cap, neighbours, keep_own ? PF_CLUBS_KEEP_OWN : 0u, w.fields ? &w : nullptr};
            topk = (int)std::min<int64_t>(topk, e->n_club_entries + 1);  // a result never holds more than every club entry
            std::vector<int32_t> ids((size_t)topk);
            std::vector<float> sc((size_t)topk);
            int32_t n = 0;
            if (call(*e, &q, topk, ids.data(), sc.data(), &n, &ci) != PF_OK) return fail_(e->ctx, out);
            for (int i = 0; i < n; ++i) out.emplace_back(ids[i], sc[i]);
        }
        if (info) *info = ci;
        if (ci.total > cap)
            throw std::length_error("clubs by interest: the window holds " + std::to_string(ci.total) + " candidates, above the cap of " +
                                    std::to_string(cap));
        return out;
    }

    // the three diverse top-k calls: call(engine, query, topk, out_uid, out_score, out_count, info) -> rc
    template <class Call>
    Ranked diverse_(int topk, float lambda, int pool, const ScoreWindow& window, int64_t cap, pf_diverse_info* info, Call call) const {
        Ranked out;
        if (info) *info = pf_diverse_info{0, 0, 0, 0};
        if (!profiles || topk <= 0) return out;
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return out;
        pf_diverse_info di{0, 0, 0, 0};
        {
            std::lock_guard<std::mutex> g(e->mu);
            const pf_scan_window w = window.c_form();
            const pf_diverse_query q{cap, pool, lambda, w.fields ? &w : nullptr};
            topk = std::min(topk, PF_DIVERSE_MAX_POOL);  // a result never holds more than the pool
            std::vector<int32_t> ids((size_t)topk);
            std::vector<float> sc((size_t)topk);
            int32_t n = 0;
            if (call(*e, &q, topk, ids.data(), sc.data(), &n, &di) != PF_OK) return fail_(e->ctx, out);
            for (int i = 0; i < n; ++i) out.emplace_back(ids[i], sc[i]);
        }
        if (info) *info = di;
        if (di.total > cap)
            throw std::length_error("diverse top-k: the window holds " + std::to_string(di.total) + " candidates, above the cap of " +
                                    std::to_string(cap));
        return out;
    }

    Ranked by_profile_(const Profile& A, int topk, const std::vector<int>& exclude, const pf_scan_window* window,
                       int64_t* total, Collect* col = nullptr) const {
        Ranked out;
        if (!profiles || topk <= 0) return out;
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return out;
        std::lock_guard<std::mutex> g(e->mu);
        QueryHold h;
        const pf_query_profile q = query_of_(e->ctx, A, exclude, h);
        topk = (int)std::min<int64_t>(topk, e->n_users + 1);
        std::vector<int32_t> ids((size_t)topk);
        std::vector<float> sc((size_t)topk);
        int32_t n = 0;
        WindowScope ws(e->ctx, window);
        int rc = ws.rc;
        if (rc == PF_OK && col) rc = col->begin(e->ctx);
        if (rc == PF_OK) rc = pf_recommend_interest_profile(e->ctx, &q, 1, topk, ids.data(), sc.data(), &n);
        if (col) rc = col->end(rc);
        if (rc != PF_OK) return fail_(e->ctx, out);
        if (!ws.total(total)) return fail_(e->ctx, out);
        for (int i = 0; i < n; ++i) out.emplace_back(ids[i], sc[i]);
        return out;
    }

    Ranked for_group_(const std::vector<int>& seeds, int topk, GroupAgg agg, bool exclude_adj, const std::vector<int>& exclude,
                      const pf_scan_window* window, int64_t* total, Collect* col = nullptr) const {
        Ranked out;
        if (!profiles || topk <= 0 || seeds.empty()) return out;
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return out;
        std::lock_guard<std::mutex> g(e->mu);
        if (exclude_adj && adj_list)
            for (int s : seeds)
                if (sync_row_(*e, s) != PF_OK) return fail_(e->ctx, out);
        const std::vector<int32_t> sd(seeds.begin(), seeds.end()), ex(exclude.begin(), exclude.end());
        const pf_group_query q{sd.data(), (int32_t)sd.size(), (int32_t)agg, exclude_adj ? PF_GROUP_EXCLUDE_ADJ : 0u,
                               ex.empty() ? nullptr : ex.data(), (int32_t)ex.size()};
        std::vector<int32_t> ids((size_t)topk);
        std::vector<float> sc((size_t)topk);
        int32_t n = 0;
        WindowScope ws(e->ctx, window);
        int rc = ws.rc;
        if (rc == PF_OK && col) rc = col->begin(e->ctx);
        if (rc == PF_OK) rc = pf_recommend_group(e->ctx, &q, 1, topk, ids.data(), sc.data(), &n);
        if (col) rc = col->end(rc);
        if (rc != PF_OK) return fail_(e->ctx, out);
        if (!ws.total(total)) return fail_(e->ctx, out);
        for (int i = 0; i < n; ++i) out.emplace_back(ids[i], sc[i]);
        return out;
    }

    Ranked run_(int kind, int user, int topk, int limit, const pf_cand_filter* filter = nullptr,
                const pf_field_select* select = nullptr, const pf_scan_window* window = nullptr, int64_t* total = nullptr,
                Collect* col = nullptr) const {
        Ranked out;
        if (!profiles || !adj_list || topk <= 0) return out;
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return out;
        std::lock_guard<std::mutex> g(e->mu);
        // the rows this call reads, as the caller's adj_list holds them now
        int rc = sync_row_(*e, user);
        auto it = adj_list->find(user);
        if (it != adj_list->end() && kind != 3)
            for (int f : it->second)
                if (rc == PF_OK) rc = sync_row_(*e, f);
        if (rc != PF_OK) return fail_(e->ctx, out);
        // a result never holds more than every profile (or every club entry): size the
        // buffers by that, not by topk (the reference's callers pass up to 2^30)
        topk = (int)std::min<int64_t>(topk, kind == 2 ? e->n_club_entries + 1 : e->n_users + 1);
        std::vector<int32_t> ids((size_t)topk);
        std::vector<float> sc((size_t)topk);
        int32_t n = 0;
        const int32_t q = user;
        switch (kind) {
            case 0: rc = pf_recommend_interest(e->ctx, &q, 1, topk, PF_MODE_FOF, limit, ids.data(), sc.data(), &n); break;
            case 1: rc = pf_recommend_collab(e->ctx, &q, 1, topk, limit, ids.data(), sc.data(), &n); break;
            case 2: rc = pf_recommend_clubs(e->ctx, &q, 1, topk, limit, ids.data(), sc.data(), &n); break;
            default:
                if (filter) rc = pf_set_scan_filter(e->ctx, filter);
                if (select && rc == PF_OK) rc = pf_set_scan_select(e->ctx, select);
                {
                    WindowScope ws(e->ctx, rc == PF_OK ? window : nullptr);
                    if (rc == PF_OK) rc = ws.rc;
                    if (rc == PF_OK && col) rc = col->begin(e->ctx);
                    if (rc == PF_OK) rc = pf_recommend_interest(e->ctx, &q, 1, topk, PF_MODE_ALL, 0, ids.data(), sc.data(), &n);
                    if (col) rc = col->end(rc);
                    if (rc == PF_OK && !ws.total(total)) rc = PF_EINTERNAL;
                }
                if (filter) {  // the filter in force before the call
                    const int rr = pf_set_scan_filter(e->ctx, e->scan_filter.fields ? &e->scan_filter : nullptr);
                    if (rc == PF_OK) rc = rr;
                }
                if (select) {  // and the selection
                    const int rr = pf_set_scan_select(e->ctx, e->has_scan_select ? &e->scan_select : nullptr);
                    if (rc == PF_OK) rc = rr;
                }
                break;
        }
        if (rc != PF_OK) return fail_(e->ctx, out);
        out.reserve((size_t)n);
        for (int i = 0; i < n; ++i) out.emplace_back(ids[i], sc[i]);
        return out;
    }

    float pair_(const std::shared_ptr<detail::Engine>& e, int a, int b, const pf_field_select* select = nullptr) const {
        if (!e) return NAN;
        std::lock_guard<std::mutex> g(e->mu);
        const int32_t x = a, y = b;
        float out = NAN;
        const int rc = select ? pf_fas_pairs_select(e->ctx, &x, &y, 1, select, &out) : pf_fas_pairs(e->ctx, &x, &y, 1, &out);
        return rc == PF_OK ? out : NAN;
    }

    ScoreTerms pair_terms_(const std::shared_ptr<detail::Engine>& e, int a, int b, const pf_field_select* select) const {
        ScoreTerms out;
        if (!e) return out;
        try {
            std::lock_guard<std::mutex> g(e->mu);
            const int32_t x = a, y = b;
            pf_pair_terms_head h{};
            std::vector<double> row((size_t)(PF_NUM_FIXED + pf_num_cols(e->ctx)));
            if (pf_fas_pairs_terms(e->ctx, &x, &y, 1, select, &h, row.data()) != PF_OK || h.score != h.score) return out;
            out.score = h.score;
            out.fixed = h.fixed;
            out.cols = h.cols;
            out.terms = std::move(row);
        } catch (...) {  // an allocation failure: the empty result
            return ScoreTerms{};
        }
        return out;
    }

    // the arrays behind a pf_query_profile built from a Profile
    struct QueryHold {
        std::vector<int64_t> off;
        std::vector<int32_t> tid, tf, excl;
    };
    pf_query_profile query_of_(pf_ctx* c, const Profile& A, const std::vector<int>& exclude, QueryHold& h) const {
        const int T = pf_num_cols(c);
        h.off.assign(1, 0);
        for (int t = 0; t < T; ++t) {
            if ((size_t)t < A.token_cols.size())
                for (const auto& kv : A.token_cols[(size_t)t]) {
                    h.tid.push_back(kv.first);
                    h.tf.push_back(kv.second);
                }
            h.off.push_back((int64_t)h.tid.size());
        }
        h.excl.assign(exclude.begin(), exclude.end());
        pf_query_profile q{};
        q.public_flag = A.public_flag;
        q.gender = A.gender;
        q.completion = A.completion_percentage;
        q.age = A.age;
        for (int k = 0; k < 3; ++k) q.region[k] = A.region_parts[(size_t)k];
        q.club_ids = A.clubs.data();
        q.n_clubs = (int32_t)A.clubs.size();
        q.friend_ids = A.friends.data();
        q.n_friends = (int32_t)A.friends.size();
        q.tok_off = h.off.data();
        q.tok_tid = h.tid.data();
        q.tok_tf = h.tf.data();
        q.exclude_uid = h.excl.data();
        q.n_exclude = (int32_t)h.excl.size();
        return q;
    }

    float adhoc_(const Profile& A, int b, const pf_field_select* select) const {
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return NAN;
        try {
            std::lock_guard<std::mutex> g(e->mu);
            QueryHold h;
            const pf_query_profile q = query_of_(e->ctx, A, {}, h);
            const int32_t y = b;
            float out = NAN;
            return pf_fas_profile_pairs(e->ctx, &q, &y, 1, select, &out) == PF_OK ? out : NAN;
        } catch (...) {
            return NAN;
        }
    }

    ScoreTerms adhoc_terms_(const Profile& A, int b, const pf_field_select* select) const {
        ScoreTerms out;
        std::shared_ptr<detail::Engine> e = engine_();
        if (!e) return out;
        try {
            std::lock_guard<std::mutex> g(e->mu);
            QueryHold hold;
            const pf_query_profile q = query_of_(e->ctx, A, {}, hold);
            const int32_t y = b;
            pf_pair_terms_head h{};
            std::vector<double> row((size_t)(PF_NUM_FIXED + pf_num_cols(e->ctx)));
            if (pf_fas_profile_pairs_terms(e->ctx, &q, &y, 1, select, &h, row.data()) != PF_OK || h.score != h.score) return out;
            out.score = h.score;
            out.fixed = h.fixed;
            out.cols = h.cols;
            out.terms = std::move(row);
        } catch (...) {
            return ScoreTerms{};
        }
        return out;
    }

    Ranked fail_(pf_ctx* c, Ranked& out) const {
        std::lock_guard<std::mutex> g(err_mu_);
        err_ = pf_last_error(c);
        return out;
    }

    // The engine's row of x := the caller's adj_list row of x (absent rows erased).
    int sync_row_(detail::Engine& e, int x) const {
        auto ci = adj_list->find(x);
        auto ei = e.rows.find(x);
        const bool cp = ci != adj_list->end(), ep = ei != e.rows.end();
        if (!cp && !ep) return PF_OK;
        if (cp && ep && ci->second == ei->second) return PF_OK;
        if (!cp) {
            e.rows.erase(ei);
            return pf_set_adj(e.ctx, x, nullptr, -1);
        }
        e.rows[x] = ci->second;
        static_assert(sizeof(int) == sizeof(int32_t), "adj_list rows pass as int32");
        return pf_set_adj(e.ctx, x, reinterpret_cast<const int32_t*>(ci->second.data()), (int32_t)ci->second.size());
    }

    void reset_() {
        std::lock_guard<std::mutex> g(open_mu_);
        eng_.reset();
    }

    std::shared_ptr<detail::Engine> engine_() const {
        std::lock_guard<std::mutex> g(open_mu_);
        if (!eng_) eng_ = open_for_(text_columns_internal_);
        return eng_;
    }

    // The shared engine for scoring columns `cols` with this object's settings (opened on first use).
    std::shared_ptr<detail::Engine> open_for_(const std::vector<std::string>& cols) const {
        if (!profiles || !adj_list) {
            std::lock_guard<std::mutex> g(err_mu_);
            err_ = "null profiles or adj_list";
            return nullptr;
        }
        detail::EngineKey key;
        key.profiles = profiles;
        key.n_profiles = profiles->size();
        key.fingerprint = detail::profiles_fingerprint(*profiles);
        key.device = device_;
        key.cols = cols;
        key.field = field_normalizers;
        key.column = column_normalizers;
        // the idf values by column name (recommender_similarity.cpp:97-104), whether computed
        // (compute_idf_from_profiles over these columns: the engine recomputes them, F3) or
        // explicit (set_tfidf_index): equal values score equally
        key.idf = std::make_shared<const IdfMap>(idf_per_col);
        const bool computed = idf_computed_ && idf_cols_ == cols;
        auto& R = detail::registry();
        std::lock_guard<std::mutex> g(R.mu);
        for (auto it = R.engines.begin(); it != R.engines.end(); ++it)
            if (it->first.same(key)) {
                R.engines.splice(R.engines.begin(), R.engines, it);  // most recently used first
                return R.engines.front().second;
            }
        auto e = std::make_shared<detail::Engine>();
        if (!open_with_(cols, computed, *e)) return nullptr;
        R.engines.emplace_front(std::move(key), e);
        int idle = 0;  // keep at most kMaxEngines engines nobody holds
        for (auto it = R.engines.begin(); it != R.engines.end();) {
            if (it->second.use_count() == 1 && ++idle > kMaxEngines) it = R.engines.erase(it);
            else ++it;
        }
        return e;
    }

    // Flatten the maps into a pf_corpus_desc over column list `cols` and open an engine context.
    bool open_with_(const std::vector<std::string>& cols, bool computed, detail::Engine& e) const {
        const int T = (int)cols.size();
        D d;
        const size_t n = profiles->size();
        d.club_off.push_back(0); d.friend_off.push_back(0); d.tok_off.push_back(0);
        for (auto& kv : *profiles) {
            const Profile& p = kv.second;
            d.uid.push_back(kv.first); d.pub.push_back(p.public_flag); d.comp.push_back(p.completion_percentage);
            d.gen.push_back(p.gender); d.age.push_back(p.age);
            for (int k = 0; k < 3; ++k) d.reg.push_back(p.region_parts[k]);
            d.clubs.insert(d.clubs.end(), p.clubs.begin(), p.clubs.end());
            d.club_off.push_back((int64_t)d.clubs.size());
            d.friends.insert(d.friends.end(), p.friends.begin(), p.friends.end());
            d.friend_off.push_back((int64_t)d.friends.size());
            for (int t = 0; t < T; ++t) {
                if ((size_t)t < p.token_cols.size())
                    for (auto& pr : p.token_cols[t]) { d.tid.push_back(pr.first); d.tf.push_back(pr.second); }
                d.tok_off.push_back((int64_t)d.tid.size());
            }
        }
        d.adj_off.push_back(0);
        for (auto& kv : *adj_list) {
            d.adj_uid.push_back(kv.first);
            d.adj_nbr.insert(d.adj_nbr.end(), kv.second.begin(), kv.second.end());
            d.adj_off.push_back((int64_t)d.adj_nbr.size());
        }
        static const char* const keys[PF_NUM_FIXED] = {"public", "gender", "completion", "age",
                                                       "region", "clubs", "friends"};
        d.npres.assign(PF_NUM_FIXED + T, 0);
        d.nmean.assign(PF_NUM_FIXED + T, 0.f);
        d.nsd.assign(PF_NUM_FIXED + T, 0.f);
        for (int k = 0; k < PF_NUM_FIXED + T; ++k) {
            const NormMap& m = k < PF_NUM_FIXED ? field_normalizers : column_normalizers;
            auto it = m.find(k < PF_NUM_FIXED ? std::string(keys[k]) : cols[k - PF_NUM_FIXED]);
            if (it == m.end()) continue;
            d.npres[k] = 1; d.nmean[k] = it->second.first; d.nsd[k] = it->second.second;
        }
        pf_corpus_desc c{};
        c.n_users = (int32_t)n; c.n_cols = T;
        c.user_id = d.uid.data(); c.public_flag = d.pub.data(); c.completion = d.comp.data();
        c.gender = d.gen.data(); c.age = d.age.data(); c.region = d.reg.data();
        c.club_off = d.club_off.data(); c.club_ids = d.clubs.data();
        c.friend_off = d.friend_off.data(); c.friend_ids = d.friends.data();
        c.tok_off = d.tok_off.data(); c.tok_tid = d.tid.data(); c.tok_tf = d.tf.data();
        c.n_adj = (int32_t)d.adj_uid.size();
        c.adj_uid = d.adj_uid.data(); c.adj_off = d.adj_off.data(); c.adj_nbr = d.adj_nbr.data();
        c.norm_present = d.npres.data(); c.norm_mean = d.nmean.data(); c.norm_sd = d.nsd.data();
        if (computed) {  // recommender.cpp:43-66 over the same columns: the engine computes it (F3)
            c.idf_mode = PF_IDF_FROM_PROFILES;
        } else {
            c.idf_mode = PF_IDF_EXPLICIT;
            d.has_idf.assign(T, 0);
            d.idf_off.push_back(0);
            for (int t = 0; t < T; ++t) {
                auto it = idf_per_col.find(cols[t]);
                if (it != idf_per_col.end()) {
                    d.has_idf[t] = 1;
                    for (auto& pr : it->second) { d.idf_tid.push_back(pr.first); d.idf_val.push_back(pr.second); }
                }
                d.idf_off.push_back((int64_t)d.idf_tid.size());
            }
            c.col_has_idf = d.has_idf.data(); c.idf_off = d.idf_off.data();
            c.idf_tid = d.idf_tid.data(); c.idf_val = d.idf_val.data();
        }
        if (pf_open(&c, device_, &e.ctx) != PF_OK) {
            std::lock_guard<std::mutex> g(err_mu_);
            err_ = pf_last_error(nullptr);
            e.ctx = nullptr;
            return false;
        }
        e.rows = *adj_list;
        e.n_users = (int64_t)n;
        e.n_club_entries = (int64_t)d.clubs.size();
        return true;
    }

    // recommender.cpp:43-66, one column per thread (the counts and logf per column are the
    // reference's; only independent columns run side by side)
    void compute_idf_(const std::vector<std::string>& cols, IdfMap& out) const {
        const float N = (float)profiles->size();
        std::vector<std::unordered_map<int, float>> per(cols.size());
        auto col = [&](size_t t) {
            std::unordered_map<int, int> df;
            for (auto& kv : *profiles)
                if (t < kv.second.token_cols.size())
                    for (auto& pr : kv.second.token_cols[t]) df[pr.first] += 1;
            for (auto& pr : df) per[t][pr.first] = logf(1.0f + N / (1.0f + (float)pr.second));
        };
        const size_t nt = std::min<size_t>(cols.size(), std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
        std::vector<std::thread> ts;
        for (size_t w = 0; w < nt; ++w)
            ts.emplace_back([&, w]() {
                for (size_t t = w; t < cols.size(); t += nt) col(t);
            });
        for (auto& t : ts) t.join();
        for (size_t t = 0; t < cols.size(); ++t) out[cols[t]] = std::move(per[t]);
    }

    struct D {
        std::vector<int32_t> uid, pub, comp, gen, age, reg, tid, tf, adj_uid, adj_nbr, idf_tid;
        std::vector<int64_t> club_off, friend_off, tok_off, adj_off, idf_off;
        std::vector<uint32_t> clubs, friends;
        std::vector<uint8_t> npres, has_idf;
        std::vector<float> nmean, nsd, idf_val;
    };

    int device_ = 0;
    std::vector<std::string> text_columns_internal_;
    std::vector<std::string> idf_cols_;
    bool idf_computed_ = false;
    mutable std::mutex open_mu_, err_mu_;
    mutable std::shared_ptr<detail::Engine> eng_;
    mutable std::string err_;
};

using Recommender = BasicRecommender<UserProfile>;

}  // namespace pokec

#ifdef POKEC_DROP_IN
// the reference's names: ::UserProfile is the caller's (the reference's user_profile.h)
using Recommender = pokec::BasicRecommender<::UserProfile>;
#endif

#endif  // POKEC_RECOMMENDER_H
