// pf_filter.h — the all-candidates scans' candidate filter (DESIGN.md "Candidate filters"): the
// device form of pf_cand_filter and its test on the two candidate headers.  Plain C++ on both
// sides, so the CPU test (tests/cpp/filter_check.cpp) runs the text the kernels run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_FHD __host__ __device__
#else
#define PF_FHD
#endif

namespace pf {

// field bits and flags: the values of PF_FILT_* (pokec_fas.h; pf_api.cpp asserts they agree)
constexpr uint32_t kFiltGender = 1u, kFiltPublic = 2u, kFiltAge = 4u, kFiltCompletion = 8u, kFiltRegion = 16u;
constexpr uint32_t kFiltAllFields = 31u;
constexpr uint32_t kFiltKeepMissing = 1u;
// header code of a missing public / gender value (pf_types.h kCodeMissing), and the code the host
// gives a filter value no user has: never equal to a header's byte
constexpr uint32_t kFiltCodeMissing = 0xFFu, kFiltCodeNobody = 0x100u;

// Passed by value as a kernel argument.  fields == 0: no filter.  pub / gen are the headers'
// equality codes of the filter's values (translated once on the host); ages, completions and
// region parts are compared in the domain the corpus was given in.
struct CandFilter {
    uint32_t fields, flags;
    uint32_t pub, gen;
    int32_t age_min, age_max;
    int32_t comp_min, comp_max;
    int32_t reg[3];
    uint32_t pad;
};
static_assert(sizeof(CandFilter) == 48, "CandFilter is a 48-B kernel argument");

// The test on a candidate's decoded fields.  Missing follows FAS (recommender_similarity.cpp:38-79):
// a code of kFiltCodeMissing (the value was < 0), an age / completion <= 0, a region part < 0; a
// missing tested field passes only with kFiltKeepMissing.
PF_FHD inline bool filter_pass(const CandFilter& F, uint32_t pb, uint32_t gb, int32_t comp, int32_t age, int32_t r0,
                               int32_t r1, int32_t r2) {
    const bool keep = (F.flags & kFiltKeepMissing) != 0u;
    bool ok = true;
    if (F.fields & kFiltGender) ok = ok && (gb == kFiltCodeMissing ? keep : gb == F.gen);
    if (F.fields & kFiltPublic) ok = ok && (pb == kFiltCodeMissing ? keep : pb == F.pub);
    if (F.fields & kFiltAge) ok = ok && (age <= 0 ? keep : (age >= F.age_min && age <= F.age_max));
    if (F.fields & kFiltCompletion) ok = ok && (comp <= 0 ? keep : (comp >= F.comp_min && comp <= F.comp_max));
    if (F.fields & kFiltRegion) {
        ok = ok && (F.reg[0] < 0 || (r0 < 0 ? keep : r0 == F.reg[0]));
        ok = ok && (F.reg[1] < 0 || (r1 < 0 ? keep : r1 == F.reg[1]));
        ok = ok && (F.reg[2] < 0 || (r2 < 0 ? keep : r2 == F.reg[2]));
    }
    return ok;
}

// Postings header (pf_types.h PostStore): ha = {colmask lo, colmask hi16 | pub << 16 | gen << 24,
// (i16) completion | (i16) age << 16, set sizes}, hb = {region0, region1, region2, uid}.  U4 is any
// type with 32-bit members x, y, z, w (uint4 on the device).
template <class U4>
PF_FHD inline bool filter_pass_post(const CandFilter& F, const U4& ha, const U4& hb) {
    return filter_pass(F, ((uint32_t)ha.y >> 16) & 0xFFu, (uint32_t)ha.y >> 24, (int32_t)(int16_t)((uint32_t)ha.z & 0xFFFFu),
                       (int32_t)(int16_t)((uint32_t)ha.z >> 16), (int32_t)hb.x, (int32_t)hb.y, (int32_t)hb.z);
}

// Tile-store header (pf_types.h): h0 = {colmask lo, colmask hi, completion, age}, h1 = {region0,
// region1, region2, uid}, h2 = {pub | gen << 8, n_clubs, n_friends, n_tok}.
template <class U4>
PF_FHD inline bool filter_pass_tile(const CandFilter& F, const U4& h0, const U4& h1, const U4& h2) {
    return filter_pass(F, (uint32_t)h2.x & 0xFFu, ((uint32_t)h2.x >> 8) & 0xFFu, (int32_t)h0.z, (int32_t)h0.w,
                       (int32_t)h1.x, (int32_t)h1.y, (int32_t)h1.z);
}

}  // namespace pf
