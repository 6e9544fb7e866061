// Host check of the candidate filter (csrc/pf_filter.h, the text the kernels run): candidates over
// every combination of field values (missing ones, ages / completions 1, 128, 129 and 32767 around
// the sigmoid tables' end and the 16-bit field's, a region part of 2,000,000,000, public / gender
// values 2 and 77) are packed into both header encodings the way the stores pack them, and every
// filter (each field alone, all 32 field sets, with and without KEEP_MISSING, values nobody has)
// must give on both what a plain restatement over the raw values gives.
// Prints "sizeof <n>" and "ok <cases>", or the first mismatch.
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "pf_filter.h"
#include "pokec_fas.h"

struct U4 {
    uint32_t x, y, z, w;
};

struct Cand {
    int32_t pub, gen, comp, age, reg[3];
};

// the rule as the issue states it, on the corpus's own values
static bool plain(const pf_cand_filter& f, const Cand& c) {
    const bool keep = (f.flags & PF_FILT_KEEP_MISSING) != 0;
    if (f.fields & PF_FILT_GENDER) {
        if (c.gen < 0) { if (!keep) return false; }
        else if (c.gen != f.gender) return false;
    }
    if (f.fields & PF_FILT_PUBLIC) {
        if (c.pub < 0) { if (!keep) return false; }
        else if (c.pub != f.public_flag) return false;
    }
    if (f.fields & PF_FILT_AGE) {
        if (c.age <= 0) { if (!keep) return false; }
        else if (c.age < f.age_min || c.age > f.age_max) return false;
    }
    if (f.fields & PF_FILT_COMPLETION) {
        if (c.comp <= 0) { if (!keep) return false; }
        else if (c.comp < f.completion_min || c.comp > f.completion_max) return false;
    }
    if (f.fields & PF_FILT_REGION) {
        for (int i = 0; i < 3; ++i) {
            if (f.region[i] < 0) continue;
            if (c.reg[i] < 0) { if (!keep) return false; }
            else if (c.reg[i] != f.region[i]) return false;
        }
    }
    return true;
}

int main() {
    std::printf("sizeof %zu %zu\n", sizeof(pf_cand_filter), sizeof(pf::CandFilter));
    if (sizeof(pf::CandFilter) > 48) {
        std::printf("CandFilter larger than 48 B\n");
        return 1;
    }
    const int32_t codes_vals[] = {0, 1, 2, 77};  // the corpus's distinct public / gender values -> codes 0..3
    std::map<int32_t, uint32_t> code;
    for (uint32_t k = 0; k < 4; ++k) code[codes_vals[k]] = k;
    auto enc = [&](int32_t v) -> uint32_t { return v < 0 ? pf::kFiltCodeMissing : code.at(v); };
    auto fcode = [&](int32_t v) -> uint32_t {  // the host's translation of a filter value (pf_set_scan_filter)
        auto it = v < 0 ? code.end() : code.find(v);
        return it == code.end() ? pf::kFiltCodeNobody : it->second;
    };
    const int32_t eq_vals[] = {-1, 0, 1, 2, 77};
    const int32_t num_vals[] = {-5, 0, 1, 20, 128, 129, 32767};
    const int32_t reg_vals[] = {-1, 0, 3, 2000000000};
    std::vector<Cand> cands;
    for (int32_t pub : eq_vals)
        for (int32_t gen : eq_vals)
            for (int32_t comp : num_vals)
                for (int32_t age : num_vals)
                    for (int32_t r0 : reg_vals)
                        for (int32_t r1 : reg_vals) cands.push_back(Cand{pub, gen, comp, age, {r0, r1, (r0 ^ r1) & 1 ? 3 : -1}});
    struct Rng { int32_t lo, hi; };
    const Rng rngs[] = {{1, 1}, {1, 128}, {128, 129}, {129, 32767}, {20, 29}, {32767, 32767}, {1, 2147483647}, {-7, 0}};
    const int32_t feq[] = {0, 1, 2, 77, 5, -1};
    const int32_t fregs[][3] = {{3, -1, -1}, {-1, 3, -1}, {2000000000, 0, -1}, {0, 0, 3}, {-1, -1, 3}, {3, 3, 3}};
    std::vector<pf_cand_filter> filters;
    for (uint32_t fields = 0; fields < 32; ++fields)
        for (uint32_t flags = 0; flags < 2; ++flags)
            for (int v = 0; v < 8; ++v) {
                pf_cand_filter f{};
                f.fields = fields;
                f.flags = flags;
                f.gender = feq[v % 6];
                f.public_flag = feq[(v + 3) % 6];
                f.age_min = rngs[v].lo;
                f.age_max = rngs[v].hi;
                f.completion_min = rngs[(v + 3) % 8].lo;
                f.completion_max = rngs[(v + 3) % 8].hi;
                for (int i = 0; i < 3; ++i) f.region[i] = fregs[v % 6][i];
                filters.push_back(f);
            }
    long cases = 0, passed = 0;
    for (const pf_cand_filter& f : filters) {
        pf::CandFilter d{};
        d.fields = f.fields;
        d.flags = f.flags;
        d.pub = fcode(f.public_flag);
        d.gen = fcode(f.gender);
        d.age_min = f.age_min;
        d.age_max = f.age_max;
        d.comp_min = f.completion_min;
        d.comp_max = f.completion_max;
        for (int i = 0; i < 3; ++i) d.reg[i] = (f.fields & PF_FILT_REGION) ? f.region[i] : -1;
        for (const Cand& c : cands) {
            // postings header (pf_types.h PostStore) and tile header, as pf_store.cpp packs them
            const U4 ha{0xDEADBEEFu, 0xBEEFu | enc(c.pub) << 16 | enc(c.gen) << 24,
                        ((uint32_t)c.comp & 0xFFFFu) | ((uint32_t)c.age & 0xFFFFu) << 16, 0x00070009u};
            const U4 hb{(uint32_t)c.reg[0], (uint32_t)c.reg[1], (uint32_t)c.reg[2], 12345u};
            const U4 h0{0xDEADBEEFu, 0xBEEFu, (uint32_t)c.comp, (uint32_t)c.age};
            const U4 h2{enc(c.pub) | enc(c.gen) << 8, 9u, 7u, 100u};
            const bool want = plain(f, c);
            const bool post = pf::filter_pass_post(d, ha, hb), tile = pf::filter_pass_tile(d, h0, hb, h2);
            ++cases;
            passed += want;
            if (post != want || tile != want) {
                std::printf("fields=%u flags=%u gender=%d public=%d age=[%d,%d] comp=[%d,%d] region=(%d,%d,%d) on pub=%d gen=%d "
                            "comp=%d age=%d reg=(%d,%d,%d): want %d, postings %d, tile %d\n",
                            f.fields, f.flags, f.gender, f.public_flag, f.age_min, f.age_max, f.completion_min,
                            f.completion_max, f.region[0], f.region[1], f.region[2], c.pub, c.gen, c.comp, c.age, c.reg[0],
                            c.reg[1], c.reg[2], (int)want, (int)post, (int)tile);
                return 1;
            }
        }
    }
    if (passed == 0 || passed == cases) {
        std::printf("vacuous sweep: %ld of %ld pass\n", passed, cases);
        return 1;
    }
    std::printf("ok %ld cases, %ld pass\n", cases, passed);
    return 0;
}
