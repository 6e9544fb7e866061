/*
 * pokec_fas.h — C ABI of the MI355X-native Fill-Aware-Similarity (FAS) engine.
 *
 * Drop-in boundary for the hot path of pymlex/recommendation-system-pokec:
 *   - Recommender::profile_similarity        src/recommender_similarity.cpp:10-124  (FAS, A10)
 *   - Recommender::tfidf_cosine_for_column   src/recommender.cpp:68-117             (A6)
 *   - Recommender::vec_set_similarity        src/recommender.cpp:119-128            (A8)
 *   - Recommender::region_similarity_local   src/recommender.cpp:130-139            (A9)
 *   - Recommender::compute_idf_from_profiles src/recommender.cpp:43-66              (A4)
 *   - gather_candidates_local                src/recommender_graph.cpp:10-31        (A11)
 *   - recommend_graph_registration / _by_interest  src/recommender_graph.cpp:33-103,224-227 (A12)
 *   - recommend_collaborative                src/recommender_graph.cpp:105-222      (A14)
 *   - recommend_clubs_collab                 src/recommender_clubs.cpp:10-73        (A15)
 *   - build_adj_list / GraphBuilder          src/utils.cpp:26-34, src/graph_builder.cpp:39-59 (A17)
 *
 * The reference exposes these as methods of the C++ class `Recommender`
 * (include/recommender.h:17-71).  This header is the flat C ABI the C++
 * facade (include/pokec/recommender.h) and any FFI (ctypes, cgo, JNI) bind.
 * Shape follows the reference's only FFI precedent, lemmagen
 * (third_party/lemmagen/include/lemmagen.h:40-76): extern "C", int status
 * codes, caller-owned buffers, no exceptions across the boundary.
 *
 * Conventions
 *   - 0 = PF_OK, < 0 = error; pf_last_error() describes the last failure.
 *   - All pointers in pf_corpus_desc are HOST pointers owned by the caller;
 *     pf_open copies everything it needs to the GPU and keeps no reference.
 *   - An unknown query uid yields count 0 (the reference returns an empty
 *     vector: recommender_graph.cpp:36-40,130; recommender_clubs.cpp:13-16).
 *   - One context per host thread; distinct contexts are independent.
 *   - There is NO CPU fallback: if the HIP runtime or a gfx950 device is
 *     missing, pf_open fails with PF_ENODEV.
 */
#ifndef POKEC_FAS_H
#define POKEC_FAS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 2

/* status codes */
#define PF_OK          0
#define PF_EINVAL     -1   /* bad argument / malformed descriptor            */
#define PF_ENODEV     -2   /* no HIP device / HIP runtime failure            */
#define PF_ENOMEM     -3   /* host or device allocation failed               */
#define PF_ENOTFOUND  -4   /* query uid has no profile (outputs count 0)     */
#define PF_EUNSUPP    -5   /* input outside what the device layout encodes   */
#define PF_EINTERNAL  -6

/* Number of fixed (structured) fields of FAS, recommender_similarity.cpp:12 */
#define PF_NUM_FIXED   7
#define PF_MAX_COLS    64
/* fixed-field normaliser slots, recommender_similarity.cpp:28-91 order */
#define PF_F_PUBLIC     0
#define PF_F_GENDER     1
#define PF_F_COMPLETION 2
#define PF_F_AGE        3
#define PF_F_REGION     4
#define PF_F_CLUBS      5
#define PF_F_FRIENDS    6

/* IDF source (Recommender::compute_idf_from_profiles vs set_tfidf_index) */
#define PF_IDF_FROM_PROFILES 0  /* idf = logf(1 + N/(1+df)), recommender.cpp:43-66 */
#define PF_IDF_EXPLICIT      1  /* use idf_* arrays below (set_tfidf_index)          */

/* candidate-set modes for interest scoring */
#define PF_MODE_FOF   0  /* reference: 2-hop candidates truncated at candidate_limit (A12) */
#define PF_MODE_ALL   1  /* every loaded profile except q and adj[q] (A13)                 */

/* 2-hop gather flavours (they differ, see A11 vs A14 in SURVEY.md) */
#define PF_FOF_GRAPH  0  /* gather_candidates_local, recommender_graph.cpp:10-31  */
#define PF_FOF_COLLAB 1  /* collaborative candidate loop, recommender_graph.cpp:114-125 */

/*
 * In-memory corpus: the reference's unordered_map<int,UserProfile>
 * (include/user_profile.h:10-20) plus adj_list, normalisers and IDF,
 * flattened to CSR.  Profiles may be given in any order; user ids must be
 * distinct.  Ages must already be median-filled (api_cli.cpp:139-153).
 */
typedef struct pf_corpus_desc {
    int32_t         n_users;
    int32_t         n_cols;        /* T: number of text columns (<= PF_MAX_COLS)  */

    const int32_t*  user_id;       /* [n_users]                                    */
    const int32_t*  public_flag;   /* [n_users]  -1 = missing                      */
    const int32_t*  completion;    /* [n_users]  used when > 0                     */
    const int32_t*  gender;        /* [n_users]  -1 = missing                      */
    const int32_t*  age;           /* [n_users]  used when > 0                     */
    const int32_t*  region;        /* [3*n_users] -1 = missing part                */

    const int64_t*  club_off;      /* [n_users+1]                                  */
    const uint32_t* club_ids;      /* clubs in profile order, duplicates allowed   */
    const int64_t*  friend_off;    /* [n_users+1]                                  */
    const uint32_t* friend_ids;    /* profile `friends` column (NOT adj_list)      */

    const int64_t*  tok_off;       /* [n_users*n_cols+1], row (u,t) = u*n_cols+t   */
    const int32_t*  tok_tid;       /* token ids; distinct within a row             */
    const int32_t*  tok_tf;        /* token counts                                 */

    /* adj_list (unordered_map<int, vector<int>>): directed, file order, dups kept */
    int32_t         n_adj;
    const int32_t*  adj_uid;       /* [n_adj] distinct                             */
    const int64_t*  adj_off;       /* [n_adj+1]                                    */
    const int32_t*  adj_nbr;

    /* IDF (idf_per_col).  idf_mode = PF_IDF_FROM_PROFILES ignores the arrays.
     * PF_IDF_EXPLICIT: col_has_idf[t] = 0 means the column name is absent from
     * idf_per_col (raw-count cosine, recommender_similarity.cpp:102-104);
     * otherwise row t of (idf_off, idf_tid, idf_val) is its map; a token absent
     * from a present map gets idf 1.0 (recommender.cpp:78). */
    int32_t         idf_mode;
    const uint8_t*  col_has_idf;   /* [n_cols]                                     */
    const int64_t*  idf_off;       /* [n_cols+1]                                   */
    const int32_t*  idf_tid;
    const float*    idf_val;

    /* normalisers, slots 0..6 = field_normalizers["public".."friends"],
     * 7+t = column_normalizers[text_columns[t]]; norm_present = 0 means the key
     * is absent (then z = 6(s-0.5), recommender_similarity.cpp:28-36). */
    const uint8_t*  norm_present;  /* [PF_NUM_FIXED + n_cols]                      */
    const float*    norm_mean;
    const float*    norm_sd;
} pf_corpus_desc;

typedef struct pf_ctx pf_ctx;

int         pf_abi_version(void);
/* Copies the corpus to device `device` (HIP ordinal) and builds the tile store. */
int         pf_open(const pf_corpus_desc* desc, int device, pf_ctx** out);
void        pf_close(pf_ctx* ctx);
/* Message of the last failure on ctx (or of the last failed pf_open when ctx is NULL). */
const char* pf_last_error(const pf_ctx* ctx);
int32_t     pf_num_users(const pf_ctx* ctx);
/* float32 IDF the context uses for (col, tid); 1.0 for an absent token; NaN when
 * the column has no idf map (raw-count cosine). */
float       pf_idf(const pf_ctx* ctx, int32_t col, int32_t tid);

/* FAS(A=a_uid[i], B=b_uid[i]) for n pairs (profile_similarity(A,B)); a pair with
 * an unknown uid scores NaN.  Parity probe for recommender_similarity.cpp:10-124. */
int pf_fas_pairs(pf_ctx* ctx, const int32_t* a_uid, const int32_t* b_uid,
                 int64_t n, float* out);

/*
 * Top-k recommenders.  For every query i the results go to
 * out_uid[i*topk .. ], out_score[i*topk .. ], out_count[i] (<= topk), sorted
 * by (score desc, id asc) exactly as recommender_graph.cpp:97-101.
 *   pf_recommend_interest: mode PF_MODE_FOF = recommend_graph_registration /
 *       recommend_by_interest(u, topk, candidate_limit); PF_MODE_ALL = the
 *       all-candidates scan (candidate_limit ignored).
 *   pf_recommend_collab:  recommend_collaborative(u, topk, candidate_limit).
 *   pf_recommend_clubs:   recommend_clubs_collab(u, topk, candidate_limit)
 *       (ids are club ids).
 * Returns PF_OK even when some queries are unknown (their count is 0).
 */
int pf_recommend_interest(pf_ctx* ctx, const int32_t* query_uid, int32_t nq,
                          int32_t topk, int32_t mode, int32_t candidate_limit,
                          int32_t* out_uid, float* out_score, int32_t* out_count);
int pf_recommend_collab(pf_ctx* ctx, const int32_t* query_uid, int32_t nq,
                        int32_t topk, int32_t candidate_limit,
                        int32_t* out_uid, float* out_score, int32_t* out_count);
int pf_recommend_clubs(pf_ctx* ctx, const int32_t* query_uid, int32_t nq,
                       int32_t topk, int32_t candidate_limit,
                       int32_t* out_uid, float* out_score, int32_t* out_count);

/*
 * Asynchronous forms of the three job recommenders (interest in PF_MODE_FOF): the call plans the
 * batch on the host and queues its device stages on the context's stream, then returns; the
 * outputs (same layout as above) are written when pf_wait(ctx, ticket) returns, so the caller
 * keeps its buffers alive until then.  While call i runs on the device the host can plan call
 * i + 1: one context then keeps the GPU busy where the synchronous calls leave it idle during
 * planning (what several contexts per GPU were used for).  At most three calls are in flight: a
 * fourth waits for the oldest itself.  Any other call on the context (synchronous recommenders,
 * pf_set_adj, pf_jobs_stats_*) first completes the pending ones; pf_close drops them unwritten.
 * pf_wait(ticket) completes every call up to that ticket, in launch order; it returns the first
 * failure among them (PF_OK for a ticket already completed).
 */
int pf_recommend_interest_async(pf_ctx* ctx, const int32_t* query_uid, int32_t nq, int32_t topk,
                                int32_t candidate_limit, int32_t* out_uid, float* out_score,
                                int32_t* out_count, uint64_t* ticket);
int pf_recommend_collab_async(pf_ctx* ctx, const int32_t* query_uid, int32_t nq, int32_t topk,
                              int32_t candidate_limit, int32_t* out_uid, float* out_score,
                              int32_t* out_count, uint64_t* ticket);
int pf_recommend_clubs_async(pf_ctx* ctx, const int32_t* query_uid, int32_t nq, int32_t topk,
                             int32_t candidate_limit, int32_t* out_uid, float* out_score,
                             int32_t* out_count, uint64_t* ticket);
int pf_wait(pf_ctx* ctx, uint64_t ticket);
/* The highest ticket whose call has completed (its outputs written): every ticket <= it is
 * done, by pf_wait or by another call that completed the pending ones first.  0 when no
 * asynchronous call has completed (or ctx is NULL).  Bindings drop their references to a
 * call's output buffers once its ticket is <= this. */
uint64_t pf_completed_ticket(const pf_ctx* ctx);

/* Ordered, de-duplicated, limit-truncated 2-hop candidate list of uid
 * (flavour PF_FOF_GRAPH or PF_FOF_COLLAB).  Writes at most `cap` ids; *n gets
 * the full list length. */
int pf_fof_candidates(pf_ctx* ctx, int32_t uid, int32_t limit, int32_t flavour,
                      int32_t* out, int32_t cap, int32_t* n);

/* Replace adj_list[uid] (hold-out drivers mutate the adjacency between
 * queries: test.cpp:73, recommendation_tests.cpp:111-114).  n = -1 erases the
 * row (uid absent from adj_list). */
int pf_set_adj(pf_ctx* ctx, int32_t uid, const int32_t* nbrs, int32_t n);

/* Restrict the all-candidates scan to shard `shard` of `nshards`: contiguous
 * candidate ranges of equal stream bytes (K1 tiles) and of equal posting weight
 * (K5 blocks: a fixed share per candidate plus its tokens, clubs and friends);
 * the multi-GPU path merges the per-shard top-k. */
int pf_set_shard(pf_ctx* ctx, int32_t shard, int32_t nshards);

/* All-candidates scan kernel.  PF_SCAN_AUTO (default) takes the postings scan
 * (K5: per-token candidate lists, only the lists the query names are read) when the
 * corpus fits its encoding, else the record-stream scan (K1: every candidate's record
 * is walked).  Both give bit-identical results; forcing POSTINGS on a corpus outside
 * its encoding returns PF_EUNSUPP. */
#define PF_SCAN_AUTO     0
#define PF_SCAN_STREAM   1
#define PF_SCAN_POSTINGS 2
int pf_set_scan_kernel(pf_ctx* ctx, int32_t kind);

/*
 * Candidate filter of the all-candidates scans: only candidates that pass it are ranked ("the k
 * most similar women aged 20-29 of my region").  Context state like pf_set_shard; it applies to
 * pf_recommend_interest(PF_MODE_ALL) at any topk and to pf_scan_keys_async, on top of the query's
 * own exclusions (adj[q] + {q}), and to nothing else: FoF interest, collab, clubs, pf_fas_pairs,
 * pf_fof_candidates and the hold-out drivers never see it.  Every launch takes the filter by value
 * as it stands when the call is made, so asynchronous scans already queued keep theirs.  The
 * reference has no such call: with no filter set every result is what it was.
 * Values are compared in the domain the corpus was given in (ages as given to pf_open, that is
 * median-filled); a gender / public value no user has passes nobody.  A field is missing by FAS's
 * own rules (public / gender < 0, age / completion <= 0, a region part < 0); a candidate whose
 * tested field is missing fails that test unless PF_FILT_KEEP_MISSING is set.
 */
#define PF_FILT_GENDER 1u      /* candidate.gender == gender */
#define PF_FILT_PUBLIC 2u      /* candidate.public_flag == public_flag */
#define PF_FILT_AGE 4u         /* age_min <= age <= age_max (ages as given to pf_open: median-filled) */
#define PF_FILT_COMPLETION 8u  /* completion_min <= completion <= completion_max */
#define PF_FILT_REGION 16u     /* every region[i] >= 0 equals the candidate's part i; -1 = any */
#define PF_FILT_KEEP_MISSING 1u /* flags: a candidate whose tested field is missing passes that test */

typedef struct pf_cand_filter {
    uint32_t fields, flags;
    int32_t gender, public_flag;
    int32_t age_min, age_max;
    int32_t completion_min, completion_max;
    int32_t region[3], pad;
} pf_cand_filter;

/* NULL or fields == 0 clears.  PF_EINVAL: unknown bits in fields / flags, a min above its max,
 * PF_FILT_REGION with all three parts -1. */
int pf_set_scan_filter(pf_ctx* ctx, const pf_cand_filter* filter);
/* Candidates of this context's shard that pass the filter (all of them when none is set), the
 * query's exclusions not counted.  Synchronises the context's stream. */
int pf_scan_filter_count(pf_ctx* ctx, int64_t* n);

/*
 * Field selection of the all-candidates scans: "similar in what respect".  A selection is a set
 * of FAS's fixed fields (bit k of `fixed` = PF_F_*: public .. friends) and a set of text columns
 * (bit t of `cols` = column t of the engine's list).  FAS(A, B | selection) is
 * profile_similarity(A, B, the selected columns in ascending index) with every deselected fixed
 * field treated as missing on the query's side (public / gender < 0, age / completion = 0, all
 * region parts -1, an empty clubs / friends list: what the reference does for a user who left the
 * field empty).  Each selected column keeps its own idf map and normaliser, and everything
 * selected is computed bit for bit as without a selection.  The denominator is the reference's
 * own for that column list, 7 + (selected columns): deselecting a fixed field does not shrink the
 * 7.  Scores of scans with different selections are therefore NOT comparable with each other.
 * Ranking order, exclusions, the candidate filter and shards behave as without a selection.
 * Context state like the filter: read by pf_recommend_interest(PF_MODE_ALL) at any topk and by
 * pf_scan_keys_async, and by nothing else (FoF interest, collab, clubs, plain pf_fas_pairs,
 * pf_fof_candidates and the hold-out drivers never see it).  Every launch takes the selection by
 * value as it stands when the call is made, so asynchronous scans already queued keep theirs.  No
 * query image changes and no second engine is opened.
 */
#define PF_SEL_FIXED_ALL 0x7Fu
typedef struct pf_field_select {
    uint32_t fixed, flags;  /* fixed: bits above PF_SEL_FIXED_ALL are PF_EINVAL; flags: must be 0 */
    uint64_t cols;          /* bits at or above n_cols are ignored: ~0 = all columns */
} pf_field_select;
/* NULL, or a selection that leaves nothing out, clears.  PF_EINVAL: a NULL context, unknown bits
 * in fixed, a non-zero flags. */
int pf_set_scan_select(pf_ctx* ctx, const pf_field_select* select);
/* pf_fas_pairs under a selection (NULL = none), whatever the context's scan selection is. */
int pf_fas_pairs_select(pf_ctx* ctx, const int32_t* a_uid, const int32_t* b_uid, int64_t n,
                        const pf_field_select* select, float* out);

/*
 * Score breakdown: "similar because of what".  FAS is the harmonic mean of S, the average of the
 * per-field sigmoid terms profile_similarity adds to sum_Si (recommender_similarity.cpp:38-114),
 * and F, the share of the 7 + T fields both profiles filled in.  These calls return the terms.
 * A pair's row has PF_NUM_FIXED + T doubles, T = pf_num_cols(ctx): slot k < 7 is the fixed field
 * PF_F_*, slot 7 + t text column t of the engine's list.  A slot is present when the reference adds
 * its term (the field is filled in on both sides); the head's masks say which: bit k of `fixed` =
 * slot k, bit t of `cols` = slot 7 + t, the layout of pf_field_select.  A slot that is not present
 * holds 0.0.  score is the pair's FAS, formed from the row as the reference forms it: used = the
 * masks' popcount, S = (the present terms summed in ascending slot order) / used, F = used / (7 + T),
 * (float)(2SF / (S + F)); used == 0 scores 0.
 * Under a field selection a deselected slot is not present, T in F is the selected columns' count,
 * the row keeps the engine's width (slots do not move), and the term of a slot that stays selected
 * is the same double as with no selection.
 */
typedef struct pf_pair_terms_head {
    float    score;
    uint32_t fixed;
    uint64_t cols;
} pf_pair_terms_head; /* 16 B */
/* T, the engine's text columns (0 for a NULL context) */
int32_t pf_num_cols(const pf_ctx* ctx);
/* pf_fas_pairs_select with the breakdown: head[n], terms[n * (PF_NUM_FIXED + T)].  A pair with an
 * unknown uid gets score NaN, both masks 0 and a row of 0.0.  select NULL = none; the context's scan
 * selection plays no part. */
int pf_fas_pairs_terms(pf_ctx* ctx, const int32_t* a_uid, const int32_t* b_uid, int64_t n,
                       const pf_field_select* select, pf_pair_terms_head* head, double* terms);
/* pf_recommend_interest(ctx, query_uid, nq, topk, PF_MODE_ALL, 0, ...) with the breakdown of every
 * result: the same scan (the context's filter, selection, kernel choice and shard; the job pipeline
 * for topk > 64), whose ids and scores are returned as they are, then one more launch over the
 * (query, result) pairs under the context's selection.  Result j of query i has head[i * topk + j]
 * and the row terms[(i * topk + j) * (PF_NUM_FIXED + T)]; entries at or past out_count[i] are not
 * written. */
int pf_recommend_interest_all_terms(pf_ctx* ctx, const int32_t* query_uid, int32_t nq, int32_t topk,
                                    int32_t* out_uid, float* out_score, int32_t* out_count,
                                    pf_pair_terms_head* head, double* terms);

/*
 * Query by profile: "for whom", when that person is not a user of the corpus given to pf_open (a
 * sign-up form, a profile being edited, an anonymous search, a record of another dataset).  The
 * profile is given by value; nothing of it is stored.
 *   Definition   The score of candidate B is profile_similarity(A, B) of the reference with A the given
 *                profile: bit for bit what the reference returns for a corpus that also holds A, under
 *                the same idf map and normalisers.
 *   idf          The engine's, fixed at open: the visitor counts in neither N nor df.  A token id the
 *                column's idf map does not hold gets 1.0 (pf_idf's rule, recommender.cpp:78), ids above
 *                every id the engine has seen included; a column with no idf map uses raw counts.  A
 *                query token no candidate holds meets nobody, but adds to the column's norm and keeps
 *                the column non-empty: a candidate with that column filled gets the s = 0 term there.
 *   Norm         Per column sqrt(sum ((double)tf * idf)^2) over the row in ascending token-id order, the
 *                order and the arithmetic of the stored users' rows.
 *   Codes        A public_flag / gender value no corpus user has is present and equal to nobody (not
 *                missing: the term is added, at s = 0).  An age / completion no user has gets its
 *                sigmoid row computed on the host like any stored value; values past 128 behave as
 *                they do for stored users.
 *   Exclusions   Exactly exclude_uid: no implicit self, no adjacency.  Unknown uids are ignored.
 *   State        The context's filter, field selection, shard and scan-kernel choice apply exactly as
 *                to pf_recommend_interest(PF_MODE_ALL); the `select` argument of the pair calls behaves
 *                as in pf_fas_pairs_select / pf_fas_pairs_terms.
 *   Batches      The nq profiles are one call: nq == 1 runs the one-query scan (its image uploaded with
 *                the launch), nq > 1 the batch scan over the staged images.
 *   Limits       topk > 64 returns PF_EUNSUPP (the job pipeline serves stored users only).  A row
 *                pf_open would not accept for a user is refused, never scored wrongly: PF_EUNSUPP for a
 *                club / friend id repeated more than 255 times, more than 65535 clubs or friends, a tf
 *                outside the record encoding (0..255 in the packed layout); PF_EINVAL for a negative
 *                token id, an id repeated within a column, a non-monotone tok_off, non-zero flags, a
 *                NULL profile array with nq > 0.  pf_last_error names the reason.
 *   No change    Nothing in the context changes: no resident image, store or idf is touched, and the
 *                by-uid calls before and after are identical.
 */
typedef struct pf_query_profile {
    int32_t public_flag, gender;      /* -1 = missing                                  */
    int32_t completion, age;          /* used when > 0; age in the corpus's domain     */
    int32_t region[3];                /* -1 = missing part                             */
    uint32_t flags;                   /* must be 0                                     */
    const uint32_t* club_ids;   int32_t n_clubs;    /* profile order, duplicates kept  */
    const uint32_t* friend_ids; int32_t n_friends;  /* the profile's `friends` column  */
    const int64_t* tok_off;           /* [T + 1], T = pf_num_cols(ctx); NULL = no text */
    const int32_t* tok_tid;           /* distinct within a column, >= 0                */
    const int32_t* tok_tf;
    const int32_t* exclude_uid; int32_t n_exclude;  /* never returned; unknown uids ignored */
} pf_query_profile;

/* The all-candidates top-k of each of the nq profiles; outputs as pf_recommend_interest.  nq = 0
 * returns PF_OK and writes nothing. */
int pf_recommend_interest_profile(pf_ctx* ctx, const pf_query_profile* q, int32_t nq, int32_t topk,
                                  int32_t* out_uid, float* out_score, int32_t* out_count);
/* FAS(A = the profile, B = b_uid[i]) for n stored users; an unknown b_uid scores NaN. */
int pf_fas_profile_pairs(pf_ctx* ctx, const pf_query_profile* a, const int32_t* b_uid, int64_t n,
                         const pf_field_select* select, float* out);
/* ... with the breakdown, laid out as pf_fas_pairs_terms */
int pf_fas_profile_pairs_terms(pf_ctx* ctx, const pf_query_profile* a, const int32_t* b_uid, int64_t n,
                               const pf_field_select* select, pf_pair_terms_head* head, double* terms);
/* pf_recommend_interest_profile with the breakdown of every result, laid out as
 * pf_recommend_interest_all_terms (the context's selection) */
int pf_recommend_interest_profile_terms(pf_ctx* ctx, const pf_query_profile* q, int32_t nq, int32_t topk,
                                        int32_t* out_uid, float* out_score, int32_t* out_count,
                                        pf_pair_terms_head* head, double* terms);

/*
 * Group query: "who is similar to THESE people" (the members of a club, a user's friends, a seed
 * audience).  Every candidate is scored against every seed and the scores are combined per candidate.
 *   Seeds        Stored users.  Unknown uids are dropped; of a repeated uid the first occurrence
 *                counts; G is the number that remain, in the caller's order.  G = 0 gives count 0 and
 *                PF_OK, as an unknown query uid does.
 *   Per seed     s_g(B) is the float profile_similarity(seed_g, B) of the reference, bit for bit what
 *                the all-candidates scan and the pair kernel compute, under the context's field
 *                selection (pf_set_scan_select) exactly as PF_MODE_ALL.
 *   Aggregate    PF_GROUP_MEAN: double acc = 0; acc += (double)s_g for g = 0 .. G-1 in that order;
 *                score = (float)(acc / (double)G).  PF_GROUP_MIN / PF_GROUP_MAX: m = s_0, then for
 *                g = 1 .. G-1 in order m = s_g < m ? s_g : m (MAX: s_g > m).  With G = 1 all three
 *                return s_0 itself.
 *   Candidates   A stored user of the context's shard (pf_set_shard) that passes the context's
 *                candidate filter, is not a seed, is not in exclude_uid and, under
 *                PF_GROUP_EXCLUDE_ADJ, is in no seed's current adj_list row (pf_set_adj is honoured).
 *                With the flag off a candidate in adj[seed] is scored against that seed like anyone
 *                else.  Results are ranked (score desc, uid asc).
 *   State        The filter and the selection travel by value with the launches; nothing in the
 *                context changes, and the by-uid calls before and after are identical.
 *   Refusals     PF_EINVAL: n_seeds > PF_GROUP_MAX_SEEDS, a negative count, an unknown agg, unknown
 *                flag bits, a NULL array with a positive count.  PF_EUNSUPP: topk > 64; an exclusion
 *                union (the kept seeds + the known uids of exclude_uid + under PF_GROUP_EXCLUDE_ADJ
 *                the seeds' adj_list rows, distinct) of more than PF_GROUP_MAX_EXCLUDE uids: the
 *                union rides in one query image's exclusion table, a cuckoo table of at most 2^16
 *                slots filled to 0.4.  pf_last_error names the reason.
 *   Groups       The ng groups are independent and run one after the other.
 * The scan (fas_group_kernel) packs the seeds' query images, in order, into
 * passes of as many images as fit one workgroup's LDS budget and reads the shard's record stream
 * once per pass; pf_group_plan_of reports the packing.
 */
#define PF_GROUP_MEAN 0
#define PF_GROUP_MIN  1      /* similar to every seed  */
#define PF_GROUP_MAX  2      /* similar to any seed    */
#define PF_GROUP_EXCLUDE_ADJ 1u   /* flags: also drop adj[s] of every seed s */
#define PF_GROUP_MAX_SEEDS 1024
#define PF_GROUP_MAX_EXCLUDE 26214  /* floor(0.4 * 2^16) */

typedef struct pf_group_query {
    const int32_t* seed_uid;    int32_t n_seeds;
    int32_t  agg;               uint32_t flags;
    const int32_t* exclude_uid; int32_t n_exclude;  /* never returned; unknown uids ignored */
} pf_group_query;

/* The top-k of each of the ng groups; outputs as pf_recommend_interest (row i of out_uid /
 * out_score has topk entries, out_count[i] of them written).  ng = 0 returns PF_OK. */
int pf_recommend_group(pf_ctx* ctx, const pf_group_query* g, int32_t ng, int32_t topk,
                       int32_t* out_uid, float* out_score, int32_t* out_count);
/* The aggregate of one group for n listed users (NaN for an unknown b_uid, and for every user when
 * G = 0), under `select` (NULL = none, as pf_fas_pairs_select; the context's selection plays no
 * part).  No filter and no exclusion applies: a seed is scored like anyone else.  Computed by the
 * pair kernel (G x n pairs, in chunks) and aggregated on the host: a second route to the scan's
 * numbers ("how well does this user fit the club"). */
int pf_group_scores(pf_ctx* ctx, const pf_group_query* g, const int32_t* b_uid, int64_t n,
                    const pf_field_select* select, float* out);
/* What pf_recommend_group would launch for the group: the G kept seeds, the passes over the record
 * stream, the images probed in global memory (tables above the LDS staging limit), and the bytes
 * read: n_passes x the shard's record stream and 48-B headers (pf_scan_bytes' K1 figure). */
typedef struct pf_group_plan { int32_t n_seeds, n_passes, n_global, pad; int64_t stream_bytes; } pf_group_plan;
int pf_group_plan_of(pf_ctx* ctx, const pf_group_query* g, pf_group_plan* out);
/* LDS bytes image i of the group's G kept seeds takes in a pass (out[G]: constants + staged
 * tables, the constants alone for an image probed in global memory), then out[G] = the bytes a
 * pass takes besides its images and out[G + 1] = the LDS budget of a pass; cap >= G + 2 entries.
 * A pass is the longest prefix of the remaining seeds whose sum fits the budget (at least one,
 * at most PF_DEBUG group_tile=N). */
int pf_group_image_lds(pf_ctx* ctx, const pf_group_query* g, int32_t* out, int32_t cap);

/*
 * Score window of the all-candidates scans: a floor ("at least this similar"), a paging cursor ("load
 * more") and a match count ("how many").  A window restricts which candidates are RANKED; every score
 * is computed bit for bit as without one.
 *   The test     A candidate is in the window when it is rankable as without one (in the shard, passing
 *                the filter, not excluded) and
 *                  under PF_WIN_MIN   its float score is >= min_score;
 *                  under PF_WIN_AFTER it ranks strictly after the cursor in the engine's order: score <
 *                                     after_score, or score == after_score and uid > after_uid (signed).
 *                The cursor is a position, not a member: after_uid need not be a stored user and
 *                after_score need not be anybody's score.  -0.0 is 0.0, as in the ranking.
 *   Results      The window's first topk in (score desc, uid asc); out_count < topk means the window is
 *                exhausted.
 *   Paging       Page n + 1 is the same call with after_* set to page n's last result; the pages
 *                concatenated equal the unwindowed ranking.  This holds for profile and group queries
 *                too, whose topk stops at 64: the cursor takes them to any depth.
 *   State        Context state like the filter and the selection; it travels by value with every launch,
 *                so asynchronous scans already queued keep theirs.  Read by
 *                pf_recommend_interest(PF_MODE_ALL), pf_recommend_interest_profile, pf_recommend_group,
 *                their _terms forms and pf_scan_keys_async, and by nothing else: FoF interest, collab,
 *                clubs, the pair calls, pf_group_scores and the hold-out drivers never see it.  One
 *                window serves all nq queries of a call (a floor and a count suit batches; a cursor is
 *                meant for nq == 1 but is legal for any).  No query image, resident image or store
 *                changes; with none set every result and every launch is what it was.
 *   Count        Under PF_WIN_COUNT a synchronous scan call also stores, per query, the number of
 *                candidates of this context's shard in the window, whatever topk > 0 is (topk = 0 scans
 *                nothing and stores no count).
 *                pf_scan_window_totals returns the last such call's values (*n = that call's nq; at most
 *                cap are written); a value is 0 for an unknown uid and for a group with G = 0.
 *                PF_EINVAL when no counted call has run.  Sharded callers sum the per-shard values.
 *   The floor    seeds the postings scan's pruning threshold (it is valid before the first block), so a
 *                floored scan begins no block cold and is, if anything, cheaper than the unwindowed one.
 *                A counted scan holds the threshold at the floor and prunes no further.
 *   Refusals     PF_EINVAL: unknown bits in fields, non-zero flags, a NaN score under its bit; the window
 *                in force is left alone.  PF_EUNSUPP (pf_last_error names the reason): a window in force
 *                with topk > 64 on PF_MODE_ALL (the job pipeline does not read it: the cursor is the way
 *                deep), PF_WIN_COUNT with pf_scan_keys_async.  min_score <= 0 passes everybody and
 *                min_score > 1 may pass nobody; neither is an error.
 */
#define PF_WIN_MIN   1u   /* min_score holds */
#define PF_WIN_AFTER 2u   /* after_score / after_uid hold */
#define PF_WIN_COUNT 4u   /* also count the candidates in the window */
typedef struct pf_scan_window {
    uint32_t fields, flags;          /* flags must be 0 */
    float    min_score, after_score;
    int32_t  after_uid, pad;
} pf_scan_window; /* 24 B */
/* NULL or fields == 0 clears. */
int pf_set_scan_window(pf_ctx* ctx, const pf_scan_window* window);
int pf_scan_window_totals(pf_ctx* ctx, int64_t* out, int32_t cap, int32_t* n);

/*
 * Collect: every candidate of the score window in one pass.  With a collector in force a scan call
 * also keeps the whole set PF_WIN_COUNT counts, ranked, next to its own top-k: the look-alike audience
 * of a group, the near-duplicates of a profile, everyone above a floor inside a filter, in one scan
 * plus one sort of the matches instead of one scan per 64 results.
 *   Which calls  The synchronous pf_recommend_interest under PF_MODE_ALL with topk <= 64,
 *                pf_recommend_interest_profile, pf_recommend_group and their _terms forms, with nq (ng)
 *                == 1 and topk > 0 (topk = 0 scans nothing and collects nothing).  Refused with
 *                PF_EUNSUPP (pf_last_error says "collect"): nq or ng above 1, pf_scan_keys_async, topk >
 *                64 on PF_MODE_ALL.  FoF interest, collab, clubs, the pair calls, pf_group_scores and the
 *                hold-out drivers never see it.
 *   The set      Exactly the candidates PF_WIN_COUNT counts: in the shard, passing the filter, not
 *                excluded, in the window in force; with no window every rankable candidate.  Each comes
 *                with its uid and its float score, bit for bit what the top-k reports.
 *   Order        (score desc, uid asc): the first out_count entries are the call's own top-k, and the
 *                whole list is the cursor's pages concatenated.
 *   Overflow     total > cap is no error: *total is exact, *n = 0 and nothing is written; raise the floor
 *                or the cap (a counted call tells the size in advance).  No store ever goes past cap keys.
 *   Pruning      A collecting scan holds the postings scan's threshold at the window's seed, as a counted
 *                one does (no floor: no pruning).
 *   Unchanged    The call's own ids, scores and out_count, and pf_scan_window_totals under PF_WIN_COUNT,
 *                are what they are without a collector (a collecting call the caller did not ask a count
 *                of leaves the stored totals alone).  With no collector every result and launch is what
 *                it was.
 *   Empty        An unknown uid and a group with G = 0 give total = 0.  Under pf_set_shard the result is
 *                the shard's; the shards' lists merged by (score desc, uid asc) are the unsharded list.
 *   State        Context state like the filter, the selection and the window; the buffer and its cap
 *                travel by value with the launch.  pf_scan_bytes ignores it.
 */
/* cap > 0: collect into a buffer of cap keys; 0 clears.
 * PF_EINVAL: cap < 0 or cap > INT32_MAX.
 * PF_ENOMEM: the device buffer (8 B per key) cannot be had; the collector in force is left alone. */
int pf_set_scan_collect(pf_ctx* ctx, int64_t cap);
/* The last collecting call's result: *total = the candidates in the window; *n = the number written
 * (total when total <= the collector's cap, else 0); at most out_cap entries are written to out_uid /
 * out_score, ranked (score desc, uid asc).  PF_EINVAL when no collecting call has run. */
int pf_scan_collected(pf_ctx* ctx, int32_t* out_uid, float* out_score, int64_t out_cap, int64_t* n, int64_t* total);

/*
 * Clubs by interest: club recommendations from a scan's neighbours ("which clubs", for a stored user,
 * a profile given by value or a seed audience).  pf_recommend_clubs walks the adj_list; these calls
 * need none: a user without an adj_list row, a profile that is not in the corpus and a group all get
 * clubs.  The definition is recommender_clubs.cpp:30-44 and :66-72 (its phase 1) with "friends"
 * replaced by "neighbours"; there is no reference function.
 *   Neighbours   The candidates a collecting scan of the query collects ("Collect", "The set"): in the
 *                shard, passing the context's filter, not excluded, inside `window`, ranked (score
 *                desc, uid asc) as float scores under the context's field selection; for a group the
 *                score is the group's aggregate.  With neighbours = M > 0 only the first M of that
 *                ranking are used.
 *   Own clubs    A stored user's clubs; a profile's club_ids; the union of a group's kept seeds' clubs.
 *                Not scored unless PF_CLUBS_KEEP_OWN is set.
 *   A score      double acc = 0; the neighbours in rank order, each with w = (double)score, skipped
 *                when w <= 0.0; its club list in profile order, acc += w for every occurrence of the
 *                club (a repeated club counts as often as it is listed).  The score is (float)acc.
 *                The order of the adds is part of the contract.
 *   The list     The clubs with at least one contribution as (club id, score), ordered (score desc,
 *                club id asc), cut to topk (any topk >= 0; topk = 0 scans nothing and reports zeros).
 *   info         total = the candidates in the window (exact, whatever cap is); used = the neighbours
 *                that entered (min(M, total), or total); contributions = the adds made; clubs = the
 *                clubs with at least one.  NULL is allowed.
 *   Overflow     total > cap is no error: out_count = 0, info.total is exact and used = 0.
 *   Empty        An unknown uid, a group with G = 0 and an empty window give out_count = 0.
 *   State        The calls run the scan with a collector of `cap` keys and a counted window of their
 *                own for their duration and give the context's window, collector, stored totals and
 *                pf_scan_collected result back exactly as they found them.  The filter and selection
 *                in force apply as they do to the scan.
 *   Refusals     PF_EINVAL: a NULL context, query or out_count; NULL outputs with topk > 0; topk < 0;
 *                cap <= 0 or above INT32_MAX; neighbours < 0; unknown bits in flags; a window the
 *                window setter would refuse; what the profile or group call underneath refuses.
 *                PF_EUNSUPP: a context sharded by pf_set_shard into more than one shard (partial sums
 *                of shards cannot be merged in rank order); more than INT32_MAX contributions; what
 *                the call underneath refuses.  PF_ENOMEM: a device buffer cannot be had.
 */
#define PF_CLUBS_KEEP_OWN 1u
typedef struct pf_clubs_query {
    int64_t  cap;          /* most candidates the window may hold; > 0, <= INT32_MAX            */
    int32_t  neighbours;   /* M: the first M of the ranking enter; 0 = the whole window          */
    uint32_t flags;
    const pf_scan_window* window;   /* NULL = no window (every rankable candidate)               */
} pf_clubs_query;
typedef struct pf_clubs_info { int64_t total, used, contributions, clubs; } pf_clubs_info;

int pf_recommend_clubs_interest(pf_ctx* ctx, int32_t uid, const pf_clubs_query* q, int32_t topk,
                                int32_t* out_club, float* out_score, int32_t* out_count, pf_clubs_info* info);
int pf_recommend_clubs_profile(pf_ctx* ctx, const pf_query_profile* profile, const pf_clubs_query* q, int32_t topk,
                               int32_t* out_club, float* out_score, int32_t* out_count, pf_clubs_info* info);
int pf_recommend_clubs_group(pf_ctx* ctx, const pf_group_query* group, const pf_clubs_query* q, int32_t topk,
                             int32_t* out_club, float* out_score, int32_t* out_count, pf_clubs_info* info);

/*
 * Diverse top-k: a ranked list re-ranked by maximal marginal relevance, so that a first page is not
 * ten copies of one person.  There is no reference function; this is the definition.
 *   Pool         M users p_0 .. p_{M-1} in a fixed order, each with a float relevance r_i.  Position
 *                is part of the contract: it breaks ties.
 *   Similarity   sim(s, i) is the float pf_fas_pairs_select gives for a = p_s, b = p_i under the
 *                selection named below: the picked user is on the A side (FAS is symmetric in exact
 *                arithmetic, not in floats).
 *   Penalty      pen_i is a float, 0.0f before the first pick; after each pick s,
 *                pen_i = sim(s, i) > pen_i ? sim(s, i) : pen_i.
 *   Value        v_i is a double from three separately rounded IEEE operations, never fused:
 *                a = (double)lambda * (double)r_i (exact); p = (1.0 - (double)lambda) * (double)pen_i
 *                (the subtraction rounds once, the product once); v_i = a - p (rounds once).
 *   A pick       Among the unpicked i the largest v_i; ties go to the smallest position.  Repeated
 *                min(topk, M) times.
 *   Outputs      Per pick, in pick order: out_uid, out_score = r (untouched), out_pen = the float
 *                penalty at the moment of the pick (0 for the first), out_value = the double v.
 *                out_pen and out_value may be NULL.
 *   lambda       A float in [0, 1].  1: the pool's first topk.  0: position 0, then the users least
 *                similar to anything picked so far.
 *   Limits       M <= PF_DIVERSE_MAX_POOL.  Any topk >= 0; topk = 0 scans nothing and reports zeros.
 * pf_diverse_rerank diversifies a list the caller holds (a FoF result, a collaborative result, a
 * collected window): the pool is the caller's order; unknown uids are dropped; of a repeated uid the
 * first occurrence counts; `select` (NULL = none) is the selection of the similarities, and the
 * context's selection plays no part.  PF_EINVAL: a NULL context or out_count, n < 0, a NULL list with
 * n > 0, NULL out_uid / out_score with topk > 0, topk < 0, lambda outside [0, 1] or NaN, a NaN or
 * infinite relevance (an infinity times a zero weight has no value to rank), unknown selection bits.  PF_EUNSUPP: more than PF_DIVERSE_MAX_POOL known, distinct entries.
 * The three scan calls take the pool from the collecting scan of the query, run as the clubs calls
 * above run it ("Neighbours", "State"): the candidates inside `window`, passing the context's filter,
 * ranked (score desc, uid asc) under the context's field selection (a group's score is its
 * aggregate); the pool is the first min(pool, total) of that ranking, r their scores, and the
 * similarities are scored under the same selection.  The context's window, collector, stored totals
 * and pf_scan_collected result come back as they were found.
 *   info         total = the candidates in the window (exact, whatever cap is); pool = M; pairs = the
 *                pairs scored for the similarities, M * M (the whole matrix, the diagonal included,
 *                in one launch; the rows never picked are the price of that); picked = out_count.
 *                NULL is allowed.
 *   Overflow     total > cap is no error: out_count = 0, info.total is exact, pool = picked = 0.
 *   Empty        An unknown uid, a group with G = 0 and an empty window give out_count = 0.
 *   Refusals     PF_EINVAL: a NULL context, query or out_count; NULL out_uid / out_score with
 *                topk > 0; topk < 0; cap <= 0 or above INT32_MAX; pool < 1; lambda outside [0, 1] or
 *                NaN; a window the window setter would refuse; what the call underneath refuses.
 *                PF_EUNSUPP: pool > PF_DIVERSE_MAX_POOL; a context sharded into more than one shard.
 *                PF_ENOMEM: a device buffer cannot be had.
 */
#define PF_DIVERSE_MAX_POOL 1024
typedef struct pf_diverse_query {
    int64_t  cap;        /* most candidates the window may hold; > 0, <= INT32_MAX       */
    int32_t  pool;       /* M: the first M of the ranking are the pool; 1 .. 1024        */
    float    lambda;     /* in [0, 1]                                                    */
    const pf_scan_window* window;   /* NULL = every rankable candidate                   */
} pf_diverse_query;
typedef struct pf_diverse_info { int64_t total, pool, pairs, picked; } pf_diverse_info;

int pf_diverse_rerank(pf_ctx* ctx, const int32_t* uid, const float* score, int64_t n, float lambda, int32_t topk,
                      const pf_field_select* select, int32_t* out_uid, float* out_score, float* out_pen,
                      double* out_value, int32_t* out_count);
int pf_recommend_diverse_interest(pf_ctx* ctx, int32_t uid, const pf_diverse_query* q, int32_t topk, int32_t* out_uid,
                                  float* out_score, float* out_pen, double* out_value, int32_t* out_count,
                                  pf_diverse_info* info);
int pf_recommend_diverse_profile(pf_ctx* ctx, const pf_query_profile* profile, const pf_diverse_query* q, int32_t topk,
                                 int32_t* out_uid, float* out_score, float* out_pen, double* out_value,
                                 int32_t* out_count, pf_diverse_info* info);
int pf_recommend_diverse_group(pf_ctx* ctx, const pf_group_query* group, const pf_diverse_query* q, int32_t topk,
                               int32_t* out_uid, float* out_score, float* out_pen, double* out_value,
                               int32_t* out_count, pf_diverse_info* info);

/*
 * Device-resident all-candidates scan for the multi-GPU bench: scores the
 * queries against this context's shard and writes, per query, `topk` packed
 * 64-bit keys to DEVICE memory d_keys[nq*topk] on `stream` (a hipStream_t).
 * Key = (~orderable(score) << 32) | (uid ^
 * 0x80000000): ascending key = (score desc, uid asc); unused slots are
 * UINT64_MAX.  `stream` is used as given (NULL = the HIP null stream, not the
 * context's stream), so the caller's collectives on that stream are ordered
 * after the scan.  No host synchronisation.
 * The context's device workspaces (query images, partial keys, rendezvous
 * tickets) are shared by every call on it: all calls on one context must be
 * serialised on ONE stream (the context's own calls use its internal stream and
 * synchronise before returning, so mixing them with this call is safe only after
 * the caller has synchronised `stream`).
 * nq = 1 on a stream other than the context's runs on the context's scan lanes:
 * the launch goes to the next lane's stream (the context's stream and its two aux
 * streams in turn; seven eighths of a resident round of workgroups each) without waiting for work the caller queued on `stream`
 * earlier, and `stream` waits for it and copies its row into d_keys, in call
 * order; so consecutive single-query calls overlap on the device.  A single
 * query whose resident postings image is current (built at pf_open; a
 * pf_set_adj of that user makes it stale) builds and uploads nothing: one
 * launch, one wait, one row copy.
 */
int pf_scan_keys_async(pf_ctx* ctx, const int32_t* query_uid, int32_t nq,
                       int32_t topk, uint64_t* d_keys, void* stream);
/* Merge nparts key lists laid out [part][nq][topk] (device) into d_out[nq][topk]
 * on `stream` (as given, NULL = null stream). */
int pf_merge_keys_async(pf_ctx* ctx, const uint64_t* d_parts, int32_t nparts,
                        int32_t nq, int32_t topk, uint64_t* d_out, void* stream);
/* Host-side decode of packed keys; count = number of non-empty keys. */
void pf_decode_keys(const uint64_t* keys, int32_t n, int32_t* out_uid,
                    float* out_score, int32_t* count);

/* Statistics of the device layout (for roofline accounting). */
typedef struct pf_layout_stats {
    int64_t n_slots;          /* candidates in the tile store                  */
    int64_t stream_bytes;     /* bytes of the interleaved record stream        */
    int64_t header_bytes;     /* bytes of the fixed per-candidate headers      */
    int64_t alg_bytes;        /* sum 32+4|clubs|+4|friends|+8nnz */
    int32_t packed_tokens;    /* 1 if tokens are stored as one word            */
    int32_t n_tiles;
    int64_t post_bytes;       /* postings store: entries + norms + cells + headers (0 if absent) */
    int32_t scan_kernel;      /* kernel the next all-candidates scan uses: PF_SCAN_STREAM / PF_SCAN_POSTINGS */
    int32_t resident_images;  /* 1 if every user's pair image was built at pf_open and kept (0: built per call) */
    int64_t shard_cands;      /* candidates in this context's shard (pf_set_shard) for that kernel */
    int64_t shard_entries;    /* their postings entries (tokens, clubs, friends; 0 without postings) */
} pf_layout_stats;
int pf_layout(const pf_ctx* ctx, pf_layout_stats* out);

/* Bytes the all-candidates scan kernel reads from device memory for each query
 * over this context's shard, by the kernel's access pattern (the physical byte
 * model of DESIGN.md section 4): K5 = per candidate block, the 32-B headers, two
 * cell words per query list and every entry of each list's cell range (4 B;
 * token entries also their 8-B norm), the exclusion list, and the staged query
 * image per workgroup; K1 = the shard's record stream and headers.  0 for an
 * unknown uid.  The nq queries are taken as ONE launch, as pf_recommend_interest
 * runs them: nq = 1 is the single-query scan (one resident round of workgroups,
 * each staging the image once); nq > 1 a batch (each workgroup stages its query's
 * image once for its four blocks).  The candidate filter (pf_set_scan_filter) is ignored: the
 * bytes are those of the unfiltered scan (a filtered one reads the same headers and ranges and
 * skips the list entries of the blocks in which nobody passes).  The field selection
 * (pf_set_scan_select) is ignored as well: the bytes are those of the unselected scan (a selected
 * one reads no entry of a deselected column's or set's lists).  The score window (pf_set_scan_window)
 * is ignored too: the bytes are those of the unwindowed scan (a floored one skips the list entries of
 * the candidates its seeded threshold drops). */
int pf_scan_bytes(pf_ctx* ctx, const int32_t* query_uid, int32_t nq, int64_t* out_bytes);
/* Counters of the postings scan's pruning, summed over the postings scans of this process
 * (one-query launches and batches) since the last reset while PF_DEBUG k5_prune_stats=1 is set (zeros otherwise): out[5] =
 * candidates seen, candidates dropped at a block's start, dropped at a round's end, blocks,
 * blocks begun before the query had a threshold.  A candidate the scan filter drops counts as seen and
 * in neither dropped counter.  Synchronises the device. */
int pf_scan_prune_stats(pf_ctx* ctx, int64_t* out, int32_t reset);

/* Statistics of the recommenders' device job pipeline (pf_recommend_collab / _clubs /
 * _interest FoF and the batched drivers) since pf_jobs_stats_reset(ctx, 1): jobs run,
 * candidate-list entries scored, FAS pairs scored by the pair kernel (K1'), their
 * SURVEY 8(d) D3 bytes (b_c of each pair's candidate), the bytes the pair-scoring stage
 * reads for them by access pattern (pair_record_bytes: the 48-B headers + the record words
 * of every pair's candidate), the staged query-image bytes (one image per 512-pair block),
 * and the pair-scoring stage's device time (HIP events around K1' in each launch) and
 * launch count.  enable: bit 0 = time the pair kernel (HIP events around each
 * launch), bit 1 = count pairs and bytes (one extra small kernel per launch); 0 stops
 * both.  Fields of a part that is off read 0.  pair_dispatches: every pair-kernel (K1')
 * dispatch since pf_open (the job pipeline's stages, up to three per stage by image LDS
 * class, and pf_fas_pairs), never reset, so a profiler's per-dispatch rows can be grouped
 * into the calls they belong to. */
typedef struct pf_jobs_stats {
    int64_t jobs, candidates, pairs;
    int64_t pair_alg_bytes, pair_record_bytes, pair_image_bytes;
    double  pair_ms;
    int64_t pair_launches;
    int64_t pair_dispatches;
} pf_jobs_stats;
int pf_jobs_stats_reset(pf_ctx* ctx, int32_t enable);
int pf_jobs_stats_read(pf_ctx* ctx, pf_jobs_stats* out);

/* Device time (ms) of the last all-candidates scan kernel (HIP events on the
 * stream it was launched on). */
float pf_last_scan_ms(const pf_ctx* ctx);
/* Per-launch timing of the scan kernel over a region: reset, run, then read the
 * summed device time of every scan launch since the reset (synchronises). */
int pf_profile_reset(pf_ctx* ctx);
int pf_profile_read(pf_ctx* ctx, double* total_ms, int64_t* launches);
/* Time only scan launches 0, every, 2*every, ... after a reset (default 1 = all); the
 * others run without timing events.  *launches in pf_profile_read counts timed launches.
 * every = 0 turns profiling off (until the next pf_profile_reset).  At most 65536 launches
 * are timed per reset; later ones run untimed. */
int pf_profile_sample(pf_ctx* ctx, int32_t every);

#ifdef __cplusplus
}
#endif
#endif /* POKEC_FAS_H */
