/* place_recognition.h — C ABI of libpr_amd.so, the MI355X (gfx950) implementation of the
 * so_dso_place_recognition hot path: generate_signatures (Scan-Context + M2DP) and match_signatures.
 *
 * The reference has no FFI; its boundary is two C++ classes, two executables and three MATLAB functions
 * (SURVEY.md §8-b).  Every entry point below names the reference interface it replaces (file:line under
 * /root/reference/place_recognition/).  Conventions: flat arrays, caller-owned buffers, int status
 * (0 = PR_OK, <0 = error, text via pr_last_error), no exceptions across the boundary, one host thread per
 * context, one HIP device + one HIP stream per context.  There is NO CPU fallback: every call fails with
 * PR_EHIP when no gfx950 device is usable.
 */
#ifndef PLACE_RECOGNITION_H
#define PLACE_RECOGNITION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pr_ctx pr_ctx;
typedef struct pr_sigset pr_sigset;
typedef struct pr_clouds pr_clouds;
typedef struct pr_bow_vocab pr_bow_vocab;
typedef struct pr_bow_db pr_bow_db;

enum { PR_OK = 0, PR_EINVAL = -1, PR_ENOMEM = -2, PR_EHIP = -3, PR_EIO = -4, PR_ENAN = -5 };
enum { PR_TYPE_SC = 0, PR_TYPE_M2DP = 1, PR_TYPE_DELIGHT = 2, PR_TYPE_GIST = 3, PR_TYPE_BOW = 4 };   /* run_test.m:26-36 `type` */
enum { PR_ROLE_QUERY = 0, PR_ROLE_DB = 1 };         /* hist1 / hist2 of run_test.m:1 */
enum { PR_F64 = 0, PR_F32 = 1, PR_U8 = 2 };   /* PR_U8: 8-bit images (pr_gist_generate*) */
enum { PR_HOST = 0, PR_DEVICE = 1 };
/* arithmetic of the SC and M2DP matchers (processSC.m:22-33, processM2DP.m:12-22 on the GPU): split-f16 (fp32 operands carried
 * as f16 hi + lo, three f16 MFMAs per product, fp32 accumulate; default, 2-3x faster, same 1e-7 error as fp32), plain fp32 MFMA, or
 * PR_SC_ARITH_F16 = BASELINE.json config 5's "fp16 descriptors": spectra / rows stored as ONE f16 (2976 B per SC entry and channel),
 * one f16 MFMA per product, fp32 accumulate.  No reference counterpart (run_test.m handles fp64 only).  Its all-pairs distances are
 * within PR_F16_DISTANCE_BOUND of the exact ones (worst case; ~1.3e-4 observed; SURVEY.md asks for 1e-3 on typical data); the top-k
 * calls keep EXACT indices: the k + 56 best of the f16 pass are re-evaluated in fp64, and a query whose candidate list does not provably
 * contain the exact top-k, or whose re-evaluated candidates could change places under the sigma error of the f16 pass (pr_f16_margin_dev),
 * is recomputed in split-f16 (host calls: automatically, PR_WARN_F16_FALLBACK is raised) */
#define PR_F16_DISTANCE_BOUND 2e-3   /* |d_f16 - d| per channel: 8 u (u = 2^-11) on the correlation of unit-norm rows, halved */
/* Order check: the relative error allowed for a row sigma of the all-pairs pass is eps = SIGMA_REL + DIST_ERR / sigma.  SIGMA_REL: the
 * systematic part (the minimum over 120 noisy variants compresses a row by 2.5e-7 relative in the fp32-grade passes, whatever the row length).
 * DIST_ERR: the largest error of a single distance - |sigma(d + e) - sigma(d)| <= max |e| holds for ANY error pattern (sigma is 1-Lipschitz in
 * the sup norm), also when the errors of many entries coincide, as they do for near-copies of one place (round 5; before, the term was
 * 4 x rms noise / (sigma sqrt(n - 1)), which assumes independent errors: tools/fuzz_all.py, seed 13 case 21, a row of 168 entries of which 99
 * are near-copies of two places, returned ranks 2 / 3 swapped in PR_SC_ARITH_F16 without a flag). */
#define PR_F16_SIGMA_REL 2e-4
#define PR_F16_DIST_ERR 2e-4         /* observed < 1.3e-4 (the worst-case bound of the arithmetic is PR_F16_DISTANCE_BOUND) */
#define PR_F32_SIGMA_REL 5e-7
#define PR_F32_DIST_ERR 2e-7         /* split-f16 / fp32 passes: 2.5e-8 rms, 1.3e-7 at most (tools/probe_bias.py, n = 20 000) */
enum { PR_SC_ARITH_F16X2 = 0, PR_SC_ARITH_F32 = 1, PR_SC_ARITH_F16 = 2 };
/* What a zero-norm SC row does.  MATLAB divides 0/0 (processSC.m:16,19): every distance to or from that signature is NaN, and
 * normalize(.,2) / min (run_test.m:40,57) leave NaNs out [normalize's 'omitnan' from memory], so the signature simply never matches.
 * PR_NAN_EXCLUDE (default) does exactly that and reports PR_WARN_NAN_ROWS; PR_NAN_FAIL turns it into the error PR_ENAN at pr_sync. */
enum { PR_NAN_EXCLUDE = 0, PR_NAN_FAIL = 1 };
enum { PR_WARN_NAN_ROWS = 1, PR_WARN_M2DP_SVD = 2, PR_WARN_F16_FALLBACK = 4, PR_WARN_ORDER_RESOLVED = 8,
       PR_WARN_ORDER_UNRESOLVED = 16, PR_WARN_BOW_TRUNCATED = 32, PR_WARN_BOW_ROWS = 64 };   /* bits of pr_take_warnings; ORDER_RESOLVED: a query was answered from its exact fp64 row (order or containment
                                            check, below); the last one: a caller of the sharded per-pass form stopped (last_pass != 0) with flagged queries left -
                                            those keep the answer of the re-evaluated candidate list.  The library's own calls, stream-ordered or not, run every pass */

#define PR_SC_SIG_LEN 2400    /* 2 x numS*numR = 2 x 60*20, SC/SC.h:7-8, test_sc.cpp:37-38 */
#define PR_M2DP_SIG_LEN 384   /* 2 x (numP*numQ + numS*numR) = 2 x 192, M2DP/M2DP.h:7-10, test_m2dp.cpp:37-39 */
#define PR_DELIGHT_SIG_LEN 256 /* BINS, DELIGHT/DELIGHT.h:9; 16 rows (histograms) per signature, test_delight.cpp:36-37 */

/* ---- context ------------------------------------------------------------------------------------ */
int pr_create(int device_id, pr_ctx** out);
/* The same on a stream the CALLER owns (a hipStream_t, e.g. the stream a torch / RCCL process group enqueues on): every kernel of
 * the context is ordered with the caller's work on that stream, no host synchronisation is needed between the library's phases and
 * the caller's collectives (SURVEY.md §8-e "issue A and B on the compute stream").  The stream must outlive the context. */
int pr_create_on_stream(int device_id, void* hip_stream, pr_ctx** out);
void pr_destroy(pr_ctx* ctx);
const char* pr_last_error(const pr_ctx* ctx);        /* valid until the next call on ctx; ctx may be NULL */
const char* pr_version(void);
/* Selects the matcher arithmetic (SC and M2DP) for signature sets created AFTERWARDS (a set is packed for one arithmetic; matching two
 * sets packed differently is PR_EINVAL).  Initial value: PR_SC_ARITH_F16X2, or PR_SC_ARITH_F32 if the environment has
 * PR_SC_MATCH=f32. */
int pr_set_sc_arith(pr_ctx* ctx, int arith);
int pr_get_sc_arith(const pr_ctx* ctx);
int pr_sync(pr_ctx* ctx);                            /* waits for the context's stream; reports deferred errors */
int pr_set_nan_policy(pr_ctx* ctx, int policy);      /* PR_NAN_EXCLUDE | PR_NAN_FAIL */
int pr_get_nan_policy(const pr_ctx* ctx);
/* on != 0: EVERY query of a top-k call is treated as flagged, i.e. answered from its exact fp64 row (DESIGN.md section 2 "Returned order"):
 * returned scores are then the reference's doubles to rounding (|score - oracle| < 1e-9 whatever |z|; by default they carry the fp32 pass's
 * ~2e-7 relative error of the row sigma, 3e-5 absolute at z = -160).  The host calls, pr_group and stream-ordered calls resolve all queries (passes of 64;
 * a stream-ordered call of m queries chains ceil(m / 64) of them).  Off by default; the environment variable PR_FORCE_ORDER_FLAGS=1 sets it
 * at creation (tests). */
int pr_set_exact_statistics(pr_ctx* ctx, int on);
/* Binary intensity channel (no reference counterpart as a switch; the arithmetic is processSC.m:15-33 on the values SC/SC.cpp:67-72 writes:
 * channel 1 of an SC signature is 0 / 1).  In PR_SC_ARITH_F16X2 the pack notices whether every channel-1 row of a set has all of its non-zero
 * entries equal and positive; the normalised row is then 1/sqrt(ones) on `ones` bins and every one of the 120 products of processSC.m:30 is
 * count / sqrt(ones_q ones_d) with an INTEGER count.  pr_distances_dev / the top-k calls then compute channel 1 with ONE f16 product per
 * term on the hi halves of the same packed images and round max x sqrt(ones_q ones_d) to the nearest integer: the distance is exact (to the
 * fp32 rounding of the final expression, ~1e-7) whenever |x - rint(x)| + b < 1 for the pair, x the computed count of its best variant and b a
 * rigorous bound of the pass's error evaluated ON THE DEVICE from statistics of the two sets (rounding residual norms of the packed spectra) and
 * the pair's ones; the kernel tests every pair.  Sets with non-binary rows or too many ones (beyond ~550 per signature), or a call in which a
 * pair fails the test, get channel 1 from the split-f16 kernel as channel 0 does - same results to 1e-7, no host round trip either way.  on = 0 always takes the split-f16 kernel for both channels (environment: PR_SC_BINARY=0). */
int pr_set_sc_binary(pr_ctx* ctx, int on);
/* *state = 1 when a pr_distances_dev call on these two packed sets takes the binary path for channel 1, 2 when it did and the last call's
 * per-pair rounding test failed somewhere (channel 1 was then redone in split-f16), 0 when the bound rules the path out (reads the sets'
 * statistics back: synchronises; the device takes its own decision from the same numbers). */
int pr_sc_binary_state(pr_ctx* ctx, const pr_sigset* q, const pr_sigset* db, int32_t* state);
/* Measurement hooks (bench.py): on != 0 records HIP events on the context's stream around the matcher launches of every pr_distances_dev call;
 * pr_last_distance_timing waits for the last call's events and returns ms[3] = {channel-0 (or the only) launch, channel-1 single-product
 * launch, channel-1 split-f16 launch}; of the two channel-1 launches one has left at once. */
int pr_set_kernel_timing(pr_ctx* ctx, int on);
int pr_last_distance_timing(pr_ctx* ctx, float* ms);
int pr_take_warnings(pr_ctx* ctx);                   /* PR_WARN_* bits raised since the last call (synchronises the stream), then cleared */
void* pr_stream(pr_ctx* ctx);                        /* the context's hipStream_t (for event timing by the caller) */

/* ---- host-buffer entry points = the reference's own call boundary --------------------------------- */

/* Replaces SC::getSignature looped as in SC/test_sc.cpp:40-56 (SC/SC.h:10-23, SC/SC.cpp:12-76; PCA alignment
 * utils/pts_align.h:7-46 happens inside, as in SC.cpp:17).  Clouds in CSR layout: xyz[offs[N]][3] f64 camera
 * frame, inten[offs[N]] f32, offs[N+1].  out[N][2400] = [structure | intensity], bin = sector*20 + ring. */
int pr_sc_generate(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N,
                   double max_rho, double* out);

/* Replaces the per-cloud body of M2DP/test_m2dp.cpp:41-68: align_points_PCA once, 4 sign variants,
 * M2DP::getSignature (M2DP/M2DP.h:12-30, M2DP/M2DP.cpp:38-109) each.  out[4N][384]. */
int pr_m2dp_generate(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N,
                     double max_rho, double* out);
/* The rows (cloud * 4 + variant, ascending, each once) of the LAST pr_m2dp_generate* call of this context whose leading singular pair is
 * not unique: M2DP/M2DP.cpp:94-103's JacobiSVD returns whichever of the near-equal directions its sweeps end on, and so does this library -
 * those rows may differ from the reference's; PR_WARN_M2DP_SVD is the call-wide bit, which stays until pr_take_warnings.
 * The rule, per count / intensity matrix of a row (sigma_1 >= sigma_2 its two largest singular values): the row is named when the power
 * iteration on A A^T has not converged in 400 steps, or when trace(G^256) > 1.001, G the Gram matrix normalised to unit Frobenius norm
 * after each of 8 squarings (1 for a unique pair, sqrt(j) for a j-fold tie).  A row is ALWAYS named for sigma_1 / sigma_2 <= 1.01, exact
 * ties (sigma_1 == sigma_2: common, the count matrix holds integers) included, and NEVER for sigma_1 / sigma_2 >= 1.03, a rank-1 or a zero
 * matrix; in between either.  An unnamed row is the reference's to 1e-9.  A named row is still a valid signature row: per channel u is a
 * unit vector, to 1e-9 inside the span of the left singular vectors whose sigma_i >= sigma_1 / 1.03, sum(u) >= 0, and v = A^T u / ||A^T u||;
 * a channel of a named row whose own matrix has a unique pair is the reference's to 1e-9.
 * At most cap rows are written (cap = 0: rows may be NULL), *count is the number of such rows; the library records the first 1024
 * (row, channel) pairs of a call, so *count <= 1024 and, beyond that many pairs, further rows are covered by the call-wide bit only. */
int pr_m2dp_svd_rows(pr_ctx* ctx, int32_t* rows, int32_t cap, int32_t* count);

/* Replaces DELIGHT::getSignature looped as in DELIGHT/test_delight.cpp:41-56 (DELIGHT/DELIGHT.h:11-18, DELIGHT.cpp:8-24;
 * PCA alignment inside).  out[16N][256]: 16 intensity histograms per cloud. */
int pr_delight_generate(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N, double* out);

/* Replaces GIST::extract looped as in GIST/src/test_gist.cpp:57-96 (gist.cpp:54-94 -> libgist.cpp:914-951, bw_gist_scaletab, grayscale):
 * img [N][256][256] row-major, dtype PR_U8 (mono8, as cv_bridge gives it) or PR_F32.  Images must be 256 x 256: GIST::extract resizes
 * (INTER_LANCZOS4) and centre-crops other sizes first (gist.cpp:62-75), which the caller does; otherwise PR_EINVAL.
 * nblocks 1..16, n_scale 1..8, orients[n_scale] 1..32 each; the reference's defaults are 4, 4, {8, 8, 8, 8} (test_gist.cpp:57).
 * out [N][pr_gist_signature_size()] float: per filter (scale-major), the nblocks x nblocks block means, res[k * nblocks + l] with k the
 * x (column) block (libgist.cpp:600-629).  A descriptor with a NaN or Inf makes the host form return PR_ENAN (the reference returns NULL,
 * libgist.cpp:936-945); the device form (img, out device pointers) leaves such a row as NaN, is stream-ordered without host waits, and after
 * its first call with a parameter set and batch size allocates nothing (graph-capturable). */
int pr_gist_signature_size(int32_t nblocks, int32_t n_scale, const int32_t* orients);
int pr_gist_generate(pr_ctx* ctx, const void* img, int dtype, int32_t N, int32_t height, int32_t width, int32_t nblocks, int32_t n_scale,
                     const int32_t* orients, float* out);
int pr_gist_generate_dev(pr_ctx* ctx, const void* img, int dtype, int32_t N, int32_t height, int32_t width, int32_t nblocks,
                         int32_t n_scale, const int32_t* orients, float* out);

/* DBoW2 vocabulary of ORB descriptors (ORB_SLAM2::ORBVocabulary = TemplatedVocabulary<FORB::TDescriptor, FORB>), independent of any
 * context.  pr_bow_vocab_load reads ORBvoc-style text (TemplatedVocabulary.h:1338-1424, loadFromTextFile: a header `k L scoring weighting`,
 * then one node per line `parent isLeaf d0 .. d31 weight`, node id = line position, root = node 0 without a line) or the binary side-car of
 * pr_bow_vocab_save_bin, told apart by its magic.  Empty lines are skipped (the reference appends a node with undefined bytes for them).
 * PR_EINVAL (message in pr_host_last_error) for a header outside 0 <= k <= 20, 1 <= L <= 10, scoring 0..5, weighting 0..3, or a line with
 * fewer than 35 tokens, a non-numeric token, a non-finite weight or parent >= its own id.  Node arrays cover the root at index 0 (export
 * writes -1 / 0 / zeros / 0 for it, create ignores it): parent [n_nodes] i32, is_leaf [n_nodes] u8 (> 0: a word, ids in node order),
 * desc [n_nodes][32] u8, weight [n_nodes] f64.  info: [k, L, scoring, weighting]. */
int pr_bow_vocab_load(const char* path, pr_bow_vocab** out);
int pr_bow_vocab_save_bin(const pr_bow_vocab* v, const char* path);
int pr_bow_vocab_create(int32_t k, int32_t L, int32_t scoring, int32_t weighting, int64_t n_nodes, const int32_t* parent,
                        const uint8_t* is_leaf, const uint8_t* desc, const double* weight, pr_bow_vocab** out);
int pr_bow_vocab_info(const pr_bow_vocab* v, int32_t* info, int64_t* n_nodes, int64_t* n_words);
int pr_bow_vocab_export(const pr_bow_vocab* v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight);
void pr_bow_vocab_destroy(pr_bow_vocab* v);

/* Replaces ORBVocabulary::transform looped as in BoW/test_bow.cpp:127-135 (TemplatedVocabulary.h:1127-1260; the FeatureVector is not
 * produced).  desc [offs[N]][32] u8 ORB descriptors (the rows of ORBextractor's cv::Mat), offs [N+1] i64 (CSR, offs[0] = 0).
 * out [2N][cols] f64 in pr_bow_distance's layout: per image a row of word ids in ascending order and a row of their values, both padded
 * with -1.  n_words [N] (optional): each image's distinct-word count.  The host form returns PR_EINVAL naming the first image with more
 * than cols words.  The device form (desc, offs, out, n_words, feat_words device pointers; n_desc = offs[N]) is stream-ordered without host
 * waits and, after its first call with this vocabulary and at least this many descriptors, allocates nothing (graph-capturable); a row
 * with more than cols words keeps its first cols and raises PR_WARN_BOW_TRUNCATED, n_words still holds the true count.  feat_words
 * [n_desc] (optional): each descriptor's word id (-1 for every descriptor when the vocabulary has no words). */
int pr_bow_generate(pr_ctx* ctx, const pr_bow_vocab* vocab, const uint8_t* desc, const int64_t* offs, int32_t N, int32_t cols,
                    double* out, int32_t* n_words);
int pr_bow_generate_dev(pr_ctx* ctx, const pr_bow_vocab* vocab, const uint8_t* desc, int64_t n_desc, const int64_t* offs, int32_t N,
                        int32_t cols, double* out, int32_t* n_words, int32_t* feat_words);

/* Replaces processDELIGHT(hist1, hist2) (match_signatures/processDELIGHT.m:1-38).  h1[16m][256], h2[16n][256];
 * dist: host f32 [m][n] (chi-square, min over the 4 octant permutations; +Inf when no bin is occupied). */
int pr_delight_distance(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, float* dist);

/* Replaces processSC(hist1, hist2) (match_signatures/processSC.m:1-45).  h1[m][2400], h2[n][2400] host f64;
 * d_struct / d_int: host f32 [m][n], either may be NULL.  A zero-norm row (MATLAB: 0/0 = NaN, processSC.m:16,19) gives NaN distances and
 * PR_WARN_NAN_ROWS (default policy PR_NAN_EXCLUDE); with PR_NAN_FAIL the call returns PR_ENAN instead. */
int pr_sc_distance(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n,
                   float* d_struct, float* d_int);

/* Replaces processM2DP(hist1, hist2) (match_signatures/processM2DP.m:1-22).  h1[4m][384], h2[4n][384]. */
int pr_m2dp_distance(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n,
                     float* d_cnt, float* d_int);

/* Replaces run_test.m:26-57 (distance matrices, 2:1 z-score fusion :38-41, mask :47-53, row min :57),
 * generalised to top-k; k = 1 is the reference.  Ties -> lower index (MATLAB min).  idx[m][k] (0-based,
 * -1 when fewer than k candidates), score[m][k] fused z-score.  type = PR_TYPE_DELIGHT: no fusion (run_test.m:26-36),
 * score = the chi-square distance, h1[16m][256], h2[16n][256], p_weight ignored. */
int pr_match_topk(pr_ctx* ctx, int type, const double* h1, int32_t m, const double* h2, int32_t n,
                  int32_t mask_width, double p_weight, int32_t k, int32_t* idx, float* score);
/* The same with the scores as the reference holds them (MATLAB double, run_test.m:57 `diff_v`).  For SC and M2DP both variants
 * re-evaluate the k + 8 best pairs of the fp32 all-pairs pass in fp64 from the raw signatures (pr_rerank_dev): indices and scores
 * are those of the reference's double arithmetic given the row statistics (see DESIGN.md for the error of those). */
int pr_match_topk_f64(pr_ctx* ctx, int type, const double* h1, int32_t m, const double* h2, int32_t n,
                      int32_t mask_width, double p_weight, int32_t k, int32_t* idx, double* score);

/* The two remaining `type`s of run_test.m:32-35, whose signatures have no fixed length (`cols` columns per row):
 *   gist: h [m][cols];            dist(i,j) = sum_c (h1[i,c] - h2[j,c])^2                    (processGIST.m:1-10)
 *   bow:  h [2 m][cols], rows alternate word ids | weights, padded with -1 (test_bow.cpp:147-162);
 *         dist(i,j) = 1 - DBoW2 L1 score                                                    (processBoW.m:1-38)
 * pr_match_topk_cols: mask + row minimum without fusion (run_test.m:47-57), type = PR_TYPE_GIST | PR_TYPE_BOW. */
int pr_gist_distance(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, float* dist);
int pr_bow_distance(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, float* dist);
int pr_match_topk_cols(pr_ctx* ctx, int type, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols,
                       int32_t mask_width, int32_t k, int32_t* idx, float* score);

/* BoW matching through an inverted file (word-major lists of (row, weight) postings), exact in fp64: distances and top-k are those of
 * processBoW.m:22-37 + run_test.m:47-57 evaluated in double, bit for bit (ties -> lower index, masked entries +Inf, NaN never selected,
 * -1 / NaN fill), for CONFORMING rows: before the reference's end of a row (its first column p < cols - 1 with !(id > -1); the last column
 * is never read) every id is an integer in [0, n_words) and the ids ascend strictly - what test_bow.cpp:147-162 and pr_bow_generate* write.
 * Weights may be any double.  Rows: [2 n][cols] f64, ids | weights per image (pr_bow_distance's layout).
 *   pr_bow_db_create   capacities are fixed here: max_sigs rows, max_postings words over all rows; n_words the vocabulary size.  The
 *                      device scratch of one match chunk (<= 512 MB of fp64 accumulators) and a tail segment are allocated once.
 *                      Environment: PR_BOW_TAIL_ROWS (tail capacity, default 1024), PR_BOW_CHUNK (queries per chunk), PR_BOW_THREADS
 *                      (64 | 256, threads per query).
 *   pr_bow_db_set      replaces the contents with rows (where: PR_HOST | PR_DEVICE) and builds the index (validate, count, scan, scatter).
 *   pr_bow_db_append   adds rows count .. count + n_new - 1 to a tail segment whose lists are rebuilt from the tail rows only; a full tail
 *                      is first folded into the main lists (the one step whose cost grows with n).  Any sequence of appends gives the
 *                      results of one set of the same rows.
 *                      Both synchronise, reject a non-conforming row with PR_EINVAL naming the first one, exceed a capacity with PR_ENOMEM.
 *   pr_bow_match_topk_dev  q DEVICE [2 m][cols] against all rows; idx DEVICE [m][k] global rows (db_row0 + local), score DEVICE f64 [m][k],
 *                      ascending by (score, index) with -1 / NaN last (pr_merge_topk_dev merges shards unchanged); the mask compares
 *                      q_row0 + i with db_row0 + j.  k <= 128.  Stream-ordered, allocation-free, graph-capturable.  A non-conforming
 *                      query row gets -1 / NaN in all k slots and raises PR_WARN_BOW_ROWS (pr_take_warnings).
 *   pr_bow_match_topk_f64  the host form of run_test.m:32-57 for 'bow' in fp64 (h1 [2 m][cols], h2 [2 n][cols] host);
 *   pr_bow_distance_f64    the exact fp64 matrix dist [m][n] (host) through the same index.  Both return PR_EINVAL for a non-conforming
 *                      row of either side. */
int pr_bow_db_create(pr_ctx* ctx, int32_t max_sigs, int32_t cols, int32_t n_words, int64_t max_postings, pr_bow_db** out);
void pr_bow_db_destroy(pr_ctx* ctx, pr_bow_db* db);
int pr_bow_db_set(pr_ctx* ctx, pr_bow_db* db, const double* rows, int where, int32_t n);
int pr_bow_db_append(pr_ctx* ctx, pr_bow_db* db, const double* rows, int where, int32_t n_new);
int32_t pr_bow_db_count(const pr_bow_db* db);
int pr_bow_match_topk_dev(pr_ctx* ctx, const pr_bow_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0,
                          int32_t mask_width, int32_t k, int32_t* idx, double* score);
int pr_bow_match_topk_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols,
                          int32_t mask_width, int32_t k, int32_t* idx, double* score);
int pr_bow_distance_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, double* dist);

/* GIST matching against a device-resident database, exact in fp64: for rows a, b of cols doubles d = ((0 + t_0) + t_1) + ... with
 * t_c = RN(RN(a_c - b_c)^2), ascending columns, no contraction (processGIST.m:7 read left to right), then run_test.m:47-57 generalised
 * to top-k as for pr_bow_match_topk_dev: masked entries +Inf, ascending by (score, index), ties -> lower index, NaN distances (a NaN in
 * either row) never selected, -1 / NaN fill.  Indices and score bits are those of that arithmetic for every input.  A coarse pass on the
 * f16 matrix cores lists k + 8 candidates per query and DB slab, their distances are re-evaluated in fp64, and a query whose list is not
 * provably complete under a worst-case error bound is answered from its exact row.
 *   pr_gist_db_create   capacity max_sigs rows of cols doubles (any cols >= 1); all device memory, scratch included, is allocated here
 *                       (pr_gist_db_bytes reports it).  Environment: PR_GIST_EXACT=1 answers every query from its exact row;
 *                       PR_GIST_CENTRE=0 packs the rows without subtracting their mean (same results, a wider bound: for A/B runs).
 *   pr_gist_db_set      replaces the contents with rows [n][cols] (where: PR_HOST | PR_DEVICE).
 *   pr_gist_db_append   adds rows count .. count + n_new - 1; any sequence of appends gives the results of one set of the same rows.
 *                       Both synchronise; beyond max_sigs they return PR_ENOMEM.
 *   pr_gist_db_set_exact  on != 0: every query takes the exact-row path (the independent implementation tests compare against).
 *   pr_gist_match_topk_dev  q DEVICE [m][cols]; idx DEVICE [m][k] global rows (db_row0 + local), score DEVICE f64 [m][k]
 *                       (pr_merge_topk_dev merges shards unchanged); the mask compares q_row0 + i with db_row0 + j.  k <= 128.
 *                       Stream-ordered, allocation-free, graph-capturable.
 *                       The call writes the database's scratch: one match at a time per database (two contexts must not match the
 *                       same database concurrently).
 *   pr_gist_flagged_count  of the m queries of this context's last pr_gist_match_topk_dev (m must be that call's m, else PR_EINVAL; the
 *                       database must still exist), how many were answered from their exact row (synchronises).
 *   pr_gist_match_topk_f64  the host form of run_test.m:32-57 for 'gist' in fp64 (h1 [m][cols], h2 [n][cols] host).
 *   pr_gist_distance_f64    the exact fp64 matrix dist [m][n] (host). */
typedef struct pr_gist_db pr_gist_db;
int pr_gist_db_create(pr_ctx* ctx, int32_t max_sigs, int32_t cols, pr_gist_db** out);
void pr_gist_db_destroy(pr_ctx* ctx, pr_gist_db* db);
int pr_gist_db_set(pr_ctx* ctx, pr_gist_db* db, const double* rows, int where, int32_t n);
int pr_gist_db_append(pr_ctx* ctx, pr_gist_db* db, const double* rows, int where, int32_t n_new);
int32_t pr_gist_db_count(const pr_gist_db* db);
int64_t pr_gist_db_bytes(const pr_gist_db* db);
void pr_gist_db_set_exact(pr_gist_db* db, int on);
int pr_gist_match_topk_dev(pr_ctx* ctx, const pr_gist_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0,
                           int32_t mask_width, int32_t k, int32_t* idx, double* score);
int pr_gist_flagged_count(pr_ctx* ctx, int32_t m, int32_t* count);
int pr_gist_match_topk_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols,
                           int32_t mask_width, int32_t k, int32_t* idx, double* score);
int pr_gist_distance_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, double* dist);

/* DELIGHT matching against a device-resident database, exact in fp64 (processDELIGHT.m:7-37): for signatures a, b of 16 x 256 doubles and
 * each of the four octant permutations (row r of a against row r ^ X of b, X = 0, 5, 6, 3): ts = tc = 0; for c = 0..255, for r = 0..15:
 * sum = a + b, if (sum > 0) { ts += ((2 (a - b)) (a - b)) / sum; tc += 1 }; ts = ts / tc; d = the smallest ts (NaN never wins, +Inf when
 * no bin is occupied), no contraction.  Then run_test.m:47-57 generalised to top-k as for pr_gist_match_topk_dev: masked entries +Inf,
 * ascending by (score, index), ties -> lower index, NaN never selected, -1 / NaN fill.  Indices and score bits are those of that
 * arithmetic for every input.  A coarse fp32 pass (the arithmetic of pr_match_topk's DELIGHT kernel, no m x n matrix) lists k + 8
 * candidates per query and DB slab, their distances are re-evaluated in fp64, and a query whose list is not provably complete under a
 * worst-case error bound is answered from its exact row.  A signature with an element that is not an integer in
 * [0, 2^24] is outside the coarse pass: as a query it takes the exact-row path, as a DB row it sends every query there.
 *   pr_delight_db_create   capacity max_sigs signatures; all device memory, scratch included, is allocated here (pr_delight_db_bytes
 *                       reports it: 49 668 bytes per signature + scratch).  Environment: PR_DELIGHT_EXACT=1 answers every query from
 *                       its exact row.
 *   pr_delight_db_set      replaces the contents with rows [16 n][256] (where: PR_HOST | PR_DEVICE).
 *   pr_delight_db_append   adds signatures count .. count + n_new - 1; any sequence of appends equals one set of the same rows.
 *                       Both synchronise; beyond max_sigs they return PR_ENOMEM.
 *   pr_delight_db_set_exact  on != 0: every query takes the exact-row path (the independent implementation tests compare against).
 *   pr_delight_match_topk_dev  q DEVICE [16 m][256]; idx DEVICE [m][k] global rows (db_row0 + local), score DEVICE f64 [m][k]
 *                       (pr_merge_topk_dev merges shards unchanged); the mask compares q_row0 + i with db_row0 + j.  k <= 128.
 *                       Stream-ordered, allocation-free, graph-capturable.  The call writes the database's scratch: one match at a
 *                       time per database.
 *   pr_delight_flagged_count  of the m queries of this context's last pr_delight_match_topk_dev (m must be that call's m, else
 *                       PR_EINVAL; the database must still exist), how many were answered from their exact row (synchronises).
 *   pr_delight_match_topk_f64  the host form of run_test.m:32-57 for 'delight' in fp64 (h1 [16 m][256], h2 [16 n][256] host).
 *   pr_delight_distance_f64    the exact fp64 matrix dist [m][n] (host). */
typedef struct pr_delight_db pr_delight_db;
int pr_delight_db_create(pr_ctx* ctx, int32_t max_sigs, pr_delight_db** out);
void pr_delight_db_destroy(pr_ctx* ctx, pr_delight_db* db);
int pr_delight_db_set(pr_ctx* ctx, pr_delight_db* db, const double* rows, int where, int32_t n);
int pr_delight_db_append(pr_ctx* ctx, pr_delight_db* db, const double* rows, int where, int32_t n_new);
int32_t pr_delight_db_count(const pr_delight_db* db);
int64_t pr_delight_db_bytes(const pr_delight_db* db);
void pr_delight_db_set_exact(pr_delight_db* db, int on);
int pr_delight_match_topk_dev(pr_ctx* ctx, const pr_delight_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0,
                              int32_t mask_width, int32_t k, int32_t* idx, double* score);
int pr_delight_flagged_count(pr_ctx* ctx, int32_t m, int32_t* count);
int pr_delight_match_topk_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t mask_width, int32_t k,
                              int32_t* idx, double* score);
int pr_delight_distance_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, double* dist);

/* BASELINE.json config 5, "fused SC + M2DP scoring" - NO reference counterpart (run_test.m handles one type per run);
 * build-defined as in SURVEY.md §6: score = [p z(sc_struct) + z(sc_int)] + [p z(m2dp_count) + z(m2dp_int)] with the row
 * z-scores of run_test.m:40, then mask and row minimum (run_test.m:47-57).  sc: [m][2400], m2dp: [4 m][384] of the same places.
 * pr_fuse_select2_dev is the device-level step (two channel pairs over the same grid, moments as pr_row_moments_dev). */
int pr_match_topk_fused(pr_ctx* ctx, const double* sc1, const double* m2dp1, int32_t m, const double* sc2, const double* m2dp2,
                        int32_t n, int32_t mask_width, double p_weight, int32_t k, int32_t* idx, float* score);
int pr_match_topk_fused_f64(pr_ctx* ctx, const double* sc1, const double* m2dp1, int32_t m, const double* sc2, const double* m2dp2,
                            int32_t n, int32_t mask_width, double p_weight, int32_t k, int32_t* idx, double* score);
/* Host forms of pr_align_pairs_dev / pr_delight_align_pairs_dev (the variants of processSC.m:22-33, processM2DP.m:12-22,
 * processDELIGHT.m:7-37 that match() keeps only the minimum of): idx [m][k] as pr_match_topk returns it (-1 or a row of h2).  Only the
 * DB rows idx references are uploaded (at most m k distinct ones): the cost does not grow with n.  variant / dist [m][k][2]: SC structure,
 * intensity; M2DP count, intensity; DELIGHT the result in [0], -1 / NaN in [1].  The fused form: [m][k][4] in p5 channel order. */
int pr_match_align(pr_ctx* ctx, int type, const double* h1, int32_t m, const double* h2, int32_t n, int32_t k, const int32_t* idx,
                   int32_t* variant, double* dist);
int pr_match_align_fused(pr_ctx* ctx, const double* sc1, const double* m2dp1, int32_t m, const double* sc2, const double* m2dp2,
                         int32_t n, int32_t k, const int32_t* idx, int32_t* variant, double* dist);
int pr_fuse_select2_dev(pr_ctx* ctx, const float* d_p, const float* d_i, const float* e_p, const float* e_i, int32_t m, int32_t n,
                        const double* mom_all, const double* mom2_all, int32_t G, int32_t q_row0, int32_t db_row0,
                        int32_t mask_width, double p_weight, int32_t k, int32_t* idx, float* score);

/* ---- device-resident entry points (inputs already in HBM; what bench.py and the multi-GPU layer call) -- *
 * All are asynchronous on the context's stream; pr_sync() surfaces deferred errors (e.g. PR_ENAN).         */

/* A packed signature set: rows normalised as processSC.m:15-20 and stored as the per-ring sector spectra
 * (SC), or the 4-variant rows as-is (M2DP, processM2DP.m:15), in the MFMA operand layout of its role. */
#define PR_MAX_SIGS 4000000          /* capacity limit of one signature set (32-bit offsets inside the matchers) */
int pr_sigset_create(pr_ctx* ctx, int type, int role, int32_t max_sigs, pr_sigset** out);
void pr_sigset_destroy(pr_ctx* ctx, pr_sigset* s);
/* pr_sigset_pack inside a captured hipGraph: whether the image is zero-filled first is decided on the HOST from the set's history (a re-pack
 * of at least as many rows in the same geometry needs no fill) and baked into the graph as the presence or absence of a memset node.  A set
 * packed inside a captured graph must therefore not be re-packed with ANOTHER row count outside it between replays: the replayed pack would
 * run without the fill it then needs.  (Packing other sets, or this one with the captured count, is fine.) */
int pr_sigset_pack(pr_ctx* ctx, pr_sigset* s, const void* sig, int dtype, int where, int32_t n_sigs);
int32_t pr_sigset_count(const pr_sigset* s);
/* A DB that grows by one signature per keyframe (SC/test_sc.cpp:40-56 appends a row per cloud; run_test.m:57 matches a query against
 * everything before it).  The operand image is [channel][group][...]; pr_sigset_pack lays it out for the COUNT it is given, so a larger count
 * means a full re-pack.  pr_sigset_reserve fixes the layout at the CAPACITY (max_sigs of pr_sigset_create) instead: the set is emptied, and from
 * then on pr_sigset_pack (bulk: rows 0 .. n_sigs - 1, the set's new count) and pr_sigset_append (rows count .. count + n_new - 1, everything else
 * untouched) write into that one layout - an appended image is bit for bit the image a bulk pack of all rows writes, and the binary-channel
 * statistics of an SC set are folded in, not recomputed.  pr_sigset_append on an EMPTY set reserves by itself.  DB sets of SC
 * or M2DP signatures in the f16 arithmetics (the defaults); such a set is matched by the default kernels only (PR_EINVAL from
 * pr_distances_dev under PR_SC_KERNEL / PR_SC_ONLINE=h).  sig: n_new signatures, [n_new][2400] (SC) or [4 n_new][384] (M2DP), as for
 * pr_sigset_pack.  Stream-ordered (one kernel; PR_HOST buffers are staged and the call then waits).  The raw rows the fp64 re-evaluation reads
 * (pr_rerank_dev's db_sc / db_m2) are the caller's: append them to that buffer too. */
int pr_sigset_reserve(pr_ctx* ctx, pr_sigset* s);
int pr_sigset_append(pr_ctx* ctx, pr_sigset* s, const void* sig, int dtype, int where, int32_t n_new);
/* the packed operand image (DEVICE pointer, read-only), its size and its channel stride in groups / tiles: for tests and for saving a packed DB */
int pr_sigset_image(const pr_sigset* s, const void** image, size_t* bytes, int32_t* channel_stride_groups);

/* processSC.m:22-33 / processM2DP.m:15-21 / processDELIGHT.m:7-37 on packed sets.  d_p, d_i: DEVICE f32 [m][n]
 * (row stride n); DELIGHT writes d_p only (d_i may be NULL). */
int pr_distances_dev(pr_ctx* ctx, const pr_sigset* q, const pr_sigset* db, float* d_p, float* d_i);

/* Per-row moments (one fp64 pass of shifted sums) of a distance shard (first half of MATLAB normalize(.,2), run_test.m:40):
 * mom: DEVICE f64 [m][2][3] = (count, mean, M2 = sum (x-mean)^2) for channel 0 = d_p, 1 = d_i. */
int pr_row_moments_dev(pr_ctx* ctx, const float* d_p, const float* d_i, int32_t m, int32_t n, double* mom);

/* run_test.m:38-41 + :47-53 + :57 on a DB shard.  mom_all: DEVICE f64 [G][m][2][3] moments of ALL G shards
 * (combined in rank order, N-1 std); the shard's DB rows are global rows db_row0..db_row0+n-1 and its query
 * rows global q_row0..; mask is |i-j| < mask_width on GLOBAL indices.  idx: DEVICE i32 [m][k] GLOBAL DB
 * indices (-1 = none), score: DEVICE f32 [m][k].  d_i == NULL: plain selection on d_p without fusion (mom_all unused). */
int pr_fuse_select_dev(pr_ctx* ctx, const float* d_p, const float* d_i, int32_t m, int32_t n,
                       const double* mom_all, int32_t G, int32_t q_row0, int32_t db_row0, int32_t mask_width,
                       double p_weight, int32_t k, int32_t* idx, float* score);
/* The same, also leaving the (fp32-rounded) scores widened to doubles in score64 DEVICE [m][k] - the form pr_rerank_dev /
 * pr_merge_topk_dev take them in (saves a pr_widen_scores_dev launch; pr_fuse_select2_f64_dev likewise). */
int pr_fuse_select_f64_dev(pr_ctx* ctx, const float* d_p, const float* d_i, int32_t m, int32_t n,
                           const double* mom_all, int32_t G, int32_t q_row0, int32_t db_row0, int32_t mask_width,
                           double p_weight, int32_t k, int32_t* idx, float* score, double* score64);
/* pr_row_moments_dev + pr_fuse_select_f64_dev of ONE shard (G = 1) in one call: mom [m][2][3], idx, score, score64 [m][k] come out bit
 * for bit as from the two calls.  Whole-row selections of up to 16 results (the k + 8 of the fp32-grade arithmetics; more rows than
 * the sliced form takes, rows longer than the one-wave form's) read the distances ONCE: the candidates are collected in the sweep that
 * accumulates the moments, and a row whose collected set does not provably hold its k best is swept a second time.
 * PR_SELECT_FUSED=0 in the environment (read once) keeps the two passes.
 * pr_select_fallback_rows: the rows that took the second sweep since the last call of it (synchronises the stream; clears the count). */
int pr_moments_select_f64_dev(pr_ctx* ctx, const float* d_p, const float* d_i, int32_t m, int32_t n, double* mom, int32_t q_row0,
                              int32_t db_row0, int32_t mask_width, double p_weight, int32_t k, int32_t* idx, float* score, double* score64);
int pr_select_fallback_rows(pr_ctx* ctx, int64_t* rows);
int pr_fuse_select2_f64_dev(pr_ctx* ctx, const float* d_p, const float* d_i, const float* e_p, const float* e_i, int32_t m, int32_t n,
                            const double* mom_all, const double* mom2_all, int32_t G, int32_t q_row0, int32_t db_row0,
                            int32_t mask_width, double p_weight, int32_t k, int32_t* idx, float* score, double* score64);

/* fp64 re-evaluation of the survivors of pr_fuse_select_dev (run with k_in = k + 8): for every (query, idx_in entry of THIS shard)
 * the distances of the pair again from the RAW signatures in fp64, in the reference's own formulation (processSC.m:15-33: rows / L2
 * norm, 120 shifted / mirrored variants, (1 - dot)/2, min; processM2DP.m:12-22), the fused score of run_test.m:40 with the combined
 * moments, then the k best by (score, index) (run_test.m:57).  q_sc/db_sc: DEVICE [m][2400] / [n_local][2400] or NULL; q_m2/db_m2:
 * DEVICE [4m][384] / [4 n_local][384] or NULL (both pairs given = BASELINE config 5's sum of four z-scores); dtype PR_F64 | PR_F32;
 * mom_sc / mom_m2: DEVICE [G][m][2][3] as pr_row_moments_dev writes them.  idx_in: DEVICE [m][k_in] global indices inside
 * [db_row0, db_row0 + n_local) or -1.  idx: DEVICE [m][k], score: DEVICE f64 [m][k].  k_in <= 128. */
/* Width of the candidate list the top-k protocol re-evaluates for k results in the context's arithmetic: k + 8, or k + 56 in
 * PR_SC_ARITH_F16 (capped at 128). */
int pr_rerank_width(const pr_ctx* ctx, int32_t k);
/* PR_SC_ARITH_F16 only: after pr_rerank_dev / pr_rerank_finish_dev, flags[q] = 1 (DEVICE i32 [m]) for every query whose candidate list
 * (cand_score: the f16 pass scores of the k_in candidates, DEVICE f64 [m][k_in], ascending as pr_fuse_select_dev / pr_merge_topk_dev
 * return them) does not provably contain the exact top-k: exact k-th score (score: DEVICE f64 [m][k]) >= last candidate's pass score
 * minus the score error bound that PR_F16_DISTANCE_BOUND implies with the row's statistics (mom_*: as for pr_rerank_dev).
 * count: DEVICE i32 [1], set to the number of flags.  Flagged queries must be recomputed in PR_SC_ARITH_F16X2.
 * Also flagged: queries whose re-evaluated ORDER is not certain.  A re-evaluated score is exact in the pair's distances, but its
 * channel terms are divided by the f16 pass's row sigmas; two candidates whose channels disagree about their order can change places
 * when those sigmas move by what the pass's distance errors allow (PR_F16_SIGMA_REL + PR_F16_DIST_ERR / sigma).
 * pr_rerank_dev (one shard) / pr_rerank_finish_dev (sharded) check every adjacent pair of the selected k and the best candidate left out and
 * leave the result in the context; this call takes it (once). */
int pr_f16_margin_dev(pr_ctx* ctx, const double* mom_sc, const double* mom_m2, int32_t m, int32_t G, double p_weight, int32_t k_in,
                      const double* cand_score, int32_t k, const double* score, int32_t* flags, int32_t* count);
int pr_rerank_dev(pr_ctx* ctx, const void* q_sc, const void* db_sc, int sc_dtype, const void* q_m2, const void* db_m2, int m2_dtype,
                  const double* mom_sc, const double* mom_m2, int32_t m, int32_t n_local, int32_t G, int32_t q_row0, int32_t db_row0,
                  int32_t mask_width, double p_weight, int32_t k_in, const int32_t* idx_in, const double* score_in, int32_t k, int32_t* idx,
                  double* score);
/* score_in / cand_score (both forms; DEVICE f64 [m][k_in], may be NULL): the candidates' scores from the fp32 pass, ascending as
 * pr_fuse_select_dev / pr_merge_topk_dev deliver them.  With them a candidate beyond the k-th whose fp32 score exceeds the k-th by more than
 * 64 x the error bound of an fp32 score (from the row statistics) is not re-evaluated - it cannot enter the exact top-k; results are identical.
 *
 * The "p5" block of a re-evaluation, DEVICE f64 [m][5][k_in] per shard: for every query the candidates' scores [k_in], then their four exact
 * channel distances [4][k_in] (SC structure, SC intensity, M2DP count, M2DP intensity; 0 for an absent type; NaN in the first = the pair
 * was not evaluated here: masked (+Inf score), pruned (it keeps its pass score), or another shard's (NaN score)).  pr_rerank_dev keeps its
 * block in the context; the sharded protocol gathers the shards' blocks ([G][m][5][k_in]): it is all the order check and the fp64-statistics
 * resolution need.
 *
 * The sharded form of the re-evaluation (what makes its cost independent of the number of shards): the shards' fp32 top-(k+8) lists
 * are merged FIRST (pr_merge_topk_dev on the gathered lists) into the global candidates cand_idx DEVICE [m][k_in]; every shard then
 * evaluates only the candidates inside its rows [db_row0, db_row0 + n_local) (pr_rerank_partial_dev -> its p5 block), the blocks are
 * all-gathered, and pr_rerank_finish_dev takes each candidate's score from its owner, selects the k best and runs the order and containment
 * checks below (mom_*: the statistics the scores were formed with, [G_mom][m][2][3]; cand_score: the merged pass scores of cand_idx, DEVICE f64
 * [m][k_in] ascending, or NULL = no containment check); the flags stay in the context. */
int pr_rerank_partial_dev(pr_ctx* ctx, const void* q_sc, const void* db_sc, int sc_dtype, const void* q_m2, const void* db_m2, int m2_dtype,
                          const double* mom_sc, const double* mom_m2, int32_t m, int32_t n_local, int32_t G, int32_t q_row0, int32_t db_row0,
                          int32_t mask_width, double p_weight, int32_t k_in, const int32_t* cand_idx, const double* cand_score, int32_t k,
                          double* p5);
int pr_rerank_finish_dev(pr_ctx* ctx, const double* mom_sc, const double* mom_m2, int32_t G_mom, const int32_t* cand_idx, const double* cand_score,
                         const double* p5_all, int32_t G, int32_t m, int32_t k_in, int32_t k, double p_weight, int32_t* idx, double* score);
/* Two checks, every arithmetic (run_test.m:38-41,57 are fp64 over the WHOLE row; the all-pairs pass is neither).  pr_rerank_dev /
 * pr_rerank_finish_dev leave in the context one word per query:
 *   bit 0  ORDER: two neighbours among the re-evaluated candidates (the selected k and the best one left out) could change places under the
 *          sigma error of the all-pairs pass (their channels disagree about the order and the scores are closer than
 *          sum_c eps_c |z_c(a) - z_c(b)|, eps_c = PR_F32_SIGMA_REL + PR_F32_DIST_ERR / sigma_c; PR_SC_ARITH_F16: the PR_F16_*
 *          constants, and pr_f16_margin_dev takes the flags - such queries go to the split-f16 pass);
 *   bit 1  CONTAINMENT (needs the candidates' pass scores: score_in / cand_score; not in PR_SC_ARITH_F16, whose margin check is
 *          pr_f16_margin_dev): every entry outside the k_in candidates has a pass score >= the last candidate's, T, hence an exact score
 *          >= T - err(T) - (what the sigma error can move it against a listed entry); when the exact k-th best is not below that, an entry
 *          the list does not hold could belong to the top-k - more than k_in entries whose scores agree to the pass's resolution (1e-6 in
 *          the distances): near-copies of one place.
 * A flagged query is answered from its EXACT ROW: its distances to ALL n entries in fp64 -> (count, mean, M2) per channel -> fused scores,
 * mask, the k smallest by (score, index): indices and scores of that query are then those of fp64 arithmetic throughout (run_test.m:38-57),
 * whatever the all-pairs pass made of it.  Three forms, all in passes of 64 flagged queries (ascending):
 *   pr_order_resolve_async_dev  single shard, right after pr_rerank_dev; STREAM-ORDERED, no host synchronisation (fixed-grid kernels that
 *                               leave at once when nothing is flagged; hipGraph-capturable).  ceil(m / 64) passes are chained on the
 *                               stream, so ALL flagged queries are resolved whatever their number (an empty pass costs its launches,
 *                               ~10 us).  mom_sc / mom_m2 rows of resolved queries are overwritten with the exact ones.
 *                               PR_WARN_ORDER_RESOLVED is raised (at pr_take_warnings) when a query was.
 *   pr_order_resolve_dev        the same with a host round trip (reads the count back): ALL flagged queries, *resolved (may be NULL)
 *                               = their number.  The host top-k calls use this one.
 *   sharded                     after pr_rerank_finish_dev, per pass (offset = 0, 64, ...; pr_order_flagged_count gives the total, with a host
 *                               synchronisation; a stream-ordered caller chains ceil(m / 64) passes - empty ones leave at once).  The pass
 *                               called with last_pass != 0 raises PR_WARN_ORDER_UNRESOLVED when flagged queries remain behind it (a
 *                               caller that stops early); no pass ever clears that bit: pr_order_exact_moments_dev = this shard's rows of
 *                               the flagged queries (kept in the context) and their exact (count, mean, M2), exact DEVICE f64 [m][4][3] (rows
 *                               of other queries: unspecified) -> all-gather -> exact_all [G][m][4][3] -> pr_order_exact_select_dev = this
 *                               shard's k best under the statistics of all shards (Chan combination in rank order), sel DEVICE f64 [64][2][k]
 *                               (scores | global indices as doubles, -1 / NaN when the shard has fewer) -> all-gather -> sel_all [G][64][2][k] ->
 *                               pr_order_exact_merge_dev on every rank patches idx / score of the pass's queries (identical inputs, identical
 *                               results everywhere).  G <= 64. */
int pr_order_resolve_async_dev(pr_ctx* ctx, const void* q_sc, const void* db_sc, int sc_dtype, const void* q_m2, const void* db_m2, int m2_dtype,
                               double* mom_sc, double* mom_m2, int32_t m, int32_t n, int32_t q_row0, int32_t mask_width, double p_weight,
                               int32_t k, int32_t* idx, double* score);
int pr_order_resolve_dev(pr_ctx* ctx, const void* q_sc, const void* db_sc, int sc_dtype, const void* q_m2, const void* db_m2, int m2_dtype,
                         double* mom_sc, double* mom_m2, int32_t m, int32_t n, int32_t q_row0, int32_t mask_width, double p_weight, int32_t k,
                         int32_t* idx, double* score, int32_t* resolved);
int pr_order_flagged_count(pr_ctx* ctx, int32_t m, int32_t* count);   /* flagged queries of the last m-query pr_rerank_dev / pr_rerank_finish_dev (synchronises) */
int pr_order_exact_moments_dev(pr_ctx* ctx, const void* q_sc, const void* db_sc, int sc_dtype, const void* q_m2, const void* db_m2, int m2_dtype,
                               const double* mom_sc, const double* mom_m2, int32_t G_mom, int32_t m, int32_t n_local, int32_t offset,
                               int32_t last_pass /* non-zero: the caller runs no pass behind this one */, double* exact);
int pr_order_exact_select_dev(pr_ctx* ctx, const double* exact_all, int32_t G, int32_t m, int32_t n_local, int32_t q_row0, int32_t db_row0,
                              int32_t mask_width, double p_weight, int has_sc, int has_m2, int32_t k, int32_t offset, double* sel);
int pr_order_exact_merge_dev(pr_ctx* ctx, const double* sel_all, int32_t G, int32_t m, int32_t k, int32_t offset, int32_t* idx, double* score);
/* fp32 scores of pr_fuse_select_dev as doubles (the merge works on doubles): DEVICE score32 [count] -> score64 [count] */
int pr_widen_scores_dev(pr_ctx* ctx, const float* score32, int64_t count, double* score64);
/* k-way merge of the per-shard results of G shards (SURVEY.md §8-e collective B's second half): idx_all DEVICE [G][m][k],
 * score_all DEVICE f64 [G][m][k] -> idx [m][k], score [m][k] by (score, global index); -1 / NaN entries last.  PRECONDITION: every shard's list is ASCENDING by (score, index) with its missing entries (-1 / NaN) last - as
 * pr_fuse_select_dev and pr_rerank_dev write them; the merge walks one cursor per list and does not sort (an unsorted list gives a wrong
 * result, not an error).  G <= 64, k <= 128. */
int pr_merge_topk_dev(pr_ctx* ctx, const int32_t* idx_all, const double* score_all, int32_t G, int32_t m, int32_t k,
                      int32_t* idx, double* score);
/* Alignment of matched pairs: which variant of the query lines up best with its DB entry.  The reference computes the distance of every
 * variant and keeps only the minimum (processSC.m:22-33 with permute_sc :37-45, processM2DP.m:12-22, processDELIGHT.m:7-37); these calls
 * also return its position, in fp64 from the RAW signatures and in the reference's own formulation (the arithmetic of pr_rerank_dev:
 * the distance returned is, bit for bit, the channel distance pr_rerank_partial_dev writes into p5).  Variants, 0-based:
 *   SC      v = 2 s + r, s = 0..59 the sector shift, r the mirror flag: row v + 1 of sig_i (processSC.m:24-27) = permute_sc(hist, i, s + 1, r)
 *           - the entry's sector c against the query's sector (s + c) % 60 (r = 0) or (s - c) % 60 (r = 1)
 *   M2DP    v = 4 a + b, a the query's variant row and b the entry's (the 4 x 4 block of processM2DP.m:18, rows in test_m2dp.cpp:44-68 order)
 *   DELIGHT v = k, the row of Mut (processDELIGHT.m:2-5)
 * Ties go to the lowest variant (DELIGHT: the reference's strict `min_dist > ts`).  No variant: -1 with distance NaN for a zero-norm SC row
 * (processSC.m:16,19: every variant is NaN), +Inf for a DELIGHT pair without an occupied bin (the reference's untouched min_dist = Inf).
 * A pair whose idx is -1 or outside this shard's rows [db_row0, db_row0 + n_local) gets -1 / NaN: with the DB row-sharded, exactly one
 * shard fills each pair, and the shards' results combine by an element-wise max of the variants (fmax of the distances).
 * Stream-ordered on the context's stream, no allocation, no host synchronisation (can be captured in a hipGraph).
 * q_* / db_*: DEVICE raw signatures exactly as pr_rerank_dev takes them ([m][2400] / [n_local][2400], [4 m][384] / [4 n_local][384];
 * dtype PR_F64 | PR_F32); either descriptor pair may be NULL (its slots are -1 / NaN).  idx: DEVICE [m][k] GLOBAL DB rows, -1 = none.
 * variant / dist: DEVICE [m][k][4], slots in p5 channel order (SC structure, SC intensity, M2DP count, M2DP intensity). */
int pr_align_pairs_dev(pr_ctx* ctx, const void* q_sc, const void* db_sc, int sc_dtype, const void* q_m2, const void* db_m2, int m2_dtype,
                       int32_t m, int32_t n_local, int32_t db_row0, int32_t k, const int32_t* idx, int32_t* variant, double* dist);
/* The same for DELIGHT (processDELIGHT.m:7-37: chi-square over the bins with A + B > 0, mean over those bins, minimum over the 4
 * permutations): q DEVICE [16 m][256], db DEVICE [16 n_local][256]; variant / dist DEVICE [m][k]. */
int pr_delight_align_pairs_dev(pr_ctx* ctx, const void* q, const void* db, int dtype, int32_t m, int32_t n_local, int32_t db_row0, int32_t k,
                               const int32_t* idx, int32_t* variant, double* dist);

/* ---- the database row-sharded over several GPUs of one node (the reference is single-device MATLAB,
 * match_signatures/run_test.m:25-57 - this is that computation with hist2 split by rows) ---------------------------------------
 * pr_group_create: one context per entry of device_ids; with G > 1 distinct devices the two exchanges (row moments, per-shard top-k)
 * are ncclAllGather calls of ONE in-process RCCL communicator set (ncclCommInitAll; librccl.so.1 is dlopen'ed here, not linked),
 * enqueued on the compute streams between the kernels.  Device ids may repeat (several shards on one GPU - tests on a one-GPU box):
 * such a group exchanges with event-ordered device copies, since RCCL refuses duplicate devices.  PR_GROUP_EXCHANGE=rccl|copy overrides.
 * pr_group_set_database: hist2 (host f64, [n][2400] SC or [4n][384] M2DP); shard g holds rows [g n/G, (g+1) n/G) raw + packed.
 * pr_group_match_topk: run_test.m:26-57 for hist1 (host f64) against the sharded hist2: idx [m][k] GLOBAL 0-based rows (-1: none),
 * score [m][k] doubles; identical to pr_match_topk_f64 on the unsharded database (same arithmetic, Chan combination in rank order). */
typedef struct pr_group pr_group;
int pr_group_create(const int32_t* device_ids, int32_t G, pr_group** out);
void pr_group_destroy(pr_group* g);
const char* pr_group_last_error(const pr_group* g);     /* g may be NULL (creation errors) */
int32_t pr_group_size(const pr_group* g);
int pr_group_uses_rccl(const pr_group* g);
int32_t pr_group_rccl_ranks(const pr_group* g);         /* ncclCommCount of the group's communicator (0: the group exchanges by copies) */
int pr_group_set_exact_statistics(pr_group* g, int on);  /* pr_set_exact_statistics on every shard: all queries answered from their exact fp64 rows */
int32_t pr_group_last_flagged(const pr_group* g);       /* queries of the last pr_group_match_topk that were answered from their exact fp64 rows */
/* Phase times of a call, per shard (bench.py --via-group: what makes the first multi-GPU curve readable).  on != 0: every following
 * pr_group_match_topk records HIP events on every shard's stream between its phases; pr_group_last_timing waits for the last call's and
 * fills ms [G][PR_GROUP_PHASES] (cap = floats ms has room for), phases in this order:
 *   0 upload + pack(queries) | 1 all-pairs distances | 2 row moments | 3 all-gather A (moments) | 4 fp32 selection | 5 all-gather B (candidate
 *   lists) | 6 merge + fp64 re-evaluation | 7 all-gather C (evaluations) | 8 finish + order / containment checks | 9 exact rows of the flagged
 *   queries (count read back, then per pass: rows, all-gather D, selection, all-gather E, merge).
 * pr_group_create itself runs every exchange size of a one-query call on scratch buffers and checks that every rank's slice arrives in its
 * slot on every device (G > 1): a topology / RCCL problem fails there, with a message, not inside a step. */
#define PR_GROUP_PHASES 10
int pr_group_set_timing(pr_group* g, int on);
int pr_group_last_timing(pr_group* g, float* ms, int32_t cap);
int pr_group_set_database(pr_group* g, int type, const double* h2, int32_t n);
/* A database that grows (SC/test_sc.cpp:40-56 adds one signature row per keyframe; run_test.m:57 matches a frame against all earlier ones):
 * pr_group_set_database_growable = pr_group_set_database with room for extra_capacity more signatures on the LAST shard (whose rows end the
 * global numbering; its operand image is laid out for that capacity, pr_sigset_reserve); pr_group_append_database adds hist_new ([n_new][2400]
 * SC or [4 n_new][384] M2DP, host f64) there in place - no re-pack, no re-upload of what is resident - and the next pr_group_match_topk
 * sees n + n_new rows.  With one device this is the online loop of a single GPU through host buffers only. */
int pr_group_set_database_growable(pr_group* g, int type, const double* h2, int32_t n, int32_t extra_capacity);
int pr_group_append_database(pr_group* g, const double* hist_new, int32_t n_new);
int32_t pr_group_database_rows(const pr_group* g);
int pr_group_take_warnings(pr_group* g);                /* OR of the shards' pr_take_warnings (PR_WARN_* bits), then cleared */
int pr_group_match_topk(pr_group* g, const double* h1, int32_t m, int32_t mask_width, double p_weight, int32_t k, int32_t* idx,
                        double* score);

/* Device-buffer variants of the generators (same layouts as the host versions, pointers in HBM). */
int pr_sc_generate_dev(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N,
                       double max_rho, double* out);
int pr_m2dp_generate_dev(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N,
                         double max_rho, double* out);
int pr_delight_generate_dev(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N, double* out);
/* The generators with the clouds' PCA frames (utils/pts_align.h:7-46) supplied by the caller: the moments pass over the points is skipped
 * and only the binning pass runs (28 B per point once instead of twice).  frames: device [N][16] doubles = mean[3], the three
 * eigenvectors by ascending eigenvalue [9], 0, point count, then optionally the cloud's float intensity average (the reference's
 * sequential float sum in input order, SC.cpp:60-64 / M2DP.cpp:77-81, widened to double) and 1.0 where it is there.
 * pr_cloud_frames_dev writes them (asynchronously, on the context's streams; with inten != NULL the averages too), and
 * pr_pts_preprocess_gpu leaves them - averages included - beside the clouds it emits (pr_clouds_dev_frames).
 * frames_have_ave != 0: slots 14 of the frames hold the averages and the call is the binning pass alone; 0: the call computes them
 * (a chain of dependent float adds per cloud, beside the binning pass).  Same results, bit for bit, as the calls above.
 * pr_sc_generate_frames_dev with frames_have_ave != 0, and pr_delight_generate_frames_dev, are one launch without any allocation and
 * may be captured in a hipGraph (they synchronise the context's stream before they return, except while that stream is capturing).
 * pr_m2dp_generate_frames_dev allocates scratch and forks onto side streams: it cannot be captured. */
int pr_cloud_frames_dev(pr_ctx* ctx, const double* xyz, const float* inten /* may be NULL */, const int64_t* offs, int32_t N, double* frames);
int pr_sc_generate_frames_dev(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N, double max_rho,
                              const double* frames, int frames_have_ave, double* out);
int pr_m2dp_generate_frames_dev(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N, double max_rho,
                                const double* frames, int frames_have_ave, double* out);
int pr_delight_generate_frames_dev(pr_ctx* ctx, const double* xyz, const float* inten, const int64_t* offs, int32_t N,
                                   const double* frames, double* out);

/* ---- host-side rows a1/a2 (CPU in the reference too; no device, no context) ---------------------------- */
/* Relative pose of an SC match (no reference counterpart: the reference keeps no variant, processSC.m:31): from the two clouds' PCA
 * frames (utils/pts_align.h:7-46, the [16]-double layout pr_cloud_frames_dev writes) and the SC variant v = 2 s + r of the pair
 * (pr_align_pairs_dev, structure channel), T [c][3][4] = [R | t] maps points of the QUERY's camera frame into the DB entry's camera frame.
 * With D = 2 pi / 60 (SC.cpp:33-38): r = 0 turns the aligned y'z' plane by -s D, r = 1 reflects it with B = [[cos f, sin f], [sin f, -cos f]],
 * f = (s + 1) D; the height axis x' gets the sign sigma = det(E_db) det(E_q) det(B); R = E_db diag(sigma, B) E_q^T, t = mu_db - R mu_q
 * (DESIGN.md "Alignment").  An initial guess for ICP: the yaw is known to about half a sector (3 deg) where PCA's in-plane axes are
 * ambiguous, the translation is the alignment of the centroids.  PR_EINVAL (text: pr_last_error(NULL)) for a variant outside [0, 120) or
 * a frame of fewer than 3 points (slot 13). */
int pr_sc_relative_pose(const double* frames_q, const double* frames_db, const int32_t* variant, int32_t c, double* T);

/* Replaces pts_preprocess(poses_file, pts_file, incoming_id_file, lidarRange, clouds, polar_filter)
 * (utils/pts_preprocess.h:169-232, records PosesPts.h:5-40): sliding world-point window per pose, camera-frame
 * transform, range cut, voxel (polar_filter = 0, SC) or 1-degree polar (polar_filter = 1, M2DP) down-sampling with the
 * reference's point ORDER, and the incoming_id_file (written when non-NULL).  verbose prints the reference's lines. */
int pr_pts_preprocess(const char* poses_file, const char* pts_file, const char* incoming_id_file, double lidarRange,
                      int polar_filter, int verbose, pr_clouds** out);
/* The same on the GPU: identical clouds in identical point order (the order of libstdc++'s
 * std::unordered_map iteration, reproduced from the key insertion sequence), files parsed on the host.  Needs a context. */
int pr_pts_preprocess_gpu(pr_ctx* ctx, const char* poses_file, const char* pts_file, const char* incoming_id_file,
                          double lidarRange, int polar, int verbose, pr_clouds** out);
/* Iteration order of a std::unordered_map<int,...> after inserting the K distinct non-negative keys in this order
 * (order[t] = index of the t-th element); the host build of the routine the GPU pre-stage runs per cloud. */
int pr_hash_order(const int32_t* keys, int32_t K, int32_t* order);
int64_t pr_clouds_count(const pr_clouds* c);
const int64_t* pr_clouds_offs(const pr_clouds* c);      /* [N+1] */
const double* pr_clouds_xyz(const pr_clouds* c);        /* [offs[N]][3] camera frame */
const float* pr_clouds_inten(const pr_clouds* c);       /* [offs[N]] */
const int32_t* pr_clouds_ids(const pr_clouds* c);       /* [N] incoming ids */
double pr_clouds_avg_ms(const pr_clouds* c);           /* the reference's "average time" of pts_preprocess.h:221-225 (files already parsed) */
double pr_clouds_avg_pts(const pr_clouds* c);
/* Clouds made by pr_pts_preprocess_gpu also stay in HBM (device of that context) with their PCA frames, laid out as the host arrays
 * above, for pr_*_generate_frames_dev; NULL for clouds made on the host (and for an empty result).  Freed by pr_clouds_free. */
const double* pr_clouds_dev_xyz(const pr_clouds* c);
const float* pr_clouds_dev_inten(const pr_clouds* c);
const int64_t* pr_clouds_dev_offs(const pr_clouds* c);
const double* pr_clouds_dev_frames(const pr_clouds* c);  /* [N][16] */
/* The loop of SC/test_sc.cpp:40-56 / M2DP/test_m2dp.cpp:41-68 / DELIGHT/test_delight.cpp:41-56 over a pr_clouds object: type = PR_TYPE_*,
 * out = host [N][2400] | [4N][384] | [16N][256] (max_rho is ignored for DELIGHT).  Clouds that pr_pts_preprocess_gpu left in this
 * context's HBM are taken from there with their frames (no upload, binning pass only); any other pr_clouds goes the way of
 * pr_sc_generate / pr_m2dp_generate / pr_delight_generate from its host arrays.  Same signatures either way. */
int pr_generate_clouds(pr_ctx* ctx, int type, const pr_clouds* c, double max_rho, double* out);
void pr_clouds_free(pr_clouds* c);

/* ---- the pre-stage one keyframe at a time: a resident point window (window.hip) --------------------------
 * pr_pts_preprocess* need the two finished text files of a drive.  A pr_window holds the reference's "nearby" point set
 * (utils/pts_preprocess.h:135-216) in HBM instead: one push per keyframe, in this order: reset test (|translation column of
 * w2c| < 1.0 clears the set, the overflow flag and the warm-up counter), the keyframe's new world points are appended, the
 * first 30 pushes after a reset emit and prune nothing; every later push keeps the points with |p| < lidarRange in the
 * camera frame (strict; the others leave the set for good, the survivors keep their order), down-samples to the best point per
 * cell (polar = 0: voxel grid, smallest camera-y; polar = 1: 1 deg x 1 deg, smallest norm; ties: the earlier point) and emits
 * the cloud in the iteration order of the reference's std::unordered_map.  Points, order, PCA frame and float intensity
 * average are bit for bit those of pr_pts_preprocess_gpu over the same drive.
 *
 *   pr_window_create    point_capacity: most points the set holds at once (alive + one keyframe's new ones, < 2^30);
 *                       max_new_points: most new points of one push (<= point_capacity); max_out_points: most points of an
 *                       emitted cloud.  All device memory a push needs is allocated here.  The window is bound to ctx and its
 *                       stream and must be destroyed before ctx.
 *   pr_window_push_dev  stream-ordered, no host decision, no read-back, nothing allocated; the launch geometry depends on the
 *                       create capacities only, so a captured push serves every keyframe.  EVERY argument is device memory:
 *                       pose12 [12] the row-major 3x4 w2c, xyz_new [max_new][3] world points, inten_new [max_new], n_new_dev
 *                       [1] int32 (clamped to 0 .. max_new; max_new <= max_new_points).  Outputs: out_xyz [max_out_points][3],
 *                       out_inten [max_out_points], out_offs [2] int64 = {0, n_out} and out_frame [16] - what
 *                       pr_sc_generate_frames_dev / pr_m2dp_generate_frames_dev / pr_delight_generate_frames_dev take with
 *                       N = 1 and frames_have_ave = 1; a push that emits nothing writes {0, 0} and a zero frame.
 *                       info [4] int32 = {emitted 0/1, n_out, points alive after the push, flags}.
 *   OVERFLOW cannot be an error without a read-back, so it is a FLAG: when the alive set plus the new points exceeds
 *   point_capacity (or n_new exceeds max_new) the excess NEW points are dropped, when the emitted cloud exceeds max_out_points
 *   the excess OUTPUT points are dropped, and PR_WINDOW_OVERFLOW is set in info[3] of that push and of every later one until
 *   the next reset (a reset pose or pr_window_reset).  From the first flagged push on the clouds are no longer the
 *   reference's.  PR_WINDOW_ORDER_GLOBAL in info[3] (this push only) says that the order step kept its scratch in HBM
 *   rather than in LDS (more than about 2 x 10^4 cells occupied).
 *   pr_window_push      the host form: host pose, points and count in, host cloud (out_xyz / out_inten hold max_out_points),
 *                       n_out, frame and info out; uploads, runs the same device path, synchronises.  n_new > max_new_points
 *                       is PR_EINVAL here.
 *   pr_window_reset     clears the set, the flag and the warm-up counter (stream-ordered).
 *   pr_window_count     synchronising read of the alive count (diagnostics).
 * PR_EINVAL (text: pr_last_error(ctx)) for a NULL handle or pointer, a non-positive capacity, max_new_points > point_capacity,
 * max_new outside 1 .. max_new_points, polar other than 0 / 1, a lidarRange that is not finite and positive. */
typedef struct pr_window pr_window;
enum { PR_WINDOW_OVERFLOW = 1, PR_WINDOW_ORDER_GLOBAL = 2 };
int pr_window_create(pr_ctx* ctx, double lidarRange, int polar, int32_t point_capacity, int32_t max_new_points, int32_t max_out_points,
                     pr_window** out);
void pr_window_destroy(pr_window* w);
int pr_window_reset(pr_window* w);
int pr_window_count(pr_window* w, int32_t* n_alive);
int pr_window_push_dev(pr_window* w, const double* pose12, const double* xyz_new, const float* inten_new, const int32_t* n_new_dev,
                       int32_t max_new, double* out_xyz, float* out_inten, int64_t* out_offs, double* out_frame, int32_t* info);
int pr_window_push(pr_window* w, const double* pose12, const double* xyz_new, const float* inten_new, int32_t n_new, double* out_xyz,
                   float* out_inten, int32_t* n_out, double* out_frame, int32_t* info);

/* Signature matrix text I/O: writer = `ofstream << Eigen::MatrixXd` (test_sc.cpp:63-66, test_m2dp.cpp:83-86);
 * reader = whitespace-tolerant load (test_kitti.m:26); *out is released with pr_free. */
int pr_write_signatures(const char* path, const double* sig, int64_t rows, int64_t cols);
int pr_read_signatures(const char* path, double** out, int64_t* rows, int64_t* cols);
void pr_free(void* p);
/* Binary side-car of the same matrices (no reference counterpart): 32-byte header + row-major data,
 * dtype PR_F64 or PR_F32 on disk; the reader always returns f64.  The executables pick it by the ".bin" suffix. */
int pr_write_signatures_bin(const char* path, const double* sig, int64_t rows, int64_t cols, int dtype);
int pr_read_signatures_bin(const char* path, double** out, int64_t* rows, int64_t* cols);
/* PosesPts.h:12-24 / :36-39 record writers (the producer side, OutputWrapperSODSO.cpp:24-31). */
int pr_write_poses(const char* path, const int32_t* ids, const double* w2c, int64_t n);
int pr_write_points(const char* path, const int32_t* ids, const double* xyz, const float* inten, int64_t n);
/* Replaces the evaluation half of run_test(type, hist1, hist2, gt1, gt2, loop_diff, mask_width) (match_signatures/run_test.m:3-22 ground-truth
 * loop pairs, :58-85 precision / recall sweep): diff_v / diff_idx [m] = the per-query best score and 0-based index (run_test.m:57),
 * gt1 [m][cols], gt2 [n][cols] positions.  auc = trapz(recall, precision), top_recall = recall at the last 100 %-precision point,
 * lp_detected (optional) [m][2] receives the *n_detected pairs (query, match) of that prefix.  A diff_idx of -1 (no finite candidate) is
 * read as index 0: MATLAB's min over an all-NaN / all-Inf row returns index 1 (run_test.m:57). */
int pr_precision_recall(const double* diff_v, const int32_t* diff_idx, int32_t m, const double* gt1, const double* gt2, int32_t n,
                        int32_t cols, double loop_diff, int32_t mask_width, double* auc, double* top_recall, int32_t* lp_detected,
                        int32_t* n_detected);
/* The same evaluation on the device (eval.hip), bit for bit the reference's arithmetic: squared distances
 * ((0 + t_0^2) + t_1^2) + ... with every product and sum rounded, the FIRST minimum per query (strict `min_diff > diff` from +Inf / -1: a NaN
 * or +Inf distance never wins), a stable ascending rank of diff_v with NaN after +Inf, IEEE divisions, and the trapz sum added in index order.
 * cols <= 768.  m = 0 and n = 0 are valid.  PR_EINVAL (text: pr_last_error) for negative sizes, cols < 1 or a NULL required pointer.
 *   pr_ground_truth_pairs_dev  run_test.m:3-22.  d_gt1 [m][cols], d_gt2 [n][cols] DEVICE.  Outputs (DEVICE, any may be NULL): d_min_j [m]
 *                       the nearest unmasked row (-1: none), d_min_d [m] its squared distance (+Inf: none), d_lp_gt [m][2] the pairs
 *                       (i, min_j) with min_d < loop_diff^2 in ascending i (the first *d_n_gt are written), d_n_gt [1].
 *   pr_precision_recall_dev  run_test.m:3-22 + :58-85.  d_diff_v (f64) / d_diff_idx (i32): element i at [i * ld], so that column 0 of a
 *                       matcher's [m][k] result is read in place with ld = k.  A rank is a true positive when its index b (-1 read as 0)
 *                       is < n and the squared distance of gt1[a], gt2[b] is < loop_diff^2.  d_scalars: DEVICE record
 *                       {f64 auc, f64 top_recall, i32 n_gt, i32 n_detected} (24 bytes).  Optional DEVICE outputs: d_lp_gt [m][2],
 *                       d_lp_detected [m][2] (the first n_detected pairs (query, match) are written), d_precision [m], d_recall [m].
 *   pr_trapz_dev        *d_auc = sum over i < m - 1 of ((recall[i+1] - recall[i]) * (precision[i] + precision[i+1])) / 2, added in that
 *                       order from 0.0 (run_test.m:84 as the oracle evaluates it).
 *                       All three are stream-ordered on the context's stream without host read-back; their scratch is grow-only in the
 *                       context: a call whose shapes an earlier call covered allocates nothing and can be captured in a hipGraph.
 *   pr_ground_truth_pairs / pr_precision_recall_gpu  the host-buffer forms: upload, the calls above, read back, synchronise.  lp_gt and
 *                       lp_detected are [m][2] (optional, like n_gt, n_detected, precision [m], recall [m], min_j, min_d).
 *   pr_eval_tile_rows   gt2 rows a workgroup stages at a time.  pr_set_eval_path: tests and experiments - split 0: by shape, 1: every
 *                       workgroup scans all of gt2, 2: per-range partials and a combining launch; queries_per_lane 0: by shape, 1 or 4.
 *                       The results do not depend on either. */
int pr_ground_truth_pairs_dev(pr_ctx* ctx, const double* d_gt1, int32_t m, const double* d_gt2, int32_t n, int32_t cols, double loop_diff,
                              int32_t mask_width, int32_t* d_min_j, double* d_min_d, int32_t* d_lp_gt, int32_t* d_n_gt);
int pr_precision_recall_dev(pr_ctx* ctx, const double* d_diff_v, const int32_t* d_diff_idx, int32_t ld, int32_t m, const double* d_gt1,
                            const double* d_gt2, int32_t n, int32_t cols, double loop_diff, int32_t mask_width, void* d_scalars,
                            int32_t* d_lp_gt, int32_t* d_lp_detected, double* d_precision, double* d_recall);
int pr_trapz_dev(pr_ctx* ctx, const double* d_recall, const double* d_precision, int32_t m, double* d_auc);
int pr_ground_truth_pairs(pr_ctx* ctx, const double* gt1, int32_t m, const double* gt2, int32_t n, int32_t cols, double loop_diff,
                          int32_t mask_width, int32_t* min_j, double* min_d, int32_t* lp_gt, int32_t* n_gt);
int pr_precision_recall_gpu(pr_ctx* ctx, const double* diff_v, const int32_t* diff_idx, int32_t m, const double* gt1, const double* gt2,
                            int32_t n, int32_t cols, double loop_diff, int32_t mask_width, double* auc, double* top_recall, int32_t* lp_gt,
                            int32_t* n_gt, int32_t* lp_detected, int32_t* n_detected, double* precision, double* recall);
int32_t pr_eval_tile_rows(void);
int pr_set_eval_path(pr_ctx* ctx, int split, int queries_per_lane);

/* ---- ICP refinement and verification of matched cloud pairs (icp.hip; no reference counterpart) --------------------
 * Point-to-point ICP in fp64 of a source cloud (the query keyframe) onto a target cloud (the DB entry) from a seed T0 = [R | t], e.g.
 * pr_sc_relative_pose's.  Clouds are CSR sets as pr_sc_generate_dev takes them (xyz [offs[N]][3] f64, offs [N + 1] i64), one set for the
 * queries and one for the DB (they may be the same); pair i is (pair_src[i], pair_dst[i]), -1 = none; a source cloud may appear in several
 * pairs.  Per iteration: p' = ((R00 x + R01 y) + R02 z) + t0 (every product and sum rounded), the nearest target point by
 * d2 = ((dx dx) + dy dy) + dz dz with the FIRST minimum (strict `best > d2` from (+Inf, -1): a NaN or +Inf distance never wins), inliers
 * d2 < max_corr^2, Kabsch on the inliers, R <- dR R, t <- dR t + dt.  It stops when |rmse - rmse_prev| < tol_rmse and |fitness -
 * fitness_prev| < tol_fitness (PR_ICP_CONVERGED), with fewer than min_inliers inliers (PR_ICP_TOO_FEW) or collinear ones (second singular
 * value of H <= 1e-12 x the first: PR_ICP_DEGENERATE) - T is then the last one a valid update produced, T0 if none -, or after max_iter
 * updates (PR_ICP_MAX_ITER).  One more correspondence pass under the final T gives the reported fitness = n_inl / |source|, rmse =
 * sqrt(sum of the inliers' d2 / n_inl) (0 without inliers) and n_inl.  A pair of -1: PR_ICP_NO_PAIR, T0, zeros.
 *   pr_icp_nn_dev     one correspondence pass for c pairs under d_T [c][3][4].  DEVICE outputs: d_out_offs [c + 1] the prefix of the
 *                     pairs' source sizes (0 for a pair of -1), d_nn_idx (-1: none) and d_nn_d2 (+Inf: none) [out_offs[c]].
 *   pr_icp_pairs_dev  the refinement.  DEVICE outputs d_T_out [c][3][4] (may be d_T0) and d_stats [c].
 *                     Both are stream-ordered on the context's stream without host read-back, a fixed number of launches whatever the data
 *                     (a finished pair's launches return at once); the scratch is grow-only in the context: a call whose shapes an earlier
 *                     call covered allocates nothing and can be captured in a hipGraph.  max_src_pts / max_dst_pts: the most points a
 *                     source / target cloud of a pair has - the launch geometry and the scratch are sized by them, and a cloud is read
 *                     up to that many points.  c <= 65535, clouds of up to 2^26 points.
 *   pr_icp_nn / pr_icp_pairs  the host-buffer forms: upload, the calls above (bounds taken from the offsets), read back, synchronise.
 *   pr_icp_tile_rows  target rows a workgroup stages at a time.  pr_set_icp_path: tests and experiments - split 0: by shape, 1: every
 *                     workgroup scans the whole target, 2: the target split across workgroups and a combining launch.  Indices and d2
 *                     bits do not depend on it.
 * PR_EINVAL (text: pr_last_error) before any device is touched for negative sizes, a NULL required pointer, max_iter < 0, max_corr <= 0
 * or not finite, min_inliers < 3, no context.  c = 0 and empty clouds are valid. */
#define PR_ICP_CONVERGED 0
#define PR_ICP_MAX_ITER 1
#define PR_ICP_TOO_FEW 2
#define PR_ICP_DEGENERATE 3
#define PR_ICP_NO_PAIR 4
typedef struct pr_icp_stats { double fitness, rmse; int32_t n_inl, iters, status, pad; } pr_icp_stats;
int pr_icp_nn_dev(pr_ctx* ctx, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_xyz_db, const int64_t* d_offs_db,
                  int32_t Ndb, const int32_t* d_pair_src, const int32_t* d_pair_dst, int32_t c, const double* d_T, int32_t max_src_pts,
                  int32_t max_dst_pts, int64_t* d_out_offs, int32_t* d_nn_idx, double* d_nn_d2);
int pr_icp_pairs_dev(pr_ctx* ctx, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_xyz_db, const int64_t* d_offs_db,
                     int32_t Ndb, const int32_t* d_pair_src, const int32_t* d_pair_dst, int32_t c, const double* d_T0, int32_t max_src_pts,
                     int32_t max_dst_pts, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers,
                     double* d_T_out, pr_icp_stats* d_stats);
int pr_icp_nn(pr_ctx* ctx, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const double* xyz_db, const int64_t* offs_db, int32_t Ndb,
              const int32_t* pair_src, const int32_t* pair_dst, int32_t c, const double* T, int64_t* out_offs, int32_t* nn_idx, double* nn_d2);
int pr_icp_pairs(pr_ctx* ctx, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const double* xyz_db, const int64_t* offs_db, int32_t Ndb,
                 const int32_t* pair_src, const int32_t* pair_dst, int32_t c, const double* T0, int32_t max_iter, double max_corr,
                 double tol_rmse, double tol_fitness, int32_t min_inliers, double* T_out, pr_icp_stats* stats);
int32_t pr_icp_tile_rows(void);
int pr_set_icp_path(pr_ctx* ctx, int split);

/* ---- the exact uniform-grid correspondence search of the ICP stage (icp_grid.hip; no reference counterpart) ----------
 * Only correspondences with d2 < max_corr^2 enter an update or a statistic.  PR_ICP_SEARCH_GRID finds exactly those - the same indices,
 * the same d2 bits - from a uniform grid over the finite target points instead of the scan of every target point: built once per call and
 * per pair slot (cell edge h = max(max_corr (1 + 2^-10), largest extent / G), on the device), probed in the 27 cells around every
 * transformed source point.  With it pr_icp_pairs_dev (and everything built on it: pr_icp_pairs, pr_verify_pairs_dev) returns the bytes
 * PR_ICP_SEARCH_BRUTE returns under pr_set_icp_path(ctx, 2); against the other brute-force geometries status, iters, n_inl and fitness
 * are equal and rmse, R, t differ by the order of the sums only ("What is bit-reproducible").  The launch contract is the
 * brute-force one: stream-ordered, no read-back, a fixed number of launches for given (c, max_src_pts, max_dst_pts, max_iter), scratch
 * grow-only in the context (per pair slot: cells x 4 B + max_dst_pts x 4 B + a box; cells = the power of two >= 2 max_dst_pts, halved
 * until c slots hold at most 256 MiB of cell words; PR_ENOMEM if the allocation fails).  A coarser grid is slower, never wrong.
 *   pr_set_icp_search / pr_get_icp_search  the context's mode: PR_ICP_SEARCH_BRUTE (the default; nothing of the calls above changes) or
 *                     PR_ICP_SEARCH_GRID.  PR_ICP_SEARCH=brute|grid in the environment gives the initial value (read at pr_create).
 *                     PR_EINVAL for another mode (text: pr_last_error) or a NULL context.  pr_icp_nn_dev is brute force in either mode.
 *   pr_icp_nn_radius_dev  one correspondence pass as pr_icp_nn_dev's, for every source point the brute-force result (j, d2) where
 *                     d2 < max_corr^2 and (-1, +Inf) elsewhere - in BRUTE mode the scan followed by a mask, in GRID mode the grid: the two
 *                     agree bit for bit on every input (first minimum = the smaller j among equal d2; a NaN or +Inf distance never wins;
 *                     a non-finite target point is not in the grid, a source point whose p' is non-finite or more than one cell outside
 *                     the targets' box has no correspondent).  PR_EINVAL as pr_icp_nn_dev, and for max_corr <= 0 or not finite.
 *   pr_icp_nn_radius  the host-buffer form. */
#define PR_ICP_SEARCH_BRUTE 0
#define PR_ICP_SEARCH_GRID 1
int pr_set_icp_search(pr_ctx* ctx, int mode);
int pr_get_icp_search(pr_ctx* ctx);
int pr_icp_nn_radius_dev(pr_ctx* ctx, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_xyz_db, const int64_t* d_offs_db,
                         int32_t Ndb, const int32_t* d_pair_src, const int32_t* d_pair_dst, int32_t c, const double* d_T, int32_t max_src_pts,
                         int32_t max_dst_pts, double max_corr, int64_t* d_out_offs, int32_t* d_nn_idx, double* d_nn_d2);
int pr_icp_nn_radius(pr_ctx* ctx, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const double* xyz_db, const int64_t* offs_db, int32_t Ndb,
                     const int32_t* pair_src, const int32_t* pair_dst, int32_t c, const double* T, double max_corr, int64_t* out_offs,
                     int32_t* nn_idx, double* nn_d2);

/* ---- pose seeds for every matcher type and the stream-ordered verify chain (pose.hip; no reference counterpart) ------
 * The seed of a matched pair from the two clouds' PCA frames ([16] doubles as pr_cloud_frames_dev writes them: mean, E = [v0 v1 v2] by
 * ascending eigenvalue, 0, point count) and the pair's best-aligning variant (pr_align_pairs_dev / pr_delight_align_pairs_dev):
 * R = E_db S E_q^T, t = mu_db - R mu_q, T = [R | t] maps points of the QUERY's camera frame into the DB entry's.
 *   PR_POSE_SC       v = 2 s + r < 120: S = diag(sigma, B), exactly pr_sc_relative_pose (the same operations in the same order)
 *   PR_POSE_M2DP     v = 4 a + b < 16: S0 = D_b D_a, D_u = diag(dx, dy, dx dy) the variant row u of test_m2dp.cpp:46-57,
 *                    (dx, dy) = (-1,-1), (-1,+1), (+1,-1), (+1,+1) for u = 0 .. 3
 *   PR_POSE_DELIGHT  v = k < 4: S0 = I, diag(-1,1,-1), diag(1,-1,-1), diag(-1,-1,1): the octant XOR 0, 5, 6, 3 of Mut's row k
 *                    (processDELIGHT.m:2-5; octant = 4 (z > 0) + 2 (y > 0) + (x > 0), DELIGHT.cpp:21)
 *   M2DP and DELIGHT: S = diag(sigma, 1, 1) S0 with sigma = sign(det E_db) sign(det E_q): R is proper whatever the eigen-solver's handedness.
 * pr_relative_pose      the host form (no context): frames_q / frames_db [c][16], variant [c] -> T [c][3][4].  PR_EINVAL (text:
 *                       pr_last_error(NULL)) for an unknown type, a variant outside the type's range or a frame of fewer than 3 points.
 * pr_relative_pose_dev  one lane per slot of [m][k][H]: hypothesis h of pair p = q k + j reads d_idx[p] (GLOBAL DB row, frame
 *                       d_idx[p] - db_row0 of d_frames_db [n_local][16]), d_variant[p * variant_stride + h] and frame q of d_frames_q
 *                       [m][16]; DEVICE outputs d_T0 [m k H][3][4], d_pair_src (= q) and d_pair_dst (= the local DB row) [m k H] as
 *                       pr_icp_pairs_dev takes them.  A slot gets (-1, -1) and [I | 0] - PR_ICP_NO_PAIR downstream - for idx < 0 or
 *                       outside [db_row0, db_row0 + n_local), a variant that is negative or outside the type's range, a frame of fewer than
 *                       3 points or with a non-finite entry, and a hypothesis 1 whose variant equals hypothesis 0's.  variant_stride: ints
 *                       between two pairs' variants (1 for DELIGHT's [m][k]; 4 for the [m][k][4] of pr_align_pairs_dev, whose slots 0, 1
 *                       are SC's two channels and 2, 3 M2DP's: pass d_variant + 2 for those).  H = 1 | 2 (1 for DELIGHT), m k H <= 65535.
 * pr_verify_select_dev  one lane per pair: of the pair's H refined hypotheses (d_T_h [c][H][3][4], d_stats_h [c][H]) the one whose status
 *                       is converged or max_iter with the larger fitness, then the smaller rmse, then the smaller h (IEEE comparisons; a
 *                       NaN never wins over a number); hypothesis 0 when none qualifies.  DEVICE outputs d_T [c][3][4], d_stats [c],
 *                       d_hyp [c] and d_accepted [c] = qualified && fitness >= min_fitness && rmse <= max_rmse.  Public because a caller
 *                       who refines hypotheses of its own (other seeds, more than two, several pr_icp_pairs_dev calls) needs the same
 *                       rule on the device, and because the rule can only be tested on chosen statistics through it; H >= 1.
 * pr_verify_pairs_dev   the chain: seed -> pr_icp_pairs_dev over the m k H slots (query cloud q of the query set onto DB cloud
 *                       idx - db_row0 of the DB set) -> select, on the context's stream: a fixed number of launches, no read-back, the
 *                       scratch grow-only in the context - a call whose shapes an earlier call covered allocates nothing and can be
 *                       captured in a hipGraph (the first call of a context uploads the SC angle table and cannot).
 * PR_EINVAL before any device is touched as for the ICP calls, and for an unknown type, H outside 1 | 2, variant_stride < H,
 * m k H > 65535, a NaN threshold. */
#define PR_POSE_SC 0
#define PR_POSE_M2DP 1
#define PR_POSE_DELIGHT 2
int pr_relative_pose(int type, const double* frames_q, const double* frames_db, const int32_t* variant, int32_t c, double* T);
int pr_relative_pose_dev(pr_ctx* ctx, int type, const double* d_frames_q, int32_t m, const double* d_frames_db, int32_t n_local, int32_t db_row0,
                         int32_t k, const int32_t* d_idx, const int32_t* d_variant, int32_t variant_stride, int32_t H, double* d_T0,
                         int32_t* d_pair_src, int32_t* d_pair_dst);
int pr_verify_select_dev(pr_ctx* ctx, const double* d_T_h, const pr_icp_stats* d_stats_h, int32_t c, int32_t H, double min_fitness, double max_rmse,
                         double* d_T, pr_icp_stats* d_stats, uint8_t* d_accepted, int32_t* d_hyp);
int pr_verify_pairs_dev(pr_ctx* ctx, int type, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_xyz_db,
                        const int64_t* d_offs_db, int32_t Ndb, const double* d_frames_q, const double* d_frames_db, int32_t m, int32_t n_local,
                        int32_t db_row0, int32_t k, const int32_t* d_idx, const int32_t* d_variant, int32_t variant_stride, int32_t H,
                        int32_t max_src_pts, int32_t max_dst_pts, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness,
                        int32_t min_inliers, double min_fitness, double max_rmse, double* d_T, pr_icp_stats* d_stats, uint8_t* d_accepted,
                        int32_t* d_hyp);

/* ---- the resident keyframe map: a CSR set of keyframe clouds that grows on the stream (map.hip) ----------------------
 * pr_verify_pairs_dev needs the clouds and PCA frames of every earlier keyframe as one CSR set.  A pr_map keeps that set while a drive
 * runs, over CALLER-OWNED device buffers in the layouts the rest of this header takes (pr_map_buffers): xyz [point_capacity][3] f64,
 * inten [point_capacity] f32, offs [keyframe_capacity + 1] i64, frames [keyframe_capacity][16] f64 (as pr_cloud_frames_dev / a window push
 * writes them, intensity-average slots included), poses [keyframe_capacity][12] f64 (w2c), ids [keyframe_capacity] i32 and
 * state [4] i32 = {keyframes, flags, 0, 0}.  The addresses never change, so a graph captured around an append or a verify is replayed
 * for every keyframe, and every stream-ordered call of this header reads the map in place (xyz + offs as a CSR set of keyframe_capacity
 * clouds, frames as its [n][16] frames).
 *
 *   pr_map_create      binds the buffers (they must outlive the map), allocates the plan scratch (sized by max_append: the most clouds of
 *                      one append) and zeroes offs, frames and state.  max_cloud_points: most points of a stored cloud (<= point_capacity).
 *                      The map is bound to ctx and its stream and must be destroyed before ctx.  pr_map_destroy frees the handle and its
 *                      scratch, never the buffers.
 *   pr_map_append_dev  stream-ordered, no host decision, no read-back, nothing allocated: three launches (plan, copy, commit) whose
 *                      geometry depends on N, max_points and the create capacities only, so one captured append serves every keyframe.
 *                      EVERY argument is device memory: cloud i is the points [d_offs[i], d_offs[i + 1]) of d_xyz / d_inten (d_offs[0]
 *                      need not be 0; a negative size counts as 0), d_frames [N][16], d_poses [N][12] or NULL (zeros are stored), d_ids
 *                      [N] or NULL (-1), d_emitted [>= 1] or NULL, d_info [4].  max_points: the most points the N clouds hold together -
 *                      one copy lane per point; values above max_cloud_points x N are clamped.  After a window push:
 *                      pr_map_append_dev(map, out_xyz, out_inten, out_offs, out_frame, pose, id, info_of_the_push, 1, max_out_points, info).
 *     The rule, decided on the device.  d_emitted != NULL and d_emitted[0] == 0: nothing happens, info = {0, -1, keyframes, flags}.
 *     Otherwise the N clouds are taken in order.  A cloud that finds no free row (keyframes == keyframe_capacity) is not appended and
 *     PR_MAP_OVERFLOW is set.  A cloud with a free row ALWAYS consumes it - the map stays row for row in step with a signature database
 *     that grows beside it - and its pose and id are stored; its points and frame are stored too unless it has more than
 *     max_cloud_points points, its points do not fit into what is left of point_capacity, or they lie beyond the call's max_points:
 *     then the row holds an EMPTY cloud and a ZERO frame (never a truncated cloud under the full cloud's frame) and
 *     PR_MAP_OVERFLOW | PR_MAP_DROPPED is set.  info = {clouds appended, first row or -1, keyframes after, flags}: PR_MAP_OVERFLOW stays
 *     set (in state[1] and in every later info) until pr_map_reset, PR_MAP_DROPPED is reported by the call that dropped.
 *     Between calls: offs[0] = 0 and offs ascends over rows 0 .. keyframes; every row >= keyframes has an all-zero frame, so
 *     pr_relative_pose_dev turns a candidate there into PR_ICP_NO_PAIR, and its offs read as an empty or negative size, which the ICP
 *     kernels clamp to 0.  Nothing is written outside the seven buffers' stated extents or to a row >= keyframe_capacity.
 *   pr_map_append      the host form: host arrays of the same meaning (info [4] host), uploads, runs the device path, synchronises.
 *   pr_map_reset       zeroes offs, frames and state (stream-ordered).
 *   pr_map_count       synchronising read of keyframes, stored points and the flags (diagnostics).
 *   pr_map_verify_dev  pr_verify_pairs_dev with the map as the DB set: Ndb = n_local = keyframe_capacity, db_row0 = 0, max_dst_pts =
 *                      max_cloud_points, d_idx = rows of the map; the same launches, scratch and capturability, no arithmetic of its own.
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, buffer or required pointer, a non-positive capacity,
 * max_cloud_points > point_capacity, max_cloud_points x max_append >= 2^38, N outside 0 .. max_append, a negative max_points.  N = 0 is
 * valid. */
typedef struct pr_map pr_map;
typedef struct pr_map_buffers { double* xyz; float* inten; int64_t* offs; double* frames; double* poses; int32_t* ids; int32_t* state; } pr_map_buffers;
enum { PR_MAP_OVERFLOW = 1, PR_MAP_DROPPED = 2 };
int pr_map_create(pr_ctx* ctx, const pr_map_buffers* buffers, int32_t keyframe_capacity, int64_t point_capacity, int32_t max_cloud_points,
                  int32_t max_append, pr_map** out);
void pr_map_destroy(pr_map* m);
int pr_map_reset(pr_map* m);
int pr_map_count(pr_map* m, int32_t* keyframes, int64_t* points, int32_t* flags);
int pr_map_append_dev(pr_map* m, const double* d_xyz, const float* d_inten, const int64_t* d_offs, const double* d_frames, const double* d_poses,
                      const int32_t* d_ids, const int32_t* d_emitted, int32_t N, int64_t max_points, int32_t* d_info);
int pr_map_append(pr_map* m, const double* xyz, const float* inten, const int64_t* offs, const double* frames, const double* poses,
                  const int32_t* ids, const int32_t* emitted, int32_t N, int32_t* info);
int pr_map_verify_dev(pr_map* m, int type, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_frames_q, int32_t mq,
                      int32_t k, const int32_t* d_idx, const int32_t* d_variant, int32_t variant_stride, int32_t H, int32_t max_src_pts,
                      int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers, double min_fitness,
                      double max_rmse, double* d_T, pr_icp_stats* d_stats, uint8_t* d_accepted, int32_t* d_hyp);

/* ---- the online signature database: raw SC or M2DP rows with a device-side count, matched exactly in fp64 (online.hip) --
 * A pr_sigset takes its row count from the host, so a captured match is frozen at the count it was captured with.  A pr_online is the
 * sibling of pr_map for signatures: the RAW rows of the keyframes seen so far over CALLER-OWNED device buffers (pr_online_buffers):
 * sig [capacity * rows_per_sig][sig_len] f64 (1 x 2400 for PR_TYPE_SC, 4 x 384 for PR_TYPE_M2DP, the layouts pr_align_pairs_dev takes)
 * and state [4] i32 = {count, flags, 0, 0}.  The addresses never change and every launch's geometry depends on capacity and max_k
 * only, so ONE captured match + append serves every keyframe of a drive, whatever the count, and pr_align_pairs_dev reads the rows in
 * place (n_local = capacity, db_row0 = 0: every idx a match returns is below the count).  It is for drives (thousands of rows: the
 * direct pair formulation walks all 120 variants of every entry), not for a 100k database, and it is exact by construction: no order flags, no
 * containment check.
 *
 *   pr_online_create      binds the buffers (they must outlive the handle), allocates ALL scratch (the distance rows [2][capacity], the
 *                         per-workgroup partial sums, the statistics, the staging of the host form) and zeroes state.  No later call
 *                         allocates.  The handle is bound to ctx and its stream and must be destroyed before ctx; pr_online_destroy
 *                         frees the handle and its scratch, never the buffers.  1 <= max_k <= 128.
 *   pr_online_match_dev   stream-ordered, no host decision, no read-back: three launches (rows, stats, select).  d_sig: the query's
 *                         signature, DEVICE [rows_per_sig][sig_len] f64; d_emitted DEVICE [>= 1] or NULL; d_idx [k] i32, d_score [k]
 *                         f64; d_rows DEVICE [2][capacity] f64 or NULL.
 *     The rule, decided on the device.  d_emitted != NULL and d_emitted[0] == 0: d_idx[0 .. k) = -1, d_score = NaN, nothing else
 *     happens.  Otherwise, with n = state[0]: the two channel distances of the query to every row j < n in the reference's own pair
 *     formulation in fp64 (processSC.m:15-33 / processM2DP.m:12-22: the device functions the re-evaluation and pr_align_pairs_dev use,
 *     so a duplicated row gives identical bits); the row statistics of normalize(.,2) (NaN left out, N - 1; the mean from ordered partial
 *     sums, the deviation by a second pass about it: scores within 1e-9 of the fp64 restatement); fused_j = p_weight z_p + z_i;
 *     +Inf where |n - j| < mask_width - the query is row n, the row it will get; the k smallest by (score, index), NaN never selected,
 *     missing slots -1 / NaN.  With n < 2 there are no statistics and every slot is -1 / NaN, masked or not.  d_rows, when given,
 *     receives the distances: the first n of each half.  1 <= k <= max_k.
 *   pr_online_append_dev  stream-ordered, one launch.  d_emitted off: info = {0, -1, count, flags}.  Otherwise the signature goes to row
 *                         count and count + 1 is committed; at count == capacity nothing is stored and PR_ONLINE_OVERFLOW is set (in
 *                         state[1] and every later info) until pr_online_reset.  d_info DEVICE [4] = {appended, row or -1, count after,
 *                         flags}.  Nothing is written outside the two buffers' stated extents.
 *   pr_online_append      the host form: sig host [rows_per_sig][sig_len], info host [4]; uploads, runs the device path, synchronises.
 *   pr_online_reset       zeroes state (stream-ordered).    pr_online_count   synchronising read of count and flags (diagnostics).
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, buffer or required pointer, a type other than
 * PR_TYPE_SC | PR_TYPE_M2DP, capacity outside 1 .. PR_MAX_SIGS, max_k or k out of range, a non-finite p_weight, mask_width < 0. */
typedef struct pr_online pr_online;
typedef struct pr_online_buffers { double* sig; int32_t* state; } pr_online_buffers;
#define PR_ONLINE_OVERFLOW 1
int pr_online_create(pr_ctx* ctx, int type, const pr_online_buffers* buffers, int32_t capacity, int32_t max_k, pr_online** out);
void pr_online_destroy(pr_online* o);
int pr_online_reset(pr_online* o);
int pr_online_count(pr_online* o, int32_t* count, int32_t* flags);
int pr_online_match_dev(pr_online* o, const double* d_sig, const int32_t* d_emitted, int32_t mask_width, double p_weight, int32_t k,
                        int32_t* d_idx, double* d_score, double* d_rows);
int pr_online_append_dev(pr_online* o, const double* d_sig, const int32_t* d_emitted, int32_t* d_info);
int pr_online_append(pr_online* o, const double* sig, int32_t* info);

/* ---- online signature SETS: fused SC + M2DP, and DELIGHT, with ONE device-side count (online.hip) -------------------------
 * A pr_online holds one SC or one M2DP database.  BASELINE config 5 (pr_match_topk_fused_f64: the four row z-scores of the SC and the
 * M2DP distances in one selection) needs both, and two handles would mean two counts that can disagree after an overflow; DELIGHT has no
 * z-scores at all.  A pr_onlineset is the same device-counted database for these two kinds over CALLER-OWNED buffers (pr_onlineset_buffers):
 *   PR_ONLINESET_FUSED    sc [capacity][2400] f64 and m2dp [capacity * 4][384] f64; delight must be NULL;   d_rows [4][capacity] in the order
 *                         SC structure, SC intensity, M2DP count, M2DP intensity (the order of pr_align_pairs_dev's [m][k][4])
 *   PR_ONLINESET_DELIGHT  delight [capacity * 16][256] f64; sc and m2dp must be NULL;                        d_rows [1][capacity]
 * and state [4] i32 = {count, flags, 0, 0}: ONE count for all parts.  As for pr_online: create allocates all scratch in one block and no
 * later call allocates; every launch's geometry depends on capacity only; d_emitted[0] == 0 switches a call off on the device; a
 * scribbled state[0] is clamped into 0 .. capacity before an address is derived from it; nothing is written outside the stated extents.
 * A call names the parts of its set's kind and passes NULL for the others (d_sc + d_m2dp, or d_delight).
 *
 *   pr_onlineset_match_dev   stream-ordered, no host decision, no read-back.  With n = state[0]:
 *     FUSED (three launches: rows, stats, select): the four distances of every row j < n by the pair functions pr_online uses (identical
 *     bits); per channel the row statistics of normalize(.,2) exactly as pr_online (NaN left out, N - 1); f = 0; f += p_weight z0;
 *     f += z1; f += p_weight z2; f += z3; THEN +Inf where n - j < mask_width (the query is row n; a masked NaN becomes a selectable
 *     +Inf); the k smallest by (score, index), NaN never selected, missing slots -1 / NaN.  n < 2: every slot -1 / NaN.
 *     DELIGHT (two launches: rows, select): d_j = processDELIGHT.m in fp64 in the reference's summation order (the function the DELIGHT
 *     matcher's exact rows use); no statistics and no fusion (run_test.m:26-41): the score is the distance, +Inf under the mask, the k
 *     smallest by (score, index), NaN never selected, +Inf selectable.  n = 0: -1 / NaN; n = 1 already returns row 0.
 *   pr_onlineset_append_dev  stream-ordered, ONE launch: every part of the keyframe goes to row count, then one thread commits count + 1
 *                            and d_info [4] = {appended, row or -1, count after, flags}.  At count == capacity NO part is stored and
 *                            PR_ONLINE_OVERFLOW is set (sticky until pr_onlineset_reset).  d_emitted off: info = {0, -1, count, flags}.
 *   pr_onlineset_append      the host form: host arrays of one keyframe's parts, info host [4]; uploads, runs the device path, synchronises.
 *   pr_onlineset_reset       zeroes state (stream-ordered).    pr_onlineset_count   synchronising read of count and flags (diagnostics).
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, buffer or required pointer, a part that does not
 * belong to the kind, a kind other than the two, capacity outside 1 .. PR_MAX_SIGS, max_k or k outside 1 .. 128 (k <= max_k), a
 * non-finite p_weight, mask_width < 0. */
enum { PR_ONLINESET_FUSED = 0, PR_ONLINESET_DELIGHT = 1 };
typedef struct pr_onlineset pr_onlineset;
typedef struct pr_onlineset_buffers { double* sc; double* m2dp; double* delight; int32_t* state; } pr_onlineset_buffers;
int pr_onlineset_create(pr_ctx* ctx, int kind, const pr_onlineset_buffers* buffers, int32_t capacity, int32_t max_k, pr_onlineset** out);
void pr_onlineset_destroy(pr_onlineset* o);
int pr_onlineset_reset(pr_onlineset* o);
int pr_onlineset_count(pr_onlineset* o, int32_t* count, int32_t* flags);
int pr_onlineset_match_dev(pr_onlineset* o, const double* d_sc, const double* d_m2dp, const double* d_delight, const int32_t* d_emitted,
                           int32_t mask_width, double p_weight, int32_t k, int32_t* d_idx, double* d_score, double* d_rows);
int pr_onlineset_append_dev(pr_onlineset* o, const double* d_sc, const double* d_m2dp, const double* d_delight, const int32_t* d_emitted,
                            int32_t* d_info);
int pr_onlineset_append(pr_onlineset* o, const double* sc, const double* m2dp, const double* delight, int32_t* info);

/* ---- the loop-closure log and the pose-graph relaxation of the map's poses (posegraph.hip) ------------------------------
 * A verify leaves (T, stats, accepted, hyp) in buffers the next keyframe overwrites.  A pr_posegraph keeps the accepted pairs of a drive
 * over CALLER-OWNED device buffers (pr_posegraph_buffers): edge_ij [edge_capacity][2] i32 (DB row i, query row j), edge_Z
 * [edge_capacity][12] f64 (the measured Z_ij), edge_w [edge_capacity][2] f64 (w_rot, w_trans) and state [4] i32 = {edges, flags, 0, 0},
 * and relaxes the map's poses over the odometry chain plus those edges.  A pose P_i = [R_i | t_i] is a row of pr_map_buffers.poses
 * (world to camera), verify's T maps query-camera points into the DB entry's camera frame, so an edge measures Z_ij ~ P_i P_j^-1.
 * Products and inverses are of rigid transforms: A B = [R_A R_B | R_A t_B + t_A], A^-1 = [R^T | -R^T t].
 *
 *   pr_posegraph_create    binds the buffers (they must outlive the handle), allocates ALL scratch the relaxation will ever need (sized
 *                          by the two capacities) and the staging of the host form, zeroes state.  No later call allocates.  The handle
 *                          is bound to ctx and its stream and must be destroyed before ctx; pr_posegraph_destroy frees the handle and
 *                          its scratch, never the buffers.  node_capacity, edge_capacity in 1 .. 2^20, max_outer in 1 .. 64, max_inner
 *                          in 1 .. 65536.
 *   pr_posegraph_add_dev   stream-ordered, one launch of one workgroup, 1 <= k <= 128.  EVERY array is device memory: d_idx [k] i32,
 *                          d_T [k][12] f64, d_accepted [k] u8 (a verify's idx, T, accepted), d_query_row [>= 1] i32 - the row the query
 *                          keyframe received: word 1 of the map append's info ("first row or -1") - and d_info [4] i32.
 *     The rule, decided on the device.  For p = 0 .. k - 1 in ascending order slot p is logged if and only if accepted[p] != 0,
 *     idx[p] >= 0, query_row >= 0, idx[p] != query_row and all 12 entries of T[p] are finite (a negative query_row switches the call
 *     off).  A logged slot stores (idx[p], query_row), T[p] and (w_rot, w_trans) at row `edges`, then edges + 1 is committed; at
 *     edges == edge_capacity nothing is stored and PR_POSEGRAPH_OVERFLOW is set (in state[1] and in every later info) until
 *     pr_posegraph_reset.  info = {edges logged by this call, first row or -1, edges after, flags}.  A scribbled state[0] is clamped
 *     into 0 .. edge_capacity before any address is formed from it.  Nothing is written outside the four buffers' stated extents.
 *   pr_posegraph_add       the host form: host arrays of the same meaning, query_row by value, info [4] host; uploads, runs the device
 *                          path, synchronises.
 *   pr_posegraph_reset     zeroes state (stream-ordered).    pr_posegraph_count   synchronising read of edges and flags (diagnostics).
 *   pr_posegraph_relax_dev stream-ordered, 3 outer + 3 launches whose grids depend on the create sizes only: d_n[0] (pass the map's
 *                          state: word 0 is the keyframe count; clamped to 0 .. node_capacity) and the edge count (state) are read on
 *                          the device, so one captured call serves every count.  d_poses_in, d_poses_out [node_capacity][12] (they may
 *                          be equal: pass the map's poses for both to correct the map in place), d_report [outer + 2] f64.
 *     The rule (restated in fp64 in tests/posegraph_np.py).  n = d_n[0].  Edges: the odometry edges (i, i + 1), 0 <= i < n - 1, with
 *     Z = P_i (P_i+1)^-1 of the INPUT poses and the weights (w_odo_rot, w_odo_trans); behind them the logged edges in log order.  A
 *     logged edge is skipped if i or j lies outside 0 .. n - 1, if i == j, or if its Z or weights are not finite; any edge is skipped
 *     if one of its two input poses has a non-finite entry.  Residual of an edge: E = Z^-1 P_i P_j^-1, r = [log_SO3(R_E); t_E], cost
 *     w_rot |r_rot|^2 + w_trans |r_trans|^2.  log_SO3: v = vee(R_E - R_E^T) / 2, theta = atan2(|v|, (tr R_E - 1) / 2), r_rot = k v with
 *     k = theta / |v|, and below theta = 1e-4 the series k = 1 + theta^2 / 6 (the ONE small-angle branch: it also switches the inverse
 *     left Jacobian's coefficient 1 / theta^2 - (1 + cos) / (2 theta sin) to 1 / 12 + theta^2 / 720, and exp's sin / theta and
 *     (1 - cos) / theta^2 to 1 - theta^2 / 6 and 1 / 2 - theta^2 / 24).  Residual rotations above 2 rad are outside the contract.
 *     Update of a node by delta = [w; v]: R <- exp(w) R, t <- exp(w) t + v; a delta of six exact zeros leaves the row's bytes alone.
 *     Node 0 is fixed (the gauge): its delta is 0, its gradient 0, its preconditioner block the identity.  One outer step: every
 *     edge is linearised at the current poses with the analytic Jacobians A = dr / d delta_i, B = dr / d delta_j at delta = 0;
 *     g = -sum J^T W r; D_i = lambda I + sum J^T W J (6 x 6), inverted by Gauss-Jordan without pivoting - a pivot that is not positive
 *     makes the inverse the zero block (a node without a weighted edge at lambda = 0 does not move); exactly `inner` iterations of
 *     preconditioned conjugate gradients on (lambda I + J^T W J) x = g from x = 0, the matrix applied edge by edge; alpha = rz / pq if
 *     pq > 0 else 0, beta = rz' / rz if rz > 0 else 0; no early exit; then every node is updated.  After `outer` steps the poses of
 *     rows < n are written; rows >= n of d_poses_out are not.  report[s] = the cost before outer step s, report[outer] = the final
 *     cost, report[outer + 1] = the number of edges used.
 *     Nothing to relax: with n < 2, or when no LOGGED edge is used, no step is taken - the odometry edges have zero residual by
 *     construction - so rows < n are copied bit for bit and every cost is reported as 0.
 *     Every per-node sum is a gather in a fixed order (odometry edge i - 1, odometry edge i, the logged edges in log order), the dot
 *     products are summed in a fixed order, there are no floating-point atomics: two runs give the same bytes.
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, buffer, params or required pointer, a capacity or
 * max_outer / max_inner out of range, k outside 1 .. 128, outer outside 1 .. max_outer, inner outside 1 .. max_inner, a negative or
 * non-finite weight or lambda. */
typedef struct pr_posegraph pr_posegraph;
typedef struct pr_posegraph_buffers { int32_t* edge_ij; double* edge_Z; double* edge_w; int32_t* state; } pr_posegraph_buffers;
typedef struct pr_posegraph_params { int32_t outer, inner; double lambda, w_odo_rot, w_odo_trans; } pr_posegraph_params;
#define PR_POSEGRAPH_OVERFLOW 1
int pr_posegraph_create(pr_ctx* ctx, const pr_posegraph_buffers* buffers, int32_t node_capacity, int32_t edge_capacity, int32_t max_outer,
                        int32_t max_inner, pr_posegraph** out);
void pr_posegraph_destroy(pr_posegraph* g);
int pr_posegraph_reset(pr_posegraph* g);
int pr_posegraph_count(pr_posegraph* g, int32_t* edges, int32_t* flags);
int pr_posegraph_add_dev(pr_posegraph* g, const int32_t* d_idx, const double* d_T, const uint8_t* d_accepted, const int32_t* d_query_row, int32_t k,
                         double w_rot, double w_trans, int32_t* d_info);
int pr_posegraph_add(pr_posegraph* g, const int32_t* idx, const double* T, const uint8_t* accepted, int32_t query_row, int32_t k, double w_rot,
                     double w_trans, int32_t* info);
int pr_posegraph_relax_dev(pr_posegraph* g, const double* d_poses_in, const int32_t* d_n, const pr_posegraph_params* params, double* d_poses_out,
                           double* d_report);

/* ---- the world map: all clouds of a pr_map fused into one world-frame point set (worldmap.hip) ------------------------
 * A pr_map stores its clouds per camera frame; they do not move when pr_posegraph_relax_dev corrects the poses.  A pr_worldmap fuses
 * them - under ANY [keyframe_capacity][12] pose array, the map's own or the relaxed ones - into one voxel-deduplicated world-frame set over
 * CALLER-OWNED device buffers (pr_worldmap_buffers): xyz [out_capacity][3] f64, inten [out_capacity] f32, src [out_capacity] i64 (the
 * point's index in the map), row [out_capacity] i32 (its keyframe row), count [out_capacity] i32 (the points of its voxel) and state [4]
 * i32 = {rows written, flags, 0, 0}.
 *
 *   pr_worldmap_create    binds the buffers and the map (both must outlive the handle; the handle is destroyed before the map), allocates
 *                         ALL scratch a fuse will ever need in one block and zeroes state.  No later call allocates.  The scratch is a
 *                         hash table of T = the smallest power of two >= max(2 point_capacity, 64) slots of 20 bytes, one int32 per
 *                         point and two per 256 points, and the staging of the host form: 20 T + 4 point_capacity + 8 nblk4 + 96
 *                         keyframe_capacity + 64 bytes, each part rounded up to 16 (nblk4 = ceil(point_capacity / 256) rounded up to 4);
 *                         pr_worldmap_scratch_bytes returns the figure (0 for capacities create refuses).  The map's point_capacity
 *                         may not exceed 2^29.
 *   pr_worldmap_fuse_dev  stream-ordered: two memset nodes and four launches whose grids depend on the create capacities only.  No host
 *                         decision, no read-back, nothing allocated, so ONE captured fuse serves every count.  d_poses
 *                         [keyframe_capacity][12] f64 device, NULL = the map's poses; d_n [>= 1] i32 device, NULL = the map's state;
 *                         d_info [4] i64 device.  A fuse is a full rebuild: nothing of an earlier call survives.
 *     The rule (normative; restated in fp64 in tests/worldmap_np.py).  n = d_n[0] clamped into 0 .. keyframe_capacity, as every reader of
 *     the map's state does; P = offs[n] clamped into 0 .. point_capacity.  Point g, 0 <= g < P, belongs to row r with offs[r] <= g <
 *     offs[r + 1]; empty and dropped rows own nothing.
 *     1. World position.  A pose row is world-to-camera [R | t].  d = p - t componentwise, w_a = (R[0][a] d0 + R[1][a] d1) + R[2][a] d2
 *        in exactly this association, in fp64 without contraction (no fused multiply-add).
 *     2. Validity.  A point is skipped, and PR_WORLDMAP_SKIPPED set, if any of its pose's 12 entries or any w_a is not finite.
 *        c_a = floor(w_a / cell) with IEEE division.  A point with any c_a outside [-2^20, 2^20) - compared as a double, before any
 *        conversion to an integer - is skipped and sets PR_WORLDMAP_RANGE.  key = the three indices biased by 2^20, 21 bits each, packed
 *        into 63 bits.
 *     3. Voxels.  All valid points of one key form a voxel; its count is their number; its representative is the smallest g with keep =
 *        0 (the first observation) and the largest g with keep = 1 (the latest).  A voxel qualifies iff count >= min_count.
 *     4. Output.  The qualifying voxels in ascending order of their representative's g - a subsequence of the map's points in map order.
 *        For the j-th: xyz[j] = w of the representative with the bits of step 1, inten[j] its intensity, src[j] = g, row[j] = r, count[j]
 *        the voxel's count.  Only j < out_capacity are stored; if more qualify PR_WORLDMAP_OVERFLOW is set.  Rows >= min(qualifying,
 *        out_capacity) are not written.
 *     5. state = {rows written, flags, 0, 0}, d_info = {rows written, voxels that qualified, valid points, flags}.  The flags are the
 *        call's; nothing is sticky.  n = 0 or P = 0 gives zero rows and changes no byte of the five output arrays.
 *     PR_WORLDMAP_TABLE: the table's probe is bounded by T steps, past which the point is dropped with this flag; with T >= 2
 *     point_capacity that cannot happen and no input makes a lane spin.  Every reduction is an integer atomic or an integer scan and every
 *     position is computed per point in a fixed association: the output bytes are a function of the inputs alone - equal between runs,
 *     between eager and replayed calls, and to the restatement.
 *   pr_worldmap_fuse      the host form: poses [keyframe_capacity][12] and n [1] are HOST arrays (NULL = the map's), runs the device path,
 *                         synchronises, and copies info [4] and the first `rows written` rows into the host arrays xyz, inten, src, row,
 *                         count (each of out_capacity rows).
 *   pr_worldmap_count     synchronising read of rows written and flags (diagnostics).
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, buffer or required pointer, cell not finite or <= 0,
 * min_count < 1, keep outside {0, 1}, out_capacity < 1, a map of another context or of more than 2^29 points. */
typedef struct pr_worldmap pr_worldmap;
typedef struct pr_worldmap_buffers { double* xyz; float* inten; int64_t* src; int32_t* row; int32_t* count; int32_t* state; } pr_worldmap_buffers;
enum { PR_WORLDMAP_OVERFLOW = 1, PR_WORLDMAP_SKIPPED = 2, PR_WORLDMAP_RANGE = 4, PR_WORLDMAP_TABLE = 8 };
int pr_worldmap_create(pr_ctx* ctx, pr_map* map, const pr_worldmap_buffers* buffers, int64_t out_capacity, pr_worldmap** out);
void pr_worldmap_destroy(pr_worldmap* wm);
int64_t pr_worldmap_scratch_bytes(int32_t keyframe_capacity, int64_t point_capacity);
int pr_worldmap_count(pr_worldmap* wm, int64_t* rows, int32_t* flags);
int pr_worldmap_fuse_dev(pr_worldmap* wm, const double* d_poses, const int32_t* d_n, double cell, int32_t min_count, int32_t keep,
                         int64_t* d_info);
int pr_worldmap_fuse(pr_worldmap* wm, const double* poses, const int32_t* n, double cell, int32_t min_count, int32_t keep, double* xyz,
                     float* inten, int64_t* src, int32_t* row, int32_t* count, int64_t* info);

/* ---- the map localiser: scan-to-map registration against a world map through one shared voxel index (maploc.hip) -----
 * A pr_worldmap fuse leaves one world-frame point per occupied voxel in caller-owned buffers.  A pr_maploc registers clouds - keyframes of
 * this drive or of a later one over the same route - against those rows: ONE voxel hash index per fuse, shared by every pair of a call, a
 * correspondence search through it that is exact within the radius, and the ICP update of pr_icp_pairs_dev on the same code.  Everything
 * is stream-ordered, reads its counts on the device, allocates nothing after create and can be captured.
 *
 *   pr_maploc_create      takes the world map's buffer RECORD (not its handle) and reads only xyz [out_capacity][3] f64, row [out_capacity]
 *                         i32 and state [4] i32; they must outlive the handle.  `cell` is fixed for the handle's life; the caller fuses
 *                         with the same cell (a mismatch shows as PR_MAPLOC_DUPLICATE).  Allocates ALL scratch in one block; no later
 *                         call allocates.  With T = the smallest power of two >= max(2 out_capacity, 64), ld = max(max_src_pts, 1),
 *                         nchunks = ceil(ld / 256) and pc = pair_capacity the parts are, each rounded up to 16 bytes:
 *                           16 T (the table: key u64, row u64) | 16 (control: flags, rows indexed) | 16 (offs2 [2] i64) | 4 pc (pair_dst,
 *                           zeros) | 8 pc ld (nn_d) | 4 pc ld (nn_j) | 160 pc nchunks (chunk partials, 20 doubles each) | 4 pc (done) |
 *                           16 pc (prev) | staging of the host forms: 24 pc ld (xyz_q) | 8 (pc + 1) (offs_q) | 4 pc (pair_src) | 96 pc (T)
 *                           | 8 pc (excl) | 8 (pc + 1) (out_offs) | 32 pc (stats) | 32 (info)
 *                         pr_maploc_scratch_bytes returns the sum (0 for sizes create refuses).
 *   pr_maploc_index_dev   two memset nodes and two launches.  R = world.state[0] clamped into 0 .. out_capacity.  Row j < R is INDEXED iff
 *                         its three coordinates are finite (otherwise PR_MAPLOC_SKIPPED), every c_a = floor(x_a / cell) with IEEE division
 *                         lies in [-2^20, 2^20) - compared as a double before any conversion - (otherwise PR_MAPLOC_RANGE), and it is the
 *                         smallest j of its key; the key is the three indices biased by 2^20, 21 bits each, packed into 63 bits (c_0
 *                         highest) exactly as the world map packs it.  A key held by more than one row sets PR_MAPLOC_DUPLICATE: that
 *                         cannot happen after a fuse at the same cell.  d_info [4] i64 = {rows indexed, R, flags, 0}; the flags are the
 *                         call's, nothing is sticky; R = 0 gives an empty index.  An index is valid until the world buffers change:
 *                         re-index after every fuse.  A stale index can return stale rows; it never forms an address outside
 *                         xyz[0 .. out_capacity).  PR_MAPLOC_TABLE: the table's probe is bounded by T steps, past which the row is dropped
 *                         with this flag; with T >= 2 out_capacity that cannot happen and no input makes a lane spin.
 *   pr_maploc_nn_dev      one correspondence pass.  Pair p is off when d_pair_src[p] < 0 or >= Nq: its d_out_offs span is 0 long (in
 *                         refine: PR_ICP_NO_PAIR, T0 and zeros - pr_icp_pairs_dev's convention).  A source cloud is read up to max_src_pts
 *                         points.  p' = T s in pr_icp_pairs_dev's association; a non-finite p' has no correspondent; t_a = p'_a / cell by
 *                         the index's division, and a t_a outside [-2^20 - 1, 2^20 + 1) - tested in floating point - has none either.
 *                         Candidates: the indexed rows whose voxel differs from floor(t) by at most 1 per axis (27 keys; those outside
 *                         the 21-bit range are dropped); with d_excl != NULL the rows with excl[p][0] <= world.row[j] <= excl[p][1] are
 *                         dropped (lo > hi excludes nothing).  d2 = ((dx dx) + dy dy) + dz dz; "smaller d2, then smaller j"; a NaN or
 *                         +Inf distance never wins; the result is (j, d2) where d2 < fl(max_corr^2) and (-1, +Inf) elsewhere, at
 *                         d_out_offs[p] + i.  It equals the brute-force first-minimum scan over the indexed, non-excluded rows masked to
 *                         the radius on every input, because max_corr (1 + 2^-10) <= cell is required.
 *   pr_maploc_refine_dev  pr_icp_pairs_dev with this search against the one-cloud target {world.xyz, offs2 = {0, R}}: max_iter + 1 rounds
 *                         of (pass with chunk sums of 256 source points, update); stop rules, statuses and pr_icp_stats unchanged; the
 *                         bytes of pr_icp_pairs_dev under PR_ICP_SEARCH_GRID on the same target when nothing is excluded and no key is
 *                         duplicated.  d_T_out may be d_T0.
 *   pr_maploc_seed_dev    n = d_n[0] clamped into 0 .. keyframe_capacity.  Pair p is ON iff 0 <= d_idx[p] < n, d_accepted == NULL or
 *                         d_accepted[p] != 0, the pose row's 12 entries are finite and d_T_rel == NULL or its 12 entries are finite.
 *                         For a world-to-camera P = [R | t]: Rinv[a][b] = R[b][a], tinv_a = -((R[0][a] t0 + R[1][a] t1) + R[2][a] t2).
 *                         d_T_rel == NULL: T0 = [Rinv | tinv].  Otherwise T0 = inv(P_idx) o T_rel: R0[a][b] = (Rinv[a][0] Rr[0][b] +
 *                         Rinv[a][1] Rr[1][b]) + Rinv[a][2] Rr[2][b], t0_a = ((Rinv[a][0] tr0 + Rinv[a][1] tr1) + Rinv[a][2] tr2) + tinv_a,
 *                         fp64 without contraction.  An ON pair writes d_pair_src[p] = d_src ? d_src[p] : p; an OFF pair -1 and T0 =
 *                         identity.  (pr_verify_pairs_dev's T maps query-camera points into DB row idx's camera frame, so T0 maps them
 *                         into the world.)
 *   pr_maploc_index / _nn / _refine   the host forms: upload, run the device form, synchronise, read back.  Their staging is part of the
 *                         one allocation, so Nq <= pair_capacity and offs_q[Nq] <= pair_capacity x ld are required.
 *   pr_maploc_count       synchronising read of the last index's rows indexed and flags (diagnostics).
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, record member or required pointer, out_capacity < 1 or
 * > 2^29, cell not finite or <= 0, pair_capacity outside 1 .. 65535, max_src_pts outside 0 .. 2^26, c < 0 or > pair_capacity,
 * keyframe_capacity < 1, max_iter < 0, max_corr not positive and finite, min_inliers < 3, a NaN tolerance, and max_corr (1 + 2^-10) >
 * cell - the contract that makes the 27-voxel search exact. */
typedef struct pr_maploc pr_maploc;
enum { PR_MAPLOC_SKIPPED = 1, PR_MAPLOC_RANGE = 2, PR_MAPLOC_DUPLICATE = 4, PR_MAPLOC_TABLE = 8 };
int pr_maploc_create(pr_ctx* ctx, const pr_worldmap_buffers* world, int64_t out_capacity, double cell, int32_t pair_capacity, int32_t max_src_pts,
                     pr_maploc** out);
void pr_maploc_destroy(pr_maploc* ml);
int64_t pr_maploc_scratch_bytes(int64_t out_capacity, int32_t pair_capacity, int32_t max_src_pts);
int pr_maploc_count(pr_maploc* ml, int64_t* rows_indexed, int32_t* flags);
int pr_maploc_index_dev(pr_maploc* ml, int64_t* d_info);
int pr_maploc_seed_dev(pr_maploc* ml, const double* d_poses, const int32_t* d_n, int32_t keyframe_capacity, const int32_t* d_idx,
                       const uint8_t* d_accepted, const double* d_T_rel, const int32_t* d_src, int32_t c, double* d_T0, int32_t* d_pair_src);
int pr_maploc_nn_dev(pr_maploc* ml, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                     const double* d_T, const int32_t* d_excl, double max_corr, int64_t* d_out_offs, int32_t* d_nn_idx, double* d_nn_d2);
int pr_maploc_refine_dev(pr_maploc* ml, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                         const double* d_T0, const int32_t* d_excl, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness,
                         int32_t min_inliers, double* d_T_out, pr_icp_stats* d_stats);
int pr_maploc_index(pr_maploc* ml, int64_t* info);
int pr_maploc_nn(pr_maploc* ml, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T,
                 const int32_t* excl, double max_corr, int64_t* out_offs, int32_t* nn_idx, double* nn_d2);
int pr_maploc_refine(pr_maploc* ml, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T0,
                     const int32_t* excl, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers,
                     double* T_out, pr_icp_stats* stats);

/* ---- point-to-plane scan-to-map: world-map normals and a plane-metric refinement (mapplane.hip) -------------------------
 * pr_maploc_refine_dev pulls every source point towards the ONE point its voxel holds, an arbitrary in-plane position: its residual never
 * reaches zero on a correct pose.  A pr_mapplane over an existing pr_maploc estimates a normal per world row through the localiser's voxel
 * index and refines with the point-to-plane metric.  It BORROWS the localiser's table, cell, out_capacity, world record, create sizes and
 * the offsets of the last index, and makes ONE allocation of its own at create; destroy it before the localiser.  Every device call is
 * stream-ordered on the context's stream, reads nothing back, allocates nothing and can be captured; grids depend on the create sizes and
 * c only.  fp64 without contraction.
 *
 *   pr_mapplane_create    With ld = max(max_src_pts, 1), nchunks = ceil(ld / 256), pc = pair_capacity (the localiser's) the parts of the
 *                         allocation are, each rounded up to 16 bytes:
 *                           8 pc ld (nn_d) | 4 pc ld (nn_j) | 240 pc nchunks (chunk partials, 30 doubles each) | 4 pc (done) | 16 pc (prev)
 *                           | staging of the host forms: 24 pc ld (xyz_q) | 8 (pc + 1) (offs_q) | 4 pc (pair_src) | 96 pc (T) | 8 pc (excl)
 *                           | 32 pc (stats) | 24 pc ld (normals) | 4 pc ld (ninfo)
 *                         pr_mapplane_scratch_bytes(pair_capacity, max_src_pts) returns the sum (0 for sizes pr_maploc_create refuses).
 *   pr_mapplane_normals_dev   one launch, one lane per world row.  d_normals [out_capacity][3] f64 and d_ninfo [out_capacity] i32 are the
 *                         caller's; every entry is written.  Call it behind pr_maploc_index_dev.  The rule:
 *                         Row j is PROCESSED iff it is INDEXED in the sense of pr_maploc_index_dev (j < R, finite, in range, the smallest
 *                         row of its key).  Every other row < out_capacity gets ninfo = 0 and the normal (0, 0, 0).
 *                         Neighbours: the 27 keys around floor(x_a / cell) in the probe's order - d0 outer, then k = 0 .. 8 with
 *                         (k / 3 - 1, k % 3 - 1); keys outside the 21-bit range are dropped.  Each key contributes the row the table holds,
 *                         row j itself included.  A row is kept iff d2 = ((dx dx) + dy dy) + dz dz < fl(radius^2) with d = q - x_j.  The
 *                         count k includes j itself.
 *                         Sums, pivoted on the row itself (a UTM-sized offset never enters a product), in visit order from 0.0: the three
 *                         s_a = sum d_a and the six S_ab = sum d_a d_b; C_ab = S_ab - (s_a s_b) / k (IEEE division).
 *                         Eigen-decomposition of C by cyclic Jacobi in fp64: 8 sweeps, pivots (0,1), (0,2), (1,2), V = I at the start.  A
 *                         rotation about (p, q) with third index r is skipped when C_pq is exactly 0; otherwise theta = (C_qq - C_pp) /
 *                         (2 C_pq), t = sgn(theta) / (|theta| + sqrt(theta theta + 1)) with sgn(0) = +1, c = 1 / sqrt(t t + 1), s = t c;
 *                         C_pp -= t C_pq, C_qq += t C_pq, C_pq = 0; (C_rp, C_rq) <- (c C_rp - s C_rq, s C_rp + c C_rq); every row a of V:
 *                         (V_ap, V_aq) <- (c V_ap - s V_aq, s V_ap + c V_aq).  The eigenvalues are the diagonal, sorted l0 <= l1 <= l2
 *                         by three compare-exchanges (1,0), (2,1), (1,0) on strict "<": the lower index first on ties.
 *                         The row is VALID iff k >= min_nbrs, every eigenvalue is finite, l1 > 0 and l0 <= max_ratio l1.  A valid row
 *                         gets ninfo = k and n = the eigenvector (column of V) of l0, every component divided by its norm
 *                         sqrt((e0 e0 + e1 e1) + e2 e2), the sign chosen so that the component of largest magnitude is positive (the
 *                         lowest index wins a tie).  An invalid row gets ninfo = -k and the normal (0, 0, 0).
 *   pr_mapplane_refine_dev    the arguments of pr_maploc_refine_dev plus d_normals and d_ninfo.  max_iter + 1 rounds of (pass, update)
 *                         with done flags, three launches a round: a fixed launch count.
 *                         Pass: the correspondence search is pr_maploc_nn_dev's rule - the same launch, the same (j, d2), the exclusion
 *                         window included.  n_inl, fitness and rmse keep pr_maploc_refine_dev's definitions over ALL correspondents
 *                         inside the radius, so pr_verify_select_dev's thresholds keep their meaning.  A correspondent enters the UPDATE
 *                         only if ninfo[j] > 0.  For such a point, with T = [R | t]: p' = T s; u = p' - t (the lever arm about the sensor
 *                         position: no world-sized coordinate enters a cross product); e = p' - q; r = (n_0 e_0 + n_1 e_1) + n_2 e_2;
 *                         J = [u x n, n].  Per chunk of 256 source points: the inlier count, sum d2, the plane count, the 21 entries of
 *                         sum J J^T (upper triangle, row-major) and the 6 of sum J r, by a fixed tree - within a wave (64-lane shuffle
 *                         tree), then the four waves in order - to [pair][chunk][30] in the handle's own scratch.
 *                         Update: the chunks are combined in index order.  Fewer than min_inliers plane correspondents: PR_ICP_TOO_FEW.
 *                         A x = -b is solved by L D L^T without pivoting in the order (w0, w1, w2, v0, v1, v2): d_k = A_kk - sum_m<k
 *                         (L_km d_m) L_km, L_ik = (A_ik - sum_m<k (L_im d_m) L_km) / d_k, y_i = -b_i - sum_m<i L_im y_m, z_i = y_i / d_i,
 *                         x_i = z_i - sum_m>i L_mi x_m, every sum subtracted term by term with m ascending.  PR_ICP_DEGENERATE when a d_k
 *                         is not finite or d_k <= 1e-12 A_kk (the original diagonal entry; scale-free) or an x_i is not finite: a single
 *                         plane or a corridor without end walls ends here.  R <- Exp(w) R by Rodrigues, Exp(w) = (1 - b th2) I + b w w^T +
 *                         a [w]x with th2 = |w|^2, a = sin(th) / th, b = (1 - cos(th)) / th2; below th2 = 1e-4 the series
 *                         a = 1 - th2/6 (1 - th2/20 (1 - th2/42)), b = 1/2 - th2/24 (1 - th2/30 (1 - th2/56)).  t <- t + v.
 *                         Stop rules, statuses, pr_icp_stats and the convention "T is the last one a valid update produced" are
 *                         pr_icp_pairs_dev's, as is the final extra pass for the reported statistics.  d_T_out may be d_T0.
 *   pr_mapplane_normals / _refine   the host forms: upload, run the device form, synchronise, read back.  They stage through the handle's
 *                         own allocation, so out_capacity <= pair_capacity x ld, Nq <= pair_capacity and offs_q[Nq] <= pair_capacity x ld
 *                         are required.
 * PR_EINVAL (text: pr_last_error) before any device is touched: radius not positive and finite; radius (1 + 2^-10) > cell - the containment
 * argument of DESIGN.md 4.20: everything inside the ball is in the 27 voxels; min_nbrs < 3 or > 27; max_ratio not in (0, 1]; NULL handles
 * and pointers; for refine everything pr_maploc_refine_dev refuses, and min_inliers < 6. */
typedef struct pr_mapplane pr_mapplane;
int pr_mapplane_create(pr_ctx* ctx, pr_maploc* ml, pr_mapplane** out);
void pr_mapplane_destroy(pr_mapplane* mp);
int64_t pr_mapplane_scratch_bytes(int32_t pair_capacity, int32_t max_src_pts);
int pr_mapplane_normals_dev(pr_mapplane* mp, double radius, int32_t min_nbrs, double max_ratio, double* d_normals, int32_t* d_ninfo);
int pr_mapplane_refine_dev(pr_mapplane* mp, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                           const double* d_T0, const int32_t* d_excl, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness,
                           int32_t min_inliers, const double* d_normals, const int32_t* d_ninfo, double* d_T_out, pr_icp_stats* d_stats);
int pr_mapplane_normals(pr_mapplane* mp, double radius, int32_t min_nbrs, double max_ratio, double* normals, int32_t* ninfo);
int pr_mapplane_refine(pr_mapplane* mp, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c,
                       const double* T0, const int32_t* excl, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness,
                       int32_t min_inliers, const double* normals, const int32_t* ninfo, double* T_out, pr_icp_stats* stats);

/* ---- the world map, its voxel index and its normals grown one keyframe at a time (mapgrow.hip) -----------------------
 * pr_worldmap_fuse_dev is a full rebuild, and pr_maploc_index_dev and pr_mapplane_normals_dev run one lane per row of out_capacity: their
 * cost follows the drive, not the keyframe.  With keep = 0 (first observation) and min_count = 1 the world rows are a subsequence of the
 * map's points in map order, so a new keyframe's new voxels are new rows at the end, its points in known voxels only raise a count, the
 * index only gains keys, and a normal changes only for the rows the index holds in the 27 voxels around a new row.  A pr_mapgrow over an
 * existing pr_worldmap and the pr_maploc created over the same world buffer record takes in ONE map row a call and leaves THE REBUILD'S
 * BYTES.  It BORROWS both handles (their buffers, the map's arrays, the localiser's table, cell and control words) and makes ONE
 * allocation of its own at create; destroy it before them.  Every device call is stream-ordered on the context's stream, reads its counts
 * and makes its decisions - the refusals included - on the device, allocates nothing, reads nothing back, and its launch geometry depends
 * on the map's max_cloud_points only, so one captured call serves every keyframe.  fp64 without contraction; integer atomics and integer
 * scans only; no workgroup waits for another; every probe is a bounded loop of at most T steps.
 * Names: kcap, pcap and mcp are the keyframe_capacity, point_capacity and max_cloud_points of the map the world map was created over; ocap,
 * cell and T are the localiser's; the handle's own device words are fused, rows_seen and the last range [a, b).
 *
 *   pr_mapgrow_create     refuses a world map and a localiser over different buffer records (xyz, row, state) or out_capacity, or of
 *                         another context.  With nblk = ceil(mcp / 256) the parts of the allocation are, each rounded up to 16 bytes:
 *                           64 (control words) | 4 mcp (slot_of) | 8 nblk (block counts) | staging of the host forms: 96 (pose row) | 16
 *                           (row) | 32 (info) | 648 mcp (normals, 27 per point) | 108 mcp (ninfo) | 108 mcp (rows)
 *                         pr_mapgrow_scratch_bytes(max_cloud_points) returns the sum (0 for mcp < 1 or > 2^26).  It zeroes its words.
 *   pr_mapgrow_sync_dev   one small launch: fused = d_n[0] clamped into 0 .. kcap (NULL = the map's state), rows_seen = world.state[0]
 *                         clamped into 0 .. ocap, a = b = rows_seen.  Issue it behind pr_worldmap_fuse_dev(keep 0, min_count 1, the
 *                         localiser's cell) + pr_maploc_index_dev: from then on extends follow that fuse.
 *   pr_mapgrow_extend_dev six launches.  r = d_row[0] - word 1 of pr_map_append_dev's info, "first row or -1", taken as
 *                         pr_posegraph_add_dev takes d_query_row; n = the map's state[0] clamped into 0 .. kcap; R = world.state[0]
 *                         clamped into 0 .. ocap.  d_poses [kcap][12] f64 device, NULL = the map's poses; d_info [4] i64 device.
 *     r < 0: the call is off.  d_info = {0, R, 0, 0}; no other byte changes anywhere, the handle's words included.
 *     Refusals, decided on the device and OR-ed; nothing changes and d_info = {0, R, 0, flags}: r != fused or r >= n gives
 *     PR_MAPGROW_ORDER; R != rows_seen gives PR_MAPGROW_STALE (somebody fused without a sync); world.state[1] & PR_WORLDMAP_OVERFLOW
 *     gives PR_MAPGROW_FULL.
 *     Otherwise the points g in [offs[r], offs[r + 1]) clamped as the fuse at n = r + 1 clamps them (P = offs[r + 1] into 0 .. pcap,
 *     offs[r] into 0 .. P; at most mcp points, which is all a stored cloud has) are taken.  World position and validity are steps 1 and 2
 *     of pr_worldmap_fuse_dev's rule under pose row r of d_poses, the cell the localiser's - the SAME inlined code as the fuse.
 *     A valid point whose key the index holds at row j does count[j] += 1.  The other valid points form new voxels by key; the
 *     representative is the smallest g; in ascending representative g the new voxels receive the rows R, R + 1, ...  A row below ocap
 *     is stored - xyz, inten, src = g, row = r, count = the voxel's points - and the index gains key -> row.  Voxels past ocap are not
 *     stored and the index does not hold them (a lookup returns "no row"); PR_WORLDMAP_OVERFLOW is set.  The new keys enter the
 *     localiser's table by a probe of at most T steps.  A key that finds no slot - only a call with more than T - R >= ocap new voxels
 *     can fill the table - turns the call into a refusal with PR_WORLDMAP_TABLE: d_info = {0, R, 0, the call's flags}, no row is
 *     stored, no count raised and no word changed; rebuild with a larger out_capacity.
 *     Afterwards world.state[0] = R' = min(R + new voxels, ocap), state[1] |= the call's world-map flags (PR_WORLDMAP_*), words 2 and 3
 *     stay 0; the localiser's rows-indexed count rises by the stored rows and its one-cloud target becomes {0, R'}, so
 *     pr_maploc_nn_dev, pr_maploc_refine_dev, pr_mapplane_refine_dev and pr_maploc_count see the grown map; fused = r + 1, rows_seen =
 *     R', [a, b) = [R, R').  d_info = {rows stored, R', valid points of the row, the call's world-map flags}.  A row that is empty or
 *     dropped, or whose pose is not finite, advances fused and stores nothing.
 *   pr_mapgrow_normals_dev   one launch, 27 mcp lanes.  For every row in [a, b): the normal and ninfo of each row the index holds for the 27
 *                         keys around that row's voxel - the row itself included - are recomputed by pr_mapplane_normals_dev's rule, the
 *                         SAME per-row device function.  No other entry of d_normals [ocap][3] / d_ninfo [ocap] is written.  Several
 *                         lanes may recompute one row; they store equal bytes.  The refusals are pr_mapplane_normals_dev's.
 *   The contract.  Let the world buffers, the index and the normal arrays hold a rebuild at n = r under poses P - fuse(P, n, cell, 1,
 *   keep 0), then index, then normals(radius, ...).  After extend(P, r) and normals(radius, ...): the five world arrays hold the rebuild at
 *   n = r + 1 byte for byte, also when the call overflows; so do state and the two normal arrays; the index agrees with a fresh
 *   pr_maploc_index_dev as a map from keys to rows (the slot order may differ; a key past ocap may sit in the table without a row) - the
 *   observable is pr_maploc_nn_dev and the two refines, bit for bit.
 *   Out of scope: keep = 1 and min_count > 1 (they would move or insert rows in the middle of the arrays); more than one row a call;
 *   re-extending under changed poses - after a relaxation the caller rebuilds and syncs.
 *   pr_mapgrow_extend / _normals   the host forms: upload, run the device form, synchronise, read back.  poses [kcap][12] is a HOST array
 *                         (NULL = the map's) of which row `row` is uploaded; normals [ocap][3] and ninfo [ocap] are HOST arrays holding
 *                         the earlier normals, of which only the recomputed rows are overwritten.
 *   pr_mapgrow_count      synchronising read of fused, rows_seen and the last extend's info[3] (diagnostics).
 * PR_EINVAL (text: pr_last_error) before any device is touched for NULL handles and required pointers, handles of another context or over
 * different records, and for everything pr_mapplane_normals_dev refuses. */
typedef struct pr_mapgrow pr_mapgrow;
enum { PR_MAPGROW_ORDER = 16, PR_MAPGROW_STALE = 32, PR_MAPGROW_FULL = 64 };   /* beside PR_WORLDMAP_OVERFLOW/SKIPPED/RANGE/TABLE = 1/2/4/8 */
int pr_mapgrow_create(pr_ctx* ctx, pr_worldmap* wm, pr_maploc* ml, pr_mapgrow** out);
void pr_mapgrow_destroy(pr_mapgrow* mg);
int64_t pr_mapgrow_scratch_bytes(int32_t max_cloud_points);
int pr_mapgrow_sync_dev(pr_mapgrow* mg, const int32_t* d_n);
int pr_mapgrow_extend_dev(pr_mapgrow* mg, const double* d_poses, const int32_t* d_row, int64_t* d_info);
int pr_mapgrow_normals_dev(pr_mapgrow* mg, double radius, int32_t min_nbrs, double max_ratio, double* d_normals, int32_t* d_ninfo);
int pr_mapgrow_extend(pr_mapgrow* mg, const double* poses, int32_t row, int64_t* info);
int pr_mapgrow_normals(pr_mapgrow* mg, double radius, int32_t min_nbrs, double max_ratio, double* normals, int32_t* ninfo);
int pr_mapgrow_count(pr_mapgrow* mg, int32_t* fused, int64_t* rows, int32_t* flags);

/* ---- the closure consistency gate in front of the pose-graph relaxation (gate.hip) -------------------------------------
 * pr_posegraph_relax_dev has no robust kernel: one wrong closure that passed verify pulls the whole graph.  What exposes such a closure is
 * that it disagrees with the other closures and with the odometry between them.  A pr_gate checks every ordered pair of logged closures
 * of a SOURCE log against each other and copies the consistent ones, in log order, into a second log; an ordinary pr_posegraph over that
 * second log relaxes them.  Everything is stream-ordered, reads both counts on the device, allocates nothing after create; every grid is
 * a function of the create sizes only, so one capture made on an empty log serves every count.
 *
 *   pr_gate_create    takes the buffer RECORDS of two logs (the caller also holds a pr_posegraph over each; both must outlive the gate,
 *                     which must be destroyed before them).  The gate only reads src; in dst it writes rows [0, kept) of edge_ij, edge_Z
 *                     and edge_w and the four words of state, and nothing else.  rot_tab and trans2_tab are HOST arrays [max_gap + 1];
 *                     create uploads them and allocates ALL scratch in one block; no later call allocates or copies from host memory.
 *                     With EC = edge_capacity and G = max_gap + 1 the parts are, each rounded up to 16 bytes:
 *                       288 EC (L, M, N: 36 doubles an edge) | 8 EC (the edges' rows) | 4 EC (valid) | 4 EC | 4 EC (keep of the round
 *                       before and of this one) | 4 EC (support sums) | 4 EC (map) | 8 G (rot_tab) | 8 G (trans2_tab) | 16 (control)
 *                       | staging of the host form: EC (keep) | 4 EC (support) | 4 EC (map) | 16 (info)
 *                     pr_gate_scratch_bytes returns the sum (0 for sizes create refuses).
 *   pr_gate_run_dev   1 + 2 rounds + 2 launches.  d_poses [node_capacity][12] f64 and d_n [>= 1] i32: a pr_map's poses and state.
 *                     d_keep u8, d_support i32, d_map i32 are [edge_capacity], every entry is written, any of the three may be NULL;
 *                     d_info [4] i32.  No read-back.
 *   pr_gate_run       the same with HOST outputs (d_poses and d_n stay device memory); synchronises.
 *
 * The rule (restated in tests/gate_np.py; the device equals it bit for bit).  Conventions as for pr_posegraph: a pose is [R | t], 12
 * doubles row-major, world to camera; A B = [R_A R_B | R_A t_B + t_A]; A^-1 = [R^T | -(R^T t)]; a closure (i, j, Z) measures
 * Z ~ P_i P_j^-1.  fp64, + and x only, no contraction.  A 3 x 3 product entry is (a0 b0 + a1 b1) + a2 b2; the translation of a product
 * is ((r0 t0 + r1 t1) + r2 t2) + t_A, of an inverse -((R0r t0 + R1r t1) + R2r t2); R^T is formed first and then multiplied like any
 * other matrix.
 *   1. Counts.  E = src.state[0] clamped into 0 .. edge_capacity, n = d_n[0] clamped into 0 .. node_capacity, both before any address
 *      is formed from them.
 *   2. Valid edges.  Edge a < E is valid iff 0 <= i, j < n, i != j, its 12 Z entries and 2 weights are finite and the 24 entries of
 *      P_i, P_j are finite: exactly the relaxation's skip rule.
 *   3. Per valid edge.  L_a = Z_a^-1 P_ia, M_a = (P_ia^-1 Z_a) P_ja, N_a = P_ja^-1.
 *   4. Ordered pairs.  For an ordered pair a != b of valid edges: gap = |i_a - i_b| + |j_a - j_b|.  The pair is comparable iff
 *      gap <= max_gap and j_a != j_b (two candidates of one query keyframe are not independent evidence).  X = (L_a M_b) N_a - that is
 *      Z_a^-1 (P_ia P_ib^-1) Z_b (P_jb P_ja^-1) re-associated: the identity when both closures agree with each other along the odometry
 *      between them.  c_rot = 3 - ((X00 + X11) + X22) (= 2 (1 - cos theta)), c_trans = (tx tx + ty ty) + tz tz.  b supports a iff the
 *      pair is comparable, c_rot <= rot_tab[gap] and c_trans <= trans2_tab[gap].  A NaN supports nothing.  The rule is stated for ordered
 *      pairs: b supporting a need not imply the converse in floating point; it is evaluated as written.
 *   5. Rounds.  keep_0 = valid.  For r = 1 .. rounds: s_r[a] = #{b : keep_{r-1}[b], b supports a} and keep_r[a] = keep_{r-1}[a] and
 *      s_r[a] >= min_support.  The outputs are keep = keep_rounds and support[a] = s_rounds[a] for a valid a (also a removed one), -1 for
 *      an invalid a (every a >= E is invalid).  PR_GATE_UNSETTLED is set iff keep_rounds != keep_{rounds-1}; when it is clear the kept
 *      set is the min_support-core of the support relation.
 *   6. Copy.  Kept edges are copied in log order: map[a] is the rank of a among the kept, or -1; row map[a] of dst gets the bytes of
 *      row a of src (edge_ij, edge_Z, edge_w); dst.state = {kept, src.state[1] & PR_POSEGRAPH_OVERFLOW, 0, 0}; rows >= kept of dst are
 *      not written.  info = {valid, kept, E, flags}; PR_GATE_SRC_OVERFLOW mirrors the source log's overflow bit.
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL pointer or a NULL buffer of either record, src and dst sharing
 * a buffer, node_capacity outside 1 .. 2^20, edge_capacity outside 1 .. 65536, dst_edge_capacity < edge_capacity, max_gap outside
 * 0 .. 65535, min_support < 0, rounds outside 1 .. 64, and a table entry that is NaN or negative (+Inf is allowed and switches that test
 * off). */
typedef struct pr_gate pr_gate;
typedef struct pr_gate_params { int32_t max_gap, min_support, rounds; } pr_gate_params;
#define PR_GATE_SRC_OVERFLOW 1
#define PR_GATE_UNSETTLED 2
int pr_gate_create(pr_ctx* ctx, const pr_posegraph_buffers* src, const pr_posegraph_buffers* dst, int32_t node_capacity, int32_t edge_capacity,
                   int32_t dst_edge_capacity, const pr_gate_params* params, const double* rot_tab, const double* trans2_tab, pr_gate** out);
int pr_gate_run_dev(pr_gate* g, const double* d_poses, const int32_t* d_n, uint8_t* d_keep, int32_t* d_support, int32_t* d_map, int32_t* d_info);
int pr_gate_run(pr_gate* g, const double* d_poses, const int32_t* d_n, uint8_t* keep, int32_t* support, int32_t* map, int32_t* info);
size_t pr_gate_scratch_bytes(int32_t node_capacity, int32_t edge_capacity, int32_t max_gap);
void pr_gate_destroy(pr_gate* g);

/* ---- sequence matching: trajectory-summed scores and their top-k (seqmatch.hip) ------------------------------------------
 * Every other matcher answers one keyframe at a time: the row minimum of run_test.m:57.  A drive is a sequence: a true revisit is a LINE in
 * the distance matrix (query i - l matches DB row j -/+ l), a perceptual alias an isolated low cell.  The sequence form sums the fused
 * scores along short DB trajectories (SeqSLAM; Milford & Wyeth 2012) and selects on the sums, which removes aliases before any
 * verification is spent on them.
 *
 * The step table.  steps is i32 [V][L], 1 <= L <= PR_SEQ_MAX_L, 1 <= V <= PR_SEQ_MAX_V, steps[v][0] == 0, |steps[v][l]| <=
 * PR_SEQ_MAX_STEP: steps[v][l] is how many DB rows BEHIND the candidate the trajectory of velocity v lies at query lag l (negative: a
 * reverse traversal; all zeros: a standstill).  The device only indexes with it; no velocity arithmetic happens there.  A host table that
 * breaks a limit is PR_EINVAL ("bad step table"); a row of a DEVICE table that does is a dropped velocity for every cell.
 *
 *   pr_seq_select_dev   d_p, d_i f32 [m][n] and mom f64 [m][2][3]: what pr_distances_dev and pr_row_moments_dev wrote; d_steps i32 [V][L];
 *                       idx i32, score f64, vel i32 [m][k], 1 <= k <= PR_SEQ_MAX_K; d_S NULL or f64 [m][n].  All pointers are device
 *                       memory.  Stream-ordered, capturable, no read-back, no allocation: the lists of the column parts live in a block the
 *                       context allocated at create.  One launch, or two when few query rows are cut into column parts; every grid
 *                       depends on (m, n) only.  m == 0 launches nothing.
 *   pr_seq_tile         the kernel's tile: rows query rows by cols columns per workgroup and slab.
 *   pr_match_topk_seq_f64   host buffers: the shared top-k pipeline's pack + distances + moments (PR_TYPE_SC, PR_TYPE_M2DP; PR_TYPE_DELIGHT:
 *                       one matrix, the d_i == NULL form), then pr_seq_select_dev with q_row0 = db_row0 = 0.  steps is a HOST table.
 *
 * The rule (restated in tests/seqmatch_np.py; the device equals it bit for bit; fp64, no contraction).
 *   1. Cell score.  f(i, j) = p_weight * (((double)d_p[i][j] - mean_p) / sd_p) + ((double)d_i[i][j] - mean_i) / sd_i with mean = mom[i][c][1]
 *      and sd = sqrt(M2 / (count - 1.0)) = sqrt(mom[i][c][2] / (mom[i][c][0] - 1.0)): IEEE operations, every division correctly rounded.
 *      With d_i == NULL there is no normalisation: f = (double)d_p[i][j] and mom is not read (DELIGHT, GIST and BoW distance matrices).
 *   2. Masked cells.  Cell (a, c) is masked iff |(q_row0 + a) - (db_row0 + c)| < mask_width.
 *   3. Lags.  For query row i, L_i = min(L, i + 1): lags reach local rows i - l >= 0 only.  A query shard does not see earlier shards.
 *   4. Sum per velocity.  S_v(i, j) = sum over l = 0 .. L_i - 1, added in ascending l from 0.0, of f(i - l, j - steps[v][l]).
 *   5. Dropped velocities.  A velocity is dropped for the cell if any term's column lies outside 0 .. n - 1, any term's own cell is
 *      masked, any term is NaN, or the sum is NaN.  +/-Inf terms add by IEEE.
 *   6. Cell result.  S(i, j) = min over the kept v of S_v / (double)L_i, strict <, so the first v wins a tie.  A masked (i, j), or one
 *      with no kept velocity, is not a candidate; its d_S entry is +Inf.
 *   7. Selection.  Per row the k smallest candidates by (S, j), so the smaller j wins a tie: idx = db_row0 + j, score = S, vel = v.
 *      Missing slots are -1 / NaN / -1.
 * Scope.  The sequence form is a function of the f32 matrices pr_distances_dev wrote: it has NO fp64 re-evaluation and NO containment
 * check (pr_rerank_dev, pr_order_resolve_dev have no counterpart here), so its scores are fp32-grade in the distances.  There is no
 * velocity search beyond the table, no sharded form, and lags do not cross query shards.
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL pointer (d_p, d_steps, idx, score, vel; mom with d_i given),
 * m < 0, n < 1, V outside 1 .. 16, L outside 1 .. 32, k outside 1 .. 32, mask_width < 0. */
#define PR_SEQ_MAX_L 32
#define PR_SEQ_MAX_V 16
#define PR_SEQ_MAX_STEP 64
#define PR_SEQ_MAX_K 32
int pr_seq_select_dev(pr_ctx* ctx, const float* d_p, const float* d_i, int32_t m, int32_t n, const double* mom, const int32_t* d_steps,
                      int32_t V, int32_t L, int32_t q_row0, int32_t db_row0, int32_t mask_width, double p_weight, int32_t k, int32_t* idx,
                      double* score, int32_t* vel, double* d_S);
void pr_seq_tile(int32_t* rows, int32_t* cols);
int pr_match_topk_seq_f64(pr_ctx* ctx, int type, const double* h1, int32_t m, const double* h2, int32_t n, int32_t mask_width, double p_weight,
                          int32_t k, const int32_t* steps, int32_t V, int32_t L, int32_t* idx, double* score, int32_t* vel);

/* The online form: one keyframe per captured step.  A pr_seqmatch is a handle over a ring of the last L fused score rows.
 *   pr_seqmatch_create     makes ONE allocation (steps is a HOST table); no later call allocates, every grid depends on the create sizes
 *                          only.  With B = ceil(capacity / 256) and K = max_k the parts are, each rounded up to 16 bytes:
 *                            8 L capacity (the ring [L][capacity] f64) | 4 L (the slots' row ids) | 16 (the push counter) | 64 (row
 *                            statistics) | 16 (control) | 4 V L (the step table) | 8 B K | 4 B K | 4 B K (the workgroups' lists)
 *                            | staging of the host form: 8 channels capacity | 16 | 8 K | 4 K | 4 K | 16
 *                          pr_seqmatch_scratch_bytes returns the sum (0 for sizes create refuses).
 *   pr_seqmatch_push_dev   three launches, no read-back.  d_rows f64 [channels][capacity] is exactly what pr_online_match_dev /
 *                          pr_onlineset_match_dev write as their rows; d_count [>= 1] i32 is the database's state (word 0: its count);
 *                          d_emitted NULL or [>= 1] i32; weights is a HOST array [channels] (its values enter the launch: a captured push
 *                          keeps them); d_idx i32, d_score f64, d_vel i32 [k]; d_info i32 [4].
 *   pr_seqmatch_push       the same over HOST rows [channels][capacity], a host count and host outputs; synchronises.
 *   pr_seqmatch_reset      stream-ordered: ring, row ids and counter back to zero bytes.
 *   pr_seqmatch_read       ring [L][capacity], row ids [L] and the counter to the host (any may be NULL); synchronises.
 * The rule (tests/seqmatch_np.py SeqFilter restates it):
 *   1. Switched off.  d_emitted != NULL && d_emitted[0] == 0 writes -1 / NaN / -1 and info = {0, 0, pushes, 0}.  The ring, the row ids
 *      and the counter do not change by a byte.
 *   2. Row formed and stored.  Otherwise n = count clamped into 0 .. capacity before any address is formed from it.  The fused row is
 *      F_n[j] for j < n.  normalize = 1: F = sum_c weights[c] * z_c, added in ascending c from 0.0, z_c = (rows[c][j] - mean_c) / sd_c, the
 *      row z-score over the non-NaN j < n: count_c of them, mean_c = sum / count_c, M2_c = sum of (x - mean_c)^2, sd_c = sqrt(M2_c /
 *      (count_c - 1.0)).  The order of both sums is fixed by n alone: partial sum t of 256 adds the non-NaN entries j = t, t + 256, ..
 *      in ascending j from 0.0; then p[t] += p[t + s] for s = 128, 64, .. 1; the sum is p[0].  normalize = 0 needs channels == 1 and gives
 *      F = rows[0].  The row is stored in slot (pushes mod L) - columns >= n of the slot keep their bytes - together with n; the counter
 *      is committed by one thread.  The payload of a NaN that arithmetic produced is not specified.
 *   3. Sequence score.  L_n = min(L, pushes so far including this one).  S(n, j) follows the batch rule 4 - 6 with lag l the l-th earlier
 *      PUSHED row, of row id n_l: its term needs 0 <= c < n_l and |n_l - c| >= mask_width with c = j - steps[v][l]; lag 0 is F_n[j].  The
 *      query is row n, as in pr_online: selection is the k smallest by (S, j) over j < n with n - j >= mask_width; idx = j.
 *   4. Info.  info = {pushed, L_n, pushes after, 0}.  n < 2 with normalize = 1 leaves every slot -1 / NaN / -1 and still counts as a push
 *      (of an all-NaN row).
 * PR_EINVAL before any device is touched for NULL pointers, capacity outside 1 .. 2^24, channels outside {1, 2, 4}, a bad step table, k
 * outside 1 .. max_k or max_k outside 1 .. PR_SEQMATCH_MAX_K, a non-finite weight, mask_width < 0, normalize outside {0, 1}, and
 * normalize = 0 with channels != 1. */
#define PR_SEQMATCH_MAX_K 128
typedef struct pr_seqmatch pr_seqmatch;
int pr_seqmatch_create(pr_ctx* ctx, int32_t capacity, int32_t channels, const int32_t* steps, int32_t V, int32_t L, int32_t max_k,
                       pr_seqmatch** out);
int pr_seqmatch_push_dev(pr_seqmatch* s, const double* d_rows, const int32_t* d_count, const int32_t* d_emitted, const double* weights,
                         int32_t normalize, int32_t mask_width, int32_t k, int32_t* d_idx, double* d_score, int32_t* d_vel, int32_t* d_info);
int pr_seqmatch_push(pr_seqmatch* s, const double* rows, int32_t count, const double* weights, int32_t normalize, int32_t mask_width, int32_t k,
                     int32_t* idx, double* score, int32_t* vel, int32_t* info);
int pr_seqmatch_reset(pr_seqmatch* s);
int pr_seqmatch_read(pr_seqmatch* s, double* ring, int32_t* ids, int32_t* pushes);
size_t pr_seqmatch_scratch_bytes(int32_t capacity, int32_t channels, int32_t V, int32_t L, int32_t max_k);
void pr_seqmatch_destroy(pr_seqmatch* s);
const char* pr_host_last_error(void);

/* ---- registration information: covariance, weak directions, edge weights (reginfo.hip; no reference counterpart) ------
 * A registration result is a pose and two scalars, fitness and rmse; how well the geometry constrains that pose is not in them.  A
 * pr_reginfo reports it: the 6 x 6 normal matrix H of the metric at the pose T that is to be judged, Sigma = H^-1, the spectra of the
 * marginal covariances of rotation and translation with their weakest directions, a graded weakness test and a per-slot (w_rot, w_trans)
 * that pr_posegraphw_add_dev takes from device memory.  It runs BEHIND a correspondence pass the caller has already made at T:
 * the CSR triple (d_out_offs [c + 1], d_nn_idx, d_nn_d2) that pr_icp_nn_radius_dev, pr_icp_nn_dev or pr_maploc_nn_dev wrote.  Every
 * device call is stream-ordered on the context's stream, reads nothing back, allocates nothing and can be captured: two launches whose
 * grids depend on the create sizes and c only.  fp64 without contraction; no floating-point atomics; no workgroup waits for another.
 *
 *   pr_reginfo_create     ONE allocation; no later call allocates.  With ld = max(max_src_pts, 1), nchunks = ceil(ld / 256) and pc =
 *                         pair_capacity the parts are, each rounded up to 16 bytes:
 *                           200 pc nchunks (chunk partials [pc][nchunks][25] f64) | staging of the host forms: 24 pc ld (xyz_q) |
 *                           8 (pc + 1) (offs_q) | 4 pc (pair_src) | 96 pc (T) | pc (accepted) | 8 (pc + 1) (out_offs) | 4 pc ld (nn_idx)
 *                           | 8 pc ld (nn_d2) | 24 pc ld (world_xyz) | 24 pc ld (normals) | 4 pc ld (ninfo) | 288 pc (H) | 288 pc (cov)
 *                           | 128 pc (spec) | 16 pc (w) | 16 pc (stat) | pc (ok)
 *                         pr_reginfo_scratch_bytes(pair_capacity, max_src_pts) returns the sum (0 for sizes create refuses:
 *                         pair_capacity outside 1 .. 65535, max_src_pts outside 0 .. 2^26).  pr_reginfo_destroy frees the handle.
 *   pr_reginfo_point_dev  the point metric e = p' - q; it needs no target cloud.
 *   pr_reginfo_plane_dev  the plane metric r = n . (p' - q); the same arguments plus d_world_xyz [out_capacity][3], out_capacity and the
 *                         d_normals [out_capacity][3] f64 / d_ninfo [out_capacity] i32 that pr_mapplane_normals_dev wrote.
 *   pr_reginfo_point / _plane   the host forms: upload, run the device form, synchronise, read back.  They stage through the handle's
 *                         allocation, so Nq <= pair_capacity, offs_q[Nq] <= pair_capacity x ld, out_offs[c] <= pair_capacity x ld and
 *                         out_capacity <= pair_capacity x ld are required, and offs_q and out_offs ascend from a value >= 0.
 *
 * The rule (restated in fp64 in tests/reginfo_np.py).
 *   Points read.  Slot p with src = d_pair_src[p] reads ns = min(out_offs[p + 1] - out_offs[p], offs_q[src + 1] - offs_q[src],
 *     max_src_pts) points, never less than 0: source row offs_q[src] + i with the correspondence at out_offs[p] + i.
 *   Inliers.  Point i is an inlier iff nn_idx >= 0 and nn_d2 < fl(max_corr^2) - and, for the plane metric, nn_idx < out_capacity, which
 *     is checked before an address is formed.  For an inlier, with T = d_T[p] = [R | t]: p' = T s in pr_icp_pairs_dev's association,
 *     p'_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a; u = p' - t, the lever arm about the sensor position (no world-sized coordinate enters a
 *     product).
 *   Point sums (11): the count n, sum d2 (the pass's nn_d2), sum u_a (3) and sum u_a u_b (6: 00 01 02 11 12 22).  With e = p' - q and
 *     J = [-[u]x | I] in the order (w0, w1, w2, v0, v1, v2) the finish assembles H = sum J^T J from them: H_ww = (tr S) I - S with S =
 *     sum u u^T - a diagonal entry is the sum of the OTHER two diagonal sums, H_00 = S_11 + S_22, H_11 = S_00 + S_22, H_22 = S_00 + S_11,
 *     an off-diagonal entry -S_ab -; H_wv = [sum u]x (H_vw its transpose); H_vv = n I.  SSE = sum d2, n_used = n, dof = 3 n - 6.
 *   Plane sums (25): the inliers n_inl, sum d2, the plane correspondents n_pl (inliers with ninfo[j] > 0), sum r^2 and the 21 entries
 *     of sum J J^T (upper triangle, row-major), with q = world_xyz[j], n = normals[j], e = p' - q, r = (n_0 e_0 + n_1 e_1) + n_2 e_2
 *     and J = [u x n, n] exactly as pr_mapplane_refine_dev forms them.  H = sum J J^T, SSE = sum r^2, n_used = n_pl, dof = n_pl - 6.
 *   Reduction.  The project's fixed tree: a chunk is 256 source points; within a wave a 64-lane shuffle tree (v += the value of lane + d for d = 32,
 *     16, .. 1), then the four waves in order ((w0 + w1) + w2) + w3; the chunk results go to the handle's partials and are added from
 *     0.0 in chunk index order.
 *   Finish, per slot, in this order; the first rule that applies ends it, and what later steps would have produced is zero:
 *     1. PR_REGINFO_OFF when pair_src[p] is outside 0 .. Nq - 1, when d_accepted != NULL and d_accepted[p] == 0, or when the slot's
 *        span out_offs[p + 1] - out_offs[p] is <= 0 (the pass switched it off, or its cloud is empty).  stat = {0, 0, 0, OFF}.
 *     2. PR_REGINFO_NONFINITE when one of the 12 entries of T or one of the sums is not finite.  stat carries n_inl, n_used and dof
 *        (counts are always finite); H and SSE are zero.
 *     3. H and SSE are written.  PR_REGINFO_TOO_FEW when n_used < min_inliers or dof <= 0.
 *     4. L D L^T of H without pivoting in pr_mapplane_refine_dev's order: d_k = H_kk - sum_m<k (L_km d_m) L_km, L_ik = (H_ik - sum_m<k
 *        (L_im d_m) L_km) / d_k, every sum subtracted term by term with m ascending.  PR_REGINFO_SINGULAR when a d_k is not finite or
 *        not d_k > 1e-12 H_kk (the original diagonal entry), or when an entry of Sigma below is not finite.
 *     5. Sigma = H^-1 by six solves; column j from the unit vector e_j: y_i = (e_j)_i - sum_m<i L_im y_m (m ascending), z_i = y_i / d_i,
 *        x_i = z_i - sum_m>i L_mi x_m for i = 5 .. 0 (m ascending); Sigma_ij = x_i.  cov holds Sigma as computed, row-major.
 *     6. The marginal covariances are the blocks Sigma_ww (rows and columns 0 .. 2) and Sigma_vv (3 .. 5): they are the inverses of the
 *        marginal informations, so no Schur complement is formed.  Each block's upper triangle, mirrored, is decomposed by
 *        pr_mapplane_normals_dev's cyclic Jacobi (8 sweeps, pivots (0,1), (0,2), (1,2), V = I at the start, the same rotation and the
 *        same stable ascending sort by three compare-exchanges): cr0 <= cr1 <= cr2 and ct0 <= ct1 <= ct2.  The weakest directions dir_r
 *        and dir_t are the eigenvectors (columns of V) of cr2 and ct2, every component divided by sqrt((e0 e0 + e1 e1) + e2 e2), the sign
 *        chosen so that the component of largest magnitude is positive (the lowest index wins a tie).
 *     7. PR_REGINFO_WEAK_ROT iff NOT cr0 >= min_ratio cr2; PR_REGINFO_WEAK_TRANS iff NOT ct0 >= min_ratio ct2.
 *     8. s2 = max(SSE / dof, sigma_min^2) (q > sigma_min^2 ? q : sigma_min^2).  w_rot = x < w_max ? x : w_max with x = 1 / (s2 cr2);
 *        w_trans the same with ct2.  Both are exactly 0.0 when any flag is set.  The weights are in the units of the pose graph's
 *        residual (rad^-2 and length^-2): with u about the sensor position a perturbation Z' = [Exp(w) R | t + v] moves the residual of
 *        pr_posegraph_relax_dev by -R^T w and -R^T v at first order, a rotation of each block, so a scalar per block is frame-correct;
 *        the largest marginal eigenvalue is the conservative scalar.
 *   Outputs (the caller's arrays; every entry of rows < c is written): d_H [c][36] and d_cov [c][36] row-major; d_spec [c][16] = {cr0,
 *     cr1, cr2, ct0, ct1, ct2, dir_r (3), dir_t (3), SSE, s2, 0, 0}; d_w [c][2] = {w_rot, w_trans}; d_stat [c][4] i32 = {n_inl, n_used,
 *     dof, flags}; d_ok [c] u8 = (flags == 0).
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle or required pointer, c outside 0 .. pair_capacity,
 * Nq < 0, max_corr or sigma_min not positive and finite, min_ratio outside [0, 1], w_max not positive or NaN (+Inf is allowed),
 * min_inliers < 3 for the point metric and < 6 for the plane metric, out_capacity outside 1 .. 2^29 (plane).  c = 0 is valid. */
typedef struct pr_reginfo pr_reginfo;
enum { PR_REGINFO_OFF = 1, PR_REGINFO_NONFINITE = 2, PR_REGINFO_TOO_FEW = 4, PR_REGINFO_SINGULAR = 8, PR_REGINFO_WEAK_ROT = 16,
       PR_REGINFO_WEAK_TRANS = 32 };
int pr_reginfo_create(pr_ctx* ctx, int32_t pair_capacity, int32_t max_src_pts, pr_reginfo** out);
void pr_reginfo_destroy(pr_reginfo* ri);
int64_t pr_reginfo_scratch_bytes(int32_t pair_capacity, int32_t max_src_pts);
int pr_reginfo_point_dev(pr_reginfo* ri, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                         const double* d_T, const uint8_t* d_accepted, const int64_t* d_out_offs, const int32_t* d_nn_idx, const double* d_nn_d2,
                         double max_corr, int32_t min_inliers, double min_ratio, double sigma_min, double w_max, double* d_H, double* d_cov,
                         double* d_spec, double* d_w, int32_t* d_stat, uint8_t* d_ok);
int pr_reginfo_plane_dev(pr_reginfo* ri, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                         const double* d_T, const uint8_t* d_accepted, const int64_t* d_out_offs, const int32_t* d_nn_idx, const double* d_nn_d2,
                         const double* d_world_xyz, int64_t out_capacity, const double* d_normals, const int32_t* d_ninfo, double max_corr,
                         int32_t min_inliers, double min_ratio, double sigma_min, double w_max, double* d_H, double* d_cov, double* d_spec,
                         double* d_w, int32_t* d_stat, uint8_t* d_ok);
int pr_reginfo_point(pr_reginfo* ri, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T,
                     const uint8_t* accepted, const int64_t* out_offs, const int32_t* nn_idx, const double* nn_d2, double max_corr,
                     int32_t min_inliers, double min_ratio, double sigma_min, double w_max, double* H, double* cov, double* spec, double* w,
                     int32_t* stat, uint8_t* ok);
int pr_reginfo_plane(pr_reginfo* ri, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T,
                     const uint8_t* accepted, const int64_t* out_offs, const int32_t* nn_idx, const double* nn_d2, const double* world_xyz,
                     int64_t out_capacity, const double* normals, const int32_t* ninfo, double max_corr, int32_t min_inliers, double min_ratio,
                     double sigma_min, double w_max, double* H, double* cov, double* spec, double* w, int32_t* stat, uint8_t* ok);

/* The pose-graph log with weights from the device (posegraph.hip): two more calls on a pr_posegraph, named
 * pr_posegraphw_* as pr_onlineset_* stands beside pr_online_* - the pr_posegraph_* family above is closed.
 *   pr_posegraphw_add_dev   pr_posegraph_add_dev's rule slot for slot - the same launch geometry, overflow rule, info, switch-off
 *                         by a negative query_row and clamp of a scribbled count - with (w_rot, w_trans) = d_w[p] ([k][2] f64 in DEVICE
 *                         memory: pr_reginfo's d_w) and ONE more condition for logging slot p: both of its weights are finite and >= 0.
 *                         With every d_w[p] = (w_rot, w_trans) it leaves the bytes pr_posegraph_add_dev leaves.
 *   pr_posegraphw_add       the host form: host arrays, query_row by value, w [k][2] host; uploads, runs the device path,
 *                         synchronises.
 * PR_EINVAL before any device is touched for a NULL handle or pointer and k outside 1 .. 128. */
int pr_posegraphw_add_dev(pr_posegraph* g, const int32_t* d_idx, const double* d_T, const uint8_t* d_accepted, const int32_t* d_query_row,
                                  int32_t k, const double* d_w, int32_t* d_info);
int pr_posegraphw_add(pr_posegraph* g, const int32_t* idx, const double* T, const uint8_t* accepted, int32_t query_row, int32_t k,
                              const double* w, int32_t* info);

/* ---- trajectory evaluation against ground truth (trajeval.hip) ------------------------------------------------------------
 * What the loop-closure back end is for is a better trajectory; a pr_trajeval measures one: the absolute trajectory error (ATE) under an
 * alignment, the relative pose error (RPE) per row delta, KITTI's odometry metric over segments of given path lengths, and the error of
 * every logged closure against the ground truth - for B candidate pose arrays a call.  Everything is stream-ordered, reads every count on
 * the device, allocates nothing after create and uses no floating-point atomics; every grid is a function of the create sizes only, so one
 * capture made at n = 0 serves every count, and one graph gate -> relax -> evaluate can be replayed per parameter setting.
 *
 *   pr_trajeval_create   params: node_capacity (cap) 1 .. 2^20, batch (B) 1 .. 64, align PR_TRAJ_ALIGN_*, gt_kind PR_TRAJ_GT_*, n_deltas (K)
 *                        0 .. 8, n_lengths (L) 0 .. 8, step >= 1 (rows between segment starts), edge_capacity (EC) 0 .. 65536 (0: no closure
 *                        metric), rot_thr (radians) and trans_thr of a WRONG closure.  deltas [K] i32, each >= 1, and lengths [L] f64, each
 *                        finite and > 0, are HOST tables; create uploads them and allocates ALL scratch in one block.  With
 *                        slots = ceil(cap / step) the parts are, each rounded up to 16 bytes:
 *                          4 B cap (used) | 4 cap (gt used) | 24 (B + 1) cap (centres) | 16 B cap (prefixes) | 128 B (S)
 *                          | 32 B L (the lengths' segment sums) | 32 | 64 (tables)
 *                          | staging of the host form: 192 B (ate) | 64 B K (rpe) | 32 B (L + 1) (seg) | 64 (clo) | 8 B cap (err)
 *                          | 4 B slots L (seg_end) | 16 EC (edge_err)
 *                        pr_trajeval_scratch_bytes returns the sum (0 for sizes create refuses).
 *   pr_trajeval_run_dev  2 launches, + 1 with K > 0, + 2 with L > 0, + 1 with a log.  d_est [B][cap][12] f64: rows as pr_map_buffers.poses
 *                        (world to camera, row-major [R | t]).  d_n [>= 1] i32: a pr_map's state.  d_gt: [cap][12] f64 in the est's
 *                        convention (PR_TRAJ_GT_W2C), [cap][12] camera to world - KITTI's file rows - (PR_TRAJ_GT_C2W) or [cap][3]
 *                        positions (PR_TRAJ_GT_POSITIONS).  d_valid [cap] u8 or NULL (every row valid).  log: the buffer record of a
 *                        pr_posegraph (edge_ij, edge_Z, state are read; edge_w is not) or NULL: no closure metric in this call; it needs
 *                        EC > 0 and at most EC edges are read.  out: a record of DEVICE pointers.  ate is required, rpe with K > 0, seg with
 *                        L > 0, clo with a log; the other five may be NULL.  Every entry of every given array is written.  No read-back.
 *   pr_trajeval_run      the same with HOST arrays in `out` (d_est, d_n, d_gt, d_valid and the log stay device memory); synchronises.
 *
 * The rule (restated operation by operation in tests/trajeval_np.py; the device equals it bit for bit except where atan2 enters).
 * Conventions as for pr_gate: A B = [R_A R_B | R_A t_B + t_A]; A^-1 = [R^T | -(R^T t)]; fp64, no contraction; a 3 x 3 product entry is
 * (a0 b0 + a1 b1) + a2 b2, the translation of a product ((r0 t0 + r1 t1) + r2 t2) + t_A, of an inverse -((R0r t0 + R1r t1) + R2r t2);
 * |x| = sqrt((x0 x0 + x1 x1) + x2 x2); a cross product entry is a b - c d.
 *   THE TREE.  Every floating-point sum over rows (pairs, slots, edges) i = 0 .. M - 1 is formed as: 256 lane sums, lane t adding its terms
 *      i = t, t + 256, t + 512, ... in that order to +0.0, a term that does not count adding +0.0; then for s = 128, 64, .. 1 lane t < s
 *      becomes lane t + lane (t + s); the sum is lane 0.  A maximum starts at 0.0.
 *   0. Counts and rows.  n = d_n[0] clamped into 0 .. cap, E = log.state[0] clamped into 0 .. EC, both before any address is formed.
 *      gt row i is USED iff i < n, valid[i] != 0 (or valid is NULL) and its 12 (3) entries are finite; row i of candidate b is used iff
 *      its gt row is used and the 12 entries of est row (b, i) are finite.
 *   1. Centres.  Of a W2C row -(R^T t); of a C2W row t; of a position row the row.  out.centres [B + 1][cap][3]: the est centres of every
 *      b, then the gt centres; zeros for a row that is not used.
 *   2. Alignment S = (s, R, t) per b over its N used rows; x = est centre, y = gt centre.  flags: PR_TRAJ_FEW iff N < 3.
 *      NONE: S = (1, I, 0).  FIRST: with f the first used row, (R, t) = G_f^-1 P_f (W2C gt) or G_f P_f (C2W gt), s = 1; the identity if
 *      N = 0.  SE3, SIM3 with N < 3: the identity.  SE3, SIM3 with N >= 3 (Umeyama):
 *        mx = (tree sum of x) / N, my likewise; then A = (tree sum of (y - my)(x - mx)^T) / N entry by entry and
 *        var_x = (tree sum of ((dx0 dx0 + dx1 dx1) + dx2 dx2)) / N with dx = x - mx: the second pass is centred, a route at a UTM northing
 *        does not cancel.
 *        hmax = max |A_rc|.  If hmax is 0 or not finite: R = I, sigma = 0, DEGENERATE.  Else G = A / hmax, V = I and 10 sweeps, each:
 *        W = G V (formed afresh), then for (p, q) = (0, 1), (0, 2), (1, 2): al = |w_p|^2, be = |w_q|^2, ga = w_p . w_q (all three
 *        (a + b) + c); skipped unless ga ga > 1e-31 (al be); zeta = (be - al) / (2 ga); t = sign(zeta) / (|zeta| + sqrt(zeta zeta + 1))
 *        (sign(0) = +1); cs = 1 / sqrt(t t + 1); sn = t cs; columns p, q of W and of V become (cs x - sn y, sn x + cs y).  After the
 *        sweeps W = G V once more, m_k = |w_k|^2, and the columns of W and V are ordered by exchanging (0, 1), (1, 2), (0, 1), each iff
 *        m_j < m_k.  n_k = sqrt(m_k), sigma_k = n_k hmax.  PR_TRAJ_DEGENERATE iff not n_2 > 1e-12 n_1 (a straight road, a standstill).
 *        u_1 = w_1 / n_1.  u_2 = w_2 - (w_2 . u_1) u_1, divided by its norm; when DEGENERATE w_2 is replaced by the unit vector of the
 *        axis k on which |u_1[k]| is smallest (the lowest k on a tie), so S is still a rigid map taking the line onto the line.
 *        u_3 = u_1 x u_2; v_3' = v_1 x v_2 divided by its norm.  d = -1 iff not DEGENERATE and (u_3 . w_3)(v_3' . v_3) < 0, else +1: the
 *        sign of det U det V, D = diag(1, 1, d).  R_ab = (u_1a v_1b + u_2a v_2b) + u_3a v_3'b  (= U D V^T).
 *        PR_TRAJ_NO_SCALE iff not var_x > 0; s = ((sigma_1 + sigma_2) + d sigma_3) / var_x for SIM3 without NO_SCALE, else 1.
 *        t = my - s (R mx).
 *   3. ATE.  e_i = |y_i - (s (R x_i) + t)| with the parenthesis formed entry by entry as written.  out.err [B][cap]: e_i, -1 for a row
 *      that is not used.  out.ate [B][24] = N, sse (tree sum of e_i^2 BEFORE the square root), rmse = sqrt(sse / N), mean = (tree sum of
 *      e_i) / N, max, argmax (the lowest row on a tie; -1 with N = 0), s, R (9), t (3), flags, sigma_1 .. sigma_3, var_x; statistics of
 *      N = 0 are zeros.
 *   4. RPE per b and delta.  Pairs (i, i + delta), i + delta < n, both rows used.  rel_est = P_i P_j^-1 with its translation multiplied
 *      by s entry by entry (s = 1 unless SIM3); rel_gt = G_i G_j^-1 (W2C) or G_i^-1 G_j (C2W); E = rel_gt^-1 rel_est.  tr = (E00 + E11) +
 *      E22; c_rot = 3 - tr; v = (0.5 (E21 - E12), 0.5 (E02 - E20), 0.5 (E10 - E01)); theta = atan2(|v|, 0.5 (tr - 1)); d = |t_E|.
 *      out.rpe [B][K][8] = pairs, sqrt((tree sum of d d) / pairs), mean d, max d, sqrt((tree sum of theta theta) / pairs), mean theta,
 *      max theta, mean c_rot; zeros without a pair.
 *   5. Segments per b.  Over the used rows dist[i] = dist[i - 1] + |y_i - y_prev used| (an unused row and the first used row add nothing)
 *      and the same over x, in a BLOCKED order: C = ceil(cap / 256); block t holds rows t C .. t C + C - 1; w[i] is the running sum inside
 *      the block from +0.0 in row order; base[t] the running sum of the totals of blocks 0 .. t - 1 from +0.0 in block order; dist[i] =
 *      base[t] + w[i].  out.prefix [B][2][cap]: gt, then est.  For every start row f = 0, step, 2 step, .. that is used and every length:
 *      the end is the FIRST row j > f, j < n, with dist[j] > dist[f] + len (strict: a standstill never ends a segment); the segment is
 *      dropped if there is no such row or the row is not used.  With E of 4 between f and j: t_err = d / len, r_err = theta / len,
 *      ratio = (dist_est[j] - dist_est[f]) / (dist[j] - dist[f]).  out.seg [B][L + 1][4] = segments, mean t_err, mean r_err, mean ratio
 *      per length (tree sums over the slots f / step), and in row L over all segments: the lengths' tree sums added in table order from
 *      +0.0, divided by the total count; zeros without a segment.  out.seg_end [B][slots][L] i32: the end row or -1.
 *   6. Closures, once.  Edge a < E is evaluated iff 0 <= i, j < n, i != j, both gt rows are used and the 12 entries of Z are finite.
 *      Z_gt = rel_gt of 4 between i and j; E = Z_gt^-1 Z; theta and d as in 4.  out.edge_err [EC][2] = (theta, d) or (-1, -1).
 *      out.clo [8] = evaluated, wrong = #{theta > rot_thr or d > trans_thr}, sqrt((tree sum of theta theta) / evaluated), max theta,
 *      sqrt((tree sum of d d) / evaluated), max d, E, 0.
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, params, required pointer, table or log buffer, a size
 * outside the ranges above, a delta < 1, a length that is not finite and > 0, a threshold that is NaN or negative, PR_TRAJ_GT_POSITIONS
 * with K > 0, L > 0, EC > 0 or PR_TRAJ_ALIGN_FIRST (positions carry no rotation), and a log with EC = 0. */
typedef struct pr_trajeval pr_trajeval;
typedef struct pr_trajeval_params {
  int32_t node_capacity, batch, align, gt_kind, n_deltas, n_lengths, step, edge_capacity;
  double rot_thr, trans_thr;
} pr_trajeval_params;
typedef struct pr_trajeval_out {
  double* ate; double* rpe; double* seg; double* clo; double* err; int32_t* seg_end; double* edge_err; double* centres; double* prefix;
} pr_trajeval_out;
#define PR_TRAJ_ALIGN_NONE 0
#define PR_TRAJ_ALIGN_FIRST 1
#define PR_TRAJ_ALIGN_SE3 2
#define PR_TRAJ_ALIGN_SIM3 3
#define PR_TRAJ_GT_W2C 0
#define PR_TRAJ_GT_C2W 1
#define PR_TRAJ_GT_POSITIONS 2
#define PR_TRAJ_FEW 1
#define PR_TRAJ_DEGENERATE 2
#define PR_TRAJ_NO_SCALE 4
#define PR_TRAJ_ATE_STATS 24
#define PR_TRAJ_RPE_STATS 8
#define PR_TRAJ_SEG_STATS 4
#define PR_TRAJ_CLO_STATS 8
int pr_trajeval_create(pr_ctx* ctx, const pr_trajeval_params* params, const int32_t* deltas, const double* lengths, pr_trajeval** out);
int pr_trajeval_run_dev(pr_trajeval* te, const double* d_est, const int32_t* d_n, const void* d_gt, const uint8_t* d_valid,
                        const pr_posegraph_buffers* log, const pr_trajeval_out* out);
int pr_trajeval_run(pr_trajeval* te, const double* d_est, const int32_t* d_n, const void* d_gt, const uint8_t* d_valid,
                    const pr_posegraph_buffers* log, const pr_trajeval_out* out);
size_t pr_trajeval_scratch_bytes(const pr_trajeval_params* params);
void pr_trajeval_destroy(pr_trajeval* te);

/* ---- pose-proximity loop-closure candidates (proximity.hip) -----------------------------------------------------------------
 * The appearance matchers propose closures from signatures; a pr_proximity proposes them from the poses: for every query row the EARLIER
 * keyframes whose camera centre lies within a radius that grows with the path driven between the two rows (drift) and whose viewing axis
 * agrees, one per bucket of `stride` rows (one per earlier pass of the place), the k nearest of those - with the seed T0 and the pair
 * lists pr_icp_pairs_dev takes, so that search -> pr_icp_pairs_dev (the map's CSR on both sides) -> pr_verify_select_dev ->
 * pr_posegraphb_add_dev is a chain on one stream.  Pairs the closure log already holds are marked KNOWN and switched off.
 *
 *   pr_proximity_create      node_capacity 1 .. 2^20, k_max 1 .. 32, query_capacity >= 1 with query_capacity x k_max <= 65535
 *                            (pr_icp_pairs_dev's slot limit: one search feeds one ICP call).  ONE allocation; no later call allocates:
 *                            centres and axes 24 node_capacity each, path length 8 node_capacity, validity 4 node_capacity, the runs'
 *                            lists 8 P and 4 P with P = query_capacity k_max runs, the staging of the host form 4 QK + 8 QK + 96 QK +
 *                            4 QK + 4 QK + QK + 16 with QK = query_capacity k_max, each part rounded up to 16.  runs = 1 when
 *                            ceil(query_capacity / rows) >= 128, else min(16, ceil(node_capacity / cols)), (rows, cols) =
 *                            pr_proximity_tile.  pr_proximity_scratch_bytes returns the sum (0 for sizes create refuses).
 *   pr_proximity_tile        the search kernel's tile: rows query rows per workgroup, cols DB rows per slab.
 *   pr_proximity_search_dev  4 launches on the context's stream.  d_poses [node_capacity][12] f64 (pr_map_buffers.poses), d_n i32 [>= 1]
 *                            (pr_map_buffers.state), d_qrange i32 [2] = {q0, mq}; log = the closure log or NULL, log_edge_capacity its
 *                            edge_capacity (0 .. 2^20).  Outputs: d_idx i32, d_d2 f64 [query_capacity][k]; d_T0 f64 [query_capacity k][12];
 *                            d_pair_src, d_pair_dst i32, d_known u8 [query_capacity k] (d_known may be NULL without a log); d_info i32
 *                            [4] = {rows searched, slots filled, slots known, flags}.  Every grid depends on the create sizes only;
 *                            d_n, d_qrange and the log's count are read on the device: one capture made at n = 0 serves every count
 *                            and every query range.  No floating-point atomics; two runs give the same bytes.
 *   pr_proximity_search      the same with HOST outputs (d_poses, d_n, d_qrange and the log stay device memory); synchronises.
 *
 * The rule (restated operation by operation in tests/proximity_np.py; the device equals it bit for bit).  A pose is a world-to-camera row
 * [R | t]; a 3 x 3 product entry is (a0 b0 + a1 b1) + a2 b2, the translation of a product ((r0 t0 + r1 t1) + r2 t2) + t_A, the translation
 * of an inverse -((R0a t0 + R1a t1) + R2a t2); everything is fp64 without contraction.
 *  0. n = d_n[0] clamped into 0 .. node_capacity before any address is formed; q0 = d_qrange[0], mq = d_qrange[1] clamped into
 *     0 .. query_capacity.  Output row r stands for query row q = q0 + r (64 bits).  A row is VALID iff it is < n and its 12 entries are
 *     finite.  Row r is SEARCHED iff r < mq, 0 <= q < n and row q is valid.  PR_PROXIMITY_QRANGE_CLAMPED iff d_qrange[1] was clamped or
 *     some r < mq has q outside 0 .. n - 1.
 *  1. Per valid row: centre c_i = -(R^T t), viewing axis a_i = (R[2][0], R[2][1], R[2][2]).
 *  2. Path length s[i] over the valid rows, as pr_trajeval forms dist: the first valid row and every invalid row add nothing, a valid
 *     row adds |c_i - c_prev valid| = sqrt((x x + y y) + z z); BLOCKED order: 256 blocks of C = ceil(node_capacity / 256) rows, a running
 *     sum from +0.0 inside a block, the blocks' totals summed in block order, s = base of the block + running sum.
 *  3. DB row i is a CANDIDATE of q iff both rows are valid, i + min_gap <= q, d2 < rad rad (strict) with dx = c_i - c_q,
 *     d2 = (dx0 dx0 + dx1 dx1) + dx2 dx2, rad = radius + growth (s[q] - s[i]) replaced by radius_max unless rad < radius_max (a NaN too),
 *     and, when cos_min > -1, (a_i0 a_q0 + a_i1 a_q1) + a_i2 a_q2 >= cos_min (cos_min == -1 forms no dot product).
 *  4. Bucket b = i / stride.  A bucket's representative is its candidate of smallest d2, the lowest i on a tie.  The row's result is the
 *     k representatives of smallest d2 (lowest i on a tie), ascending, in slots 0 ..; the other slots hold idx = -1, d2 = +Inf.
 *  5. A filled slot with i = idx gets T0 = P_i P_q^-1 (query-camera points into DB row i's camera frame: verify's T, the log's Z_ij),
 *     pair_src = q, pair_dst = i.  With a log: E = log.state[0] clamped into 0 .. log_edge_capacity; the slot is KNOWN iff some edge
 *     a < E has both indices >= 0 and, with lo = min(i_a, j_a), hi = max(i_a, j_a), |lo - i| <= known_window and |hi - q| <=
 *     known_window.  A KNOWN slot keeps idx and d2 but gets pair_src = pair_dst = -1, T0 = identity, known = 1 (pr_icp_pairs_dev answers
 *     PR_ICP_NO_PAIR: nothing is logged twice).  An empty slot, and every slot of a row that is not searched, is
 *     -1 / +Inf / identity / -1 / -1 / 0.
 *  6. EVERY entry of the outputs' extents above is written, nothing beyond them.
 * PR_EINVAL (text: pr_last_error) before any device is touched: a NULL handle, params or required pointer ("pr_proximity_search_dev: a
 * required pointer is NULL ..."), sizes outside the limits above, radius not finite and positive, growth negative or not finite,
 * radius_max not finite or below radius, cos_min outside -1 .. 1, min_gap < 1, stride < 1, k outside 1 .. k_max, known_window < 0,
 * log_edge_capacity outside 0 .. 2^20, a log with a NULL buffer or without d_known. */
typedef struct pr_proximity pr_proximity;
typedef struct pr_proximity_params {
  double radius, growth, radius_max, cos_min;
  int32_t min_gap, stride, k, known_window;
} pr_proximity_params;
enum { PR_PROXIMITY_QRANGE_CLAMPED = 1 };
int pr_proximity_create(pr_ctx* ctx, int32_t node_capacity, int32_t query_capacity, int32_t k_max, pr_proximity** out);
void pr_proximity_destroy(pr_proximity* px);
int64_t pr_proximity_scratch_bytes(int32_t node_capacity, int32_t query_capacity, int32_t k_max);
void pr_proximity_tile(int32_t* rows, int32_t* cols);
int pr_proximity_search_dev(pr_proximity* px, const double* d_poses, const int32_t* d_n, const int32_t* d_qrange, const pr_proximity_params* params,
                            const pr_posegraph_buffers* log, int32_t log_edge_capacity, int32_t* d_idx, double* d_d2, double* d_T0,
                            int32_t* d_pair_src, int32_t* d_pair_dst, uint8_t* d_known, int32_t* d_info);
int pr_proximity_search(pr_proximity* px, const double* d_poses, const int32_t* d_n, const int32_t* d_qrange, const pr_proximity_params* params,
                        const pr_posegraph_buffers* log, int32_t log_edge_capacity, int32_t* idx, double* d2, double* T0, int32_t* pair_src,
                        int32_t* pair_dst, uint8_t* known, int32_t* info);

/* The batch add of the closure log (posegraph_batch.hpp, compiled into posegraph.hip): slot p = 0 .. c - 1 carries its own rows, so the pair lists of a pr_proximity search
 * (d_pair_dst as d_i, d_pair_src as d_j) are logged by ONE call.  Slot p is logged iff accepted[p] != 0, d_i[p] >= 0, d_j[p] >= 0,
 * d_i[p] != d_j[p], the 12 entries of T[p] are finite and its weights - d_w[p] = (w_rot, w_trans), or the host pair when d_w == NULL - are
 * finite and >= 0; a logged slot stores (d_i[p], d_j[p]), T[p] and its weights at row `edges`, in the order of p.  Overflow, the
 * clamping of a scribbled state[0], info = {logged by this call, first row or -1, edges after, flags} and PR_POSEGRAPH_OVERFLOW are
 * pr_posegraph_add_dev's: the call leaves the bytes that c calls of pr_posegraphw_add_dev (k = 1) with query_row = d_j[p] leave (so state is
 * rewritten only if some d_j[p] >= 0).  One workgroup, ascending chunks with an integer scan; capturable; the device form allocates
 * nothing.  The host form stages c slots in an allocation of its own for the call and synchronises.  PR_EINVAL: c outside 1 .. 65535,
 * a negative or non-finite w_rot / w_trans, a NULL handle or required pointer. */
int pr_posegraphb_add_dev(pr_posegraph* g, const int32_t* d_i, const int32_t* d_j, const double* d_T, const uint8_t* d_accepted,
                          const double* d_w, double w_rot, double w_trans, int32_t c, int32_t* d_info);
int pr_posegraphb_add(pr_posegraph* g, const int32_t* i, const int32_t* j, const double* T, const uint8_t* accepted, const double* w, double w_rot,
                      double w_trans, int32_t c, int32_t* info);

/* ---- local submaps: several keyframes gathered into one cloud for ICP (submap.hip) -----------------------------------------
 * Every registration between keyframes takes one keyframe cloud per side, and SO-DSO's clouds are sparse.  A pr_submap gathers, for every
 * slot of a pair list, the clouds of the map rows centre - w .. centre + w into ONE cloud in the centre row's camera frame, with the poses
 * the map holds (or relaxed ones).  The output is a CSR set pr_icp_pairs_dev reads as it stands (slot p is cloud p); both sides of a pair
 * are expressed in their centre frames, so the seed T0 = P_i P_q^-1 of a pr_proximity search and the meaning of T (query camera to DB
 * camera) do not change.  One device; no voxel de-duplication (points that several rows hold are kept); the poses are taken as given.
 *
 *   pr_submap_create      slot_capacity 1 .. 65535 (pr_icp_pairs_dev's slot limit), w_max 0 .. 31, point_capacity 1 .. 2^40 (rows of out_xyz),
 *                         max_cloud_points 1 .. 2^26 and keyframe_capacity 1 .. 2^24 (the map's).  ONE allocation; no later call of the device
 *                         form allocates: with S = slot_capacity and L = 2 w_max + 1 the entry lists 4 S L (rows) + 4 S L (starts inside the
 *                         slot) + 4 S L (lengths) + 8 S L (source starts), per slot 4 S (total) + 4 S (flags) + 4 S (rows taken) + 8 S (base),
 *                         each part rounded up to 16.  pr_submap_scratch_bytes returns the sum (0 for sizes create refuses).
 *   pr_submap_build_dev   3 launches (plan, scan, gather) on the context's stream.  map: xyz and offs are read (pr_map_buffers of the resident
 *                         map); d_poses [>= n][12] f64 world to camera, row-major [R | t]: the map's own or a relaxed array; d_n i32 [>= 1]
 *                         (pr_map_buffers.state); d_center i32 [c] (NULL with c = 0 is fine); d_avoid i32 [c] or NULL.  CALLER-OWNED outputs: out_xyz [point_capacity][3]
 *                         f64, out_offs [slot_capacity + 1] i64, out_rows [slot_capacity][2] i32 = {rows taken, flags}, d_info [4] i32 =
 *                         {slots non-empty, points written as two words (low, high), flags OR-ed}.  Every grid depends on the create sizes
 *                         only and d_n is read on the device: one capture made at n = 0 serves every count.  No read-back, no floating-point
 *                         atomics; two runs give the same bytes.
 *   pr_submap_build       the same with HOST center / avoid and HOST outputs (map, d_poses and d_n stay device memory); stages in an
 *                         allocation of its own for the call and synchronises.
 *
 * The rule (restated in fp64 in tests/submap_np.py; the device equals it byte for byte).
 *  0. n = d_n[0] clamped into 0 .. keyframe_capacity before any address is formed.  Slot p < c has centre = d_center[p].
 *  1. The walk of slot p: r_0 = centre, then centre - 1, centre + 1, centre - 2, centre + 2, ... up to distance w = half_window (64-bit
 *     row numbers).  With past_only != 0 only rows <= centre are walked.
 *  2. Row r is ELIGIBLE iff 0 <= r < n; all 12 entries of poses[r] are finite; d_avoid is NULL or |r - avoid[p]| > avoid_gap (64-bit
 *     integers: the difference cannot wrap; the centre is exempt); and offs[r] >= 0 with len_r = offs[r + 1] - offs[r] in
 *     0 .. max_cloud_points.  A length outside that range counts as not eligible, and no address is formed from it.  An ineligible row is
 *     skipped and the walk goes on.
 *  3. An eligible row whose points would take the slot above max_pts is not taken, sets PR_SUBMAP_TRUNCATED on the slot, and ends the
 *     walk: a submap never holds part of a cloud.  `rows taken` counts the eligible rows in front of that one (empty clouds included).
 *  4. centre < 0 switches the slot off: it is empty and no flag is set.  centre >= n, or a centre whose pose is not finite: the slot is
 *     empty with PR_SUBMAP_NO_CENTER.  A centre that fails only the length test is skipped like any other row.
 *  5. Placement: the slots' lengths are scanned exclusively in slot order.  A slot whose end would pass point_capacity becomes empty
 *     (rows taken = 0) with PR_SUBMAP_OVERFLOW, and later slots are placed behind the last one that fits: a slot is never partial.
 *     out_offs[0 .. c] is always written, entries c + 1 .. slot_capacity are set to out_offs[c]; out_rows[p] = {0, 0} for p >= c.
 *     Rows of out_xyz at or behind out_offs[c] are not written.  `slots non-empty` counts the slots with rows taken > 0.
 *  6. Rows are written in walk order, and points in row order.  The centre row's points are copied bit for bit.  A point x of row
 *     r != centre becomes y = R_c (R_r^T (x - t_r)) + t_c, in exactly this order: d = x - t_r; u_k = (R_r[0][k] d_0 + R_r[1][k] d_1) +
 *     R_r[2][k] d_2; v_k = (R_c[k][0] u_0 + R_c[k][1] u_1) + R_c[k][2] u_2; y_k = v_k + t_c[k]; every operation rounded, no contraction.
 *     A non-finite point goes through the same arithmetic and is written as it comes out (the ICP stage leaves it out).
 * PR_EINVAL (text: pr_last_error) before any device is touched: a NULL handle, map record, params or required pointer, sizes outside the
 * limits above, c outside 0 .. slot_capacity, half_window outside 0 .. w_max, max_pts < 1, avoid_gap < 0.  c = 0 is a valid empty call
 * that still writes out_offs and d_info. */
typedef struct pr_submap pr_submap;
typedef struct pr_submap_params { int32_t half_window, past_only, avoid_gap, max_pts; } pr_submap_params;
enum { PR_SUBMAP_TRUNCATED = 1, PR_SUBMAP_NO_CENTER = 2, PR_SUBMAP_OVERFLOW = 4 };
int pr_submap_create(pr_ctx* ctx, int32_t slot_capacity, int32_t w_max, int64_t point_capacity, int32_t max_cloud_points, int32_t keyframe_capacity,
                     pr_submap** out);
void pr_submap_destroy(pr_submap* sm);
int64_t pr_submap_scratch_bytes(int32_t slot_capacity, int32_t w_max);
int pr_submap_build_dev(pr_submap* sm, const pr_map_buffers* map, const double* d_poses, const int32_t* d_n, const int32_t* d_center,
                        const int32_t* d_avoid, int32_t c, const pr_submap_params* params, double* out_xyz, int64_t* out_offs, int32_t* out_rows,
                        int32_t* d_info);
int pr_submap_build(pr_submap* sm, const pr_map_buffers* map, const double* d_poses, const int32_t* d_n, const int32_t* center, const int32_t* avoid,
                    int32_t c, const pr_submap_params* params, double* out_xyz, int64_t* out_offs, int32_t* out_rows, int32_t* info);

/* ---- drive sessions: join a later drive to the map through its closures (session.hip) ------------------------------------
 * The reference evaluates place recognition over one drive that revisits itself and over two drives of one route (test_robotcar.m).  A
 * second drive can be appended behind the first in a pr_map and its closures logged in a pr_posegraph, but its poses start at the identity
 * of a world frame of their own.  A pr_session records where each drive begins in the map's rows, moves a later drive rigidly onto the
 * earlier ones by a consensus of the cross-drive closures, and relaxes the joined rows without the odometry edges across drive borders.
 * After an align every stage that takes one pose array in one frame (pr_gate, pr_worldmap, pr_maploc, pr_proximity, pr_trajeval) works on
 * the joined array as it stands.  Everything is stream-ordered, reads every count on the device, reads nothing back and allocates nothing
 * after create; every grid is a function of the create sizes only, so one capture made with an empty log and one session serves every
 * count.  The intended chain is align -> pr_gate_run_dev -> pr_session_relax_dev, captured once and replayed.
 *
 *   pr_session_create   binds the CALLER-OWNED device buffers (pr_session_buffers; they must outlive the handle): start [session_capacity]
 *                       i32, the first row of every session, and state [4] i32 = {sessions S, flags, 0, 0}; sets S = 1, start[0] = 0.
 *                       session_capacity in 1 .. 1024, node_capacity in 1 .. 2^20, edge_capacity in 1 .. 65536 (the gate's limit: the
 *                       alignment visits all pairs).  ONE allocation; with NC = node_capacity and EC = edge_capacity the parts are, each
 *                       rounded up to 16 bytes:
 *                         4 NC (sid) | 4 NC (breaks) | 4 EC (candidate) | 4 EC (q) | 96 EC (G_a) | 24 EC (c_a) | 24 EC (G_a c_a) |
 *                         4 EC (support sums) | 4 EC (members of I) | 192 (G, G^-1) | 48 (control)
 *                         | staging of the host forms: 96 (G) | 96 EC (hyp) | 4 EC (support) | EC (inlier) | 32 (info) | 16 (begin's info)
 *                       pr_session_scratch_bytes returns the sum (0 for sizes create refuses).
 *   pr_session_reset    S = 1, start[0] = 0, flags = 0 (stream-ordered).   pr_session_count   synchronising read of S and flags (diagnostics).
 *   pr_session_begin_dev  one launch of one thread.  d_n [>= 1] i32: pass the map's state, word 0 is the keyframe count; d_info [4] i32.
 *   pr_session_begin    the same with a HOST info (d_n stays device memory); synchronises.
 *   pr_session_align_dev  4 launches (prepare, pairs, choose, apply).  log: the buffer record of a closure log with log_edge_capacity rows,
 *                       1 <= log_edge_capacity <= edge_capacity; it is only read.  d_poses_in, d_poses_out [node_capacity][12] f64 (they
 *                       may be equal), d_n as for begin, d_G [12] f64, d_hyp [edge_capacity][12] f64 or NULL, d_support [edge_capacity] i32
 *                       or NULL, d_inlier [edge_capacity] u8 or NULL, d_info [8] i32.  Every entry of an output that is given is written.
 *   pr_session_align    the same with HOST G, hyp, support, inlier, info (the log, the poses and d_n stay device memory); synchronises.
 *   pr_session_relax_dev  1 launch (sid and breaks of every row from the table as it stands) and then pr_posegraph_relax_dev's 3 outer + 3
 *                       launches on the graph g, whose prepare step reads the break array: 3 outer + 4 launches in all.  g must live on the
 *                       session table's context and have its node_capacity.  Arguments, report and refusals are pr_posegraph_relax_dev's.
 *
 * The table.  S = state[0] clamped into 1 .. session_capacity before use.  Row r belongs to session
 *      sid(r) = #{q in 1 .. S-1 : start[q] <= r}
 * - a count, not a search: it is defined for any scribbled start, and start[0] is never read (session 0 begins at row 0).  Row r >= 1 is
 * a BREAK iff sid(r) != sid(r-1).
 * begin, decided on the device: n = d_n[0] clamped into 0 .. node_capacity; last = start[S-1] (0 when S == 1).  If n == last the current
 * last session is still empty: nothing is stored and info[3] carries PR_SESSION_REUSED.  Else if S == session_capacity nothing is stored
 * and PR_SESSION_OVERFLOW is set, in state[1] and in every later info, until pr_session_reset.  Else start[S] = n and S + 1 is committed
 * by one thread.  info = {session index now current, its first row, S after, flags}.
 *
 * The alignment (restated in tests/session_np.py).  Conventions as for pr_posegraph and pr_gate: a pose is [R | t], 12 doubles row-major,
 * world to camera; a closure (i, j, Z) measures Z ~ P_i P_j^-1; A B = [R_A R_B | R_A t_B + t_A]; A^-1 = [R^T | -(R^T t)]; fp64, no
 * contraction; a 3 x 3 product entry is (a0 b0 + a1 b1) + a2 b2; the translation of a product is ((r0 t0 + r1 t1) + r2 t2) + t_A, of an
 * inverse -((R0r t0 + R1r t1) + R2r t2); R^T is formed first and then multiplied like any other matrix.
 *   1. Counts.  E = log.state[0] clamped into 0 .. log_edge_capacity, n = d_n[0] clamped into 0 .. node_capacity, S as above, all before
 *      any address is formed from them.  The target is t = params.session, and -1 means S - 1.  If t <= 0, t >= S or session t has no row
 *      < n the status is PR_SESSION_NO_TARGET: rows < n are copied bit for bit and G is the identity.
 *   2. Candidates.  Edge a < E is a candidate iff it is valid by the relaxation's skip rule (0 <= i, j < n, i != j, its 12 Z entries and
 *      2 weights finite, the 24 entries of P_i, P_j finite) and exactly one end lies in session t and the other in a session < t: the
 *      earlier sessions are the anchor, edges to later sessions are ignored.
 *   3. Hypotheses.  With j in t: G_a = (P_i^-1 Z_a) P_j (the gate's M_a).  With i in t: G_a = (P_j^-1 Z_a^-1) P_i.  G_a maps session t's
 *      world frame into the anchor's.  q_a is the edge's row in t, c_a = -(R^T t) of P_qa that row's camera centre (the translation of
 *      P_qa^-1), and G_a c_a = ((r0 c0 + r1 c1) + r2 c2) + t_Ga.
 *   4. Support, over ordered pairs.  b supports a iff both are candidates, a != b, q_a != q_b (two candidates of one keyframe are not
 *      independent evidence), c_rot = 3 - ((x00 + x11) + x22) <= rot_c_max with x_cc = (Ra_0c Rb_0c + Ra_1c Rb_1c) + Ra_2c Rb_2c the
 *      diagonal of R_Ga^T R_Gb, and c_trans = (dx dx + dy dy) + dz dz <= trans2_max with d = G_a c_b - G_b c_b: the two hypotheses are
 *      compared AT THE CLOSURE, not at the world origin, so a small rotation difference is not multiplied by the route's lever arm.
 *      + and x only.  A NaN supports nothing.  The rule is evaluated as written; it need not be symmetric in floating point.
 *   5. Choice.  a* is the candidate with the largest support, ties to the lowest log index: a decision in integers.  No candidate:
 *      PR_SESSION_NO_CANDIDATE.  support + 1 < min_inliers: PR_SESSION_WEAK.  Both copy the poses and return the identity.
 *   6. Refinement over I = {a*} and its supporters, in log order, the sums by the fixed tree of the library's block sums:
 *      R = R_Ga* exp(mean_b log_SO3(R_Ga*^T R_Gb)) with pr_posegraph's log_SO3 and exp and their ONE small-angle branch at 1e-4;
 *      t = mean_b(G_b c_b) - R mean_b(c_b).  A non-finite G: PR_SESSION_NONFINITE, and the poses are copied.
 *   7. Apply.  Every finite row of session t becomes P_r G^-1; every other row < n is copied bit for bit; rows >= n are not written.
 *   8. Outputs.  d_G is G, or the identity unless the status is PR_SESSION_ALIGNED.  d_hyp holds G_a of every candidate and zeros
 *      elsewhere; d_support is -1 for a non-candidate; d_inlier marks the members of I (all 0 without an a*; with PR_SESSION_WEAK the
 *      members are still marked).  info = {status, a* or -1, its support, candidates, |I|, E, n, flags}: flags carries
 *      PR_SESSION_OVERFLOW of the table and PR_SESSION_LOG_OVERFLOW when the log's state[1] has PR_POSEGRAPH_OVERFLOW.
 * Everything up to the choice, d_hyp and every copied row equal the restatement bit for bit; G and the moved rows differ from it by the
 * rounding of the sums' order and of sin, cos, atan2 only (DESIGN.md 4.29 has the measured bound).  Two runs give the same bytes.
 *
 * The relaxation across breaks is pr_posegraph_relax_dev's rule with one change: odometry slot s is not an edge when row s + 1 is a break.
 * With S == 1 it leaves exactly pr_posegraph_relax_dev's bytes.  A session without a used closure to the rest does not move: its
 * odometry residuals are exactly zero, so its gradient is zero and the conjugate gradients start from 0.  Node 0 remains the only gauge.
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, record, buffer, params or required pointer, a capacity
 * out of range, log_edge_capacity outside 1 .. edge_capacity, session < -1, min_inliers < 1, a rot_c_max or trans2_max that is NaN or
 * negative (+Inf is allowed and switches that test off), a graph on another context or with another node_capacity, and everything
 * pr_posegraph_relax_dev refuses. */
typedef struct pr_session pr_session;
typedef struct pr_session_buffers { int32_t* start; int32_t* state; } pr_session_buffers;
typedef struct pr_session_align_params { int32_t session, min_inliers; double rot_c_max, trans2_max; } pr_session_align_params;
#define PR_SESSION_OVERFLOW 1
#define PR_SESSION_REUSED 2
#define PR_SESSION_LOG_OVERFLOW 4
enum { PR_SESSION_ALIGNED = 0, PR_SESSION_NO_TARGET = 1, PR_SESSION_NO_CANDIDATE = 2, PR_SESSION_WEAK = 3, PR_SESSION_NONFINITE = 4 };
int pr_session_create(pr_ctx* ctx, const pr_session_buffers* buffers, int32_t node_capacity, int32_t edge_capacity, int32_t session_capacity,
                      pr_session** out);
void pr_session_destroy(pr_session* s);
int pr_session_reset(pr_session* s);
int pr_session_count(pr_session* s, int32_t* sessions, int32_t* flags);
size_t pr_session_scratch_bytes(int32_t node_capacity, int32_t edge_capacity, int32_t session_capacity);
int pr_session_begin_dev(pr_session* s, const int32_t* d_n, int32_t* d_info);
int pr_session_begin(pr_session* s, const int32_t* d_n, int32_t* info);
int pr_session_align_dev(pr_session* s, const pr_posegraph_buffers* log, int32_t log_edge_capacity, const double* d_poses_in, const int32_t* d_n,
                         const pr_session_align_params* params, double* d_poses_out, double* d_G, double* d_hyp, int32_t* d_support,
                         uint8_t* d_inlier, int32_t* d_info);
int pr_session_align(pr_session* s, const pr_posegraph_buffers* log, int32_t log_edge_capacity, const double* d_poses_in, const int32_t* d_n,
                     const pr_session_align_params* params, double* d_poses_out, double* G, double* hyp, int32_t* support, uint8_t* inlier,
                     int32_t* info);
int pr_session_relax_dev(pr_session* s, pr_posegraph* g, const double* d_poses_in, const int32_t* d_n, const pr_posegraph_params* params,
                         double* d_poses_out, double* d_report);

/* ---- snapshots: the resident map, databases, closure logs and session table saved and restored (snapshot.hip) -----------
 * All resident state lives in caller-owned device buffers that die with the process.  A pr_snapshot packs the live rows of those buffers
 * into ONE self-describing blob on the device, validates such a blob and unpacks it into buffers of the same or LARGER capacities, also on
 * the device, and has host forms that write and read a file, so a map built by one process is continued by another.  Counts are read on
 * the device, a scribbled count never forms an address, a blob that does not fit or does not check out changes no byte, and a restored
 * state continues a drive to the same bytes as an uninterrupted run.
 * OUT OF SCOPE: the pre-stage point window (pr_window), the sequence filter's ring (pr_seqmatch), the world map with its index and normals
 * (pr_worldmap, pr_maploc, pr_mapplane, pr_mapgrow) and all scratch.  A later drive starts the window and the ring afresh; the world map,
 * index and normals are rebuilt by one fuse -> index -> normals from the restored map.
 *
 * The parts.  Each is optional; a desc names the buffer records of the parts it covers and the capacities they were created with.
 *   kind                   sections (array: bytes per row; rows)                                          count, clamped
 *   PR_SNAPSHOT_MAP        xyz 24, inten 4: points | offs 8: keyframes + 1 | frames 128, poses 96, ids 4: keyframes
 *                                                                          keyframes = state[0] in 0 .. keyframe_capacity,
 *                                                                          points = offs[keyframes] in 0 .. point_capacity
 *   PR_SNAPSHOT_ONLINE     sig 19200 (PR_TYPE_SC) or 12288 (PR_TYPE_M2DP)  state[0] in 0 .. capacity;  subtype = the type; up to two
 *   PR_SNAPSHOT_ONLINESET  fused: sc 19200, m2dp 12288; DELIGHT: delight 32768   state[0] in 0 .. capacity;  subtype = the kind
 *   PR_SNAPSHOT_GRAPH      edge_ij 8, edge_Z 96, edge_w 16                  state[0] in 0 .. edge_capacity;  subtype = 0 (the raw log), 1 (a gated one)
 *   PR_SNAPSHOT_SESSION    start 4                                          state[0] in 1 .. session_capacity
 * Sections come in this order (map, online[0], online[1], online set, graph[0], graph[1], sessions; the arrays of a part in the order
 * above): at most 17.
 *
 * The blob, little-endian, every value as its raw bytes.  With NS sections:
 *   header   8 x i64 = 64 bytes: magic "PRASNAP1", version 1, NS, total bytes, 64 + 128 NS, the table's checksum, 0, 0
 *   table    NS entries of 16 x i64 = 128 bytes: kind, subtype, array, rows, bytes per row, byte offset, byte length, checksum, the part's
 *            four state words verbatim (2 x i64; sticky flags included), the capacities the part was saved from (4 x i64: map
 *            keyframe_capacity, point_capacity, max_cloud_points, 0; else the capacity, 0, 0, 0), the part's index, 0
 *   sections the live rows of every section, compacted: byte length = rows x bytes per row, each section on a 64-byte boundary, the pad
 *            behind it zero; total bytes = the end of the last pad
 *   pr_snapshot_bound = 64 + 128 NS + sum over the sections of pad64(capacity rows x bytes per row), pad64(b) = (b + 63) & ~63, with
 *            capacity rows = point_capacity (xyz, inten), keyframe_capacity + 1 (offs), else the part's capacity.
 * The checksum of a section is the wrap-around uint64 sum over its 8-byte words w_i, i = 0, 1, ..., of mix(w_i, i); a 4-byte tail is
 * zero-extended.  mix(w, i): x = w ^ ((i + 1) * 0x9E3779B97F4A7C15); x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 * x *= 0x94D049BB133111EB; x ^= x >> 31 (all mod 2^64).  For every i it is a bijection of w, so a changed word changes its term: every
 * single-bit flip is caught.  The table's checksum is the same sum over its 16 NS words.  The sum does not depend on the order of its
 * terms: workgroup sums are combined by 64-bit integer atomic adds.  No floating-point operation anywhere.
 *
 *   pr_snapshot_create    the desc's records and capacities are copied (the buffers must outlive the handle; it never owns them).  ONE
 *                         allocation: the control words, the per-section checksum partials and the info of the host forms.  No later
 *                         call of a device form allocates.  Bound to ctx and its stream; destroy before ctx.
 *   pr_snapshot_bound     the largest blob these capacities can produce.  pr_snapshot_desc_bound: the same from a desc, without a handle.
 *   pr_snapshot_pack_dev  stream-ordered, capturable, no read-back: 3 launches (plan, copy, finish) whose geometry is fixed by the create
 *                         capacities.  d_blob DEVICE [blob_capacity] bytes on a 16-byte boundary; d_info DEVICE [4] i64.  Every count is
 *                         clamped into its capacity before an address is formed from it.  info = {bytes written, sections, flags, 0}.
 *                         If the blob would not fit, PR_SNAPSHOT_OVERFLOW is set, the header and table (checksums 0) are written when
 *                         THEY fit and nothing past the header's extent 64 + 128 NS is written; bytes written is then the size that
 *                         would have been needed.  The data is read ONCE: the copy's lanes mix the words they move.
 *   pr_snapshot_unpack_dev  stream-ordered, capturable: 4 launches (header, sum, verify, scatter).  d_blob DEVICE [blob_bytes] on a
 *                         16-byte boundary.  VALIDATE, decided on the device; a failed check sets its flag and names its section:
 *                           PR_SNAPSHOT_TRUNCATED    blob_bytes < 64, NS outside 0 .. 17, the table or a section not inside blob_bytes, an
 *                                                    offset that is not a multiple of 64 or lies before the previous section's end, a length
 *                                                    that is not rows x bytes per row, sections of one part that disagree on its count
 *                           PR_SNAPSHOT_BAD_MAGIC / PR_SNAPSHOT_BAD_VERSION   nothing else of the blob is read then
 *                           PR_SNAPSHOT_MISSING      entry s is not the handle's section s (kind, subtype, array, bytes per row), or the blob
 *                                                    has another number of sections (named: the smaller of the two numbers)
 *                           PR_SNAPSHOT_CAPACITY     rows outside 0 .. the DESTINATION's capacity rows; a cloud of the map above the
 *                                                    destination's max_cloud_points
 *                           PR_SNAPSHOT_CHECKSUM     a section's checksum, or the table's own (which names no section)
 *                           PR_SNAPSHOT_OFFSETS      the map's offs: offs[0] != 0, descending at a row, offs[keyframes] != the rows of xyz
 *                           PR_SNAPSHOT_SESSIONS     start[0] != 0 or start not strictly ascending: not an order pr_session_begin_dev
 *                                                    produces over a growing map
 *                         Only extents that passed form an address.  SCATTER is switched off on the device by any failed check; else it
 *                         copies the saved rows into the destination buffers and writes each part's four state words as saved.  Rows at
 *                         or above the saved count are left exactly as the destination held them: restore into freshly created or reset
 *                         buffers.  info = {sections restored (NS or 0), first failing section or -1, flags, 0}.  On any failure NO BYTE
 *                         of any destination buffer changes.
 *   pr_snapshot_save      the host form: packs into a staging blob of pr_snapshot_bound bytes, ONE synchronising read of info, ONE
 *                         device-to-host copy of exactly `bytes written`, written to path + ".tmp" and renamed to path.
 *   pr_snapshot_load      the host form: reads the file and refuses on the host, no device touched: a missing or unreadable file
 *                         (PR_EIO), a file shorter than a header, a header cut inside its table, a table entry that points outside the
 *                         file (PR_EINVAL).  Then uploads, runs pr_snapshot_unpack_dev and synchronises; info HOST [4] i64 as above.
 *                         The two host forms take and free their staging themselves and are not capturable.
 * Two runs give the same bytes.  Nothing is written outside the blob's reported extent or the destination buffers' stated extents.
 * PR_EINVAL (text: pr_last_error) before any device is touched for a NULL handle, desc, blob, info or path, a blob off a 16-byte boundary,
 * a negative size, a desc with no part, a NULL buffer of a named part, a non-positive or too large capacity, max_cloud_points >
 * point_capacity, an online type or set kind the library does not know, a set's buffers that do not fit its kind. */
typedef struct pr_snapshot pr_snapshot;
typedef struct pr_snapshot_desc {
  const pr_map_buffers* map; int32_t keyframe_capacity, max_cloud_points; int64_t point_capacity;
  const pr_online_buffers* online[2]; int32_t online_type[2]; int32_t online_capacity[2];
  const pr_onlineset_buffers* onlineset; int32_t onlineset_kind, onlineset_capacity;
  const pr_posegraph_buffers* graph[2]; int32_t edge_capacity[2];
  const pr_session_buffers* sessions; int32_t session_capacity, reserved;
} pr_snapshot_desc;
enum { PR_SNAPSHOT_MAP = 1, PR_SNAPSHOT_ONLINE = 2, PR_SNAPSHOT_ONLINESET = 3, PR_SNAPSHOT_GRAPH = 4, PR_SNAPSHOT_SESSION = 5 };
enum { PR_SNAPSHOT_OVERFLOW = 1, PR_SNAPSHOT_BAD_MAGIC = 2, PR_SNAPSHOT_BAD_VERSION = 4, PR_SNAPSHOT_TRUNCATED = 8, PR_SNAPSHOT_MISSING = 16,
       PR_SNAPSHOT_CAPACITY = 32, PR_SNAPSHOT_CHECKSUM = 64, PR_SNAPSHOT_OFFSETS = 128, PR_SNAPSHOT_SESSIONS = 256 };
int pr_snapshot_create(pr_ctx* ctx, const pr_snapshot_desc* desc, pr_snapshot** out);
void pr_snapshot_destroy(pr_snapshot* s);
int pr_snapshot_bound(pr_snapshot* s, int64_t* bytes);
int pr_snapshot_desc_bound(const pr_snapshot_desc* desc, int64_t* bytes);
int pr_snapshot_pack_dev(pr_snapshot* s, void* d_blob, int64_t blob_capacity, int64_t* d_info);
int pr_snapshot_unpack_dev(pr_snapshot* s, const void* d_blob, int64_t blob_bytes, int64_t* d_info);
int pr_snapshot_save(pr_snapshot* s, const char* path);
int pr_snapshot_load(pr_snapshot* s, const char* path, int64_t* info);

#ifdef __cplusplus
}
#endif
#endif /* PLACE_RECOGNITION_H */
