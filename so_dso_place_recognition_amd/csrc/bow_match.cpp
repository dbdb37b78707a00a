// bow_match.cpp — host side of the inverted-file BoW matcher (bow_match.hip): the device-resident database (main segment + a tail
// segment for online growth, folded into the main lists when full), the stream-ordered top-k and the two host forms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "resident_match.hpp"

typedef unsigned long long u64;

struct pr_bow_db {
  int device = -1;
  int32_t max_sigs = 0, cols = 0, n_words = 0;
  int64_t max_postings = 0;
  int32_t main_rows = 0, tail_rows = 0;          // rows [0, main_rows) are in the main lists, [main_rows, main_rows + tail_rows) in the tail's
  int64_t main_post = 0, tail_post = 0;
  int32_t tail_cap = 0, chunk = 0, threads = 256;     // tail_cap 0: a fixed DB (the host forms' temporary one), no tail, no fold buffers
  int64_t tail_post_cap = 0;
  u64 *moff = nullptr, *moff2 = nullptr, *toff = nullptr;   // [n_words + 1] offsets: main, main being folded into, tail
  int *mrow = nullptr, *mrow2 = nullptr, *trow = nullptr;  // postings: local row
  double *mw = nullptr, *mw2 = nullptr, *tw = nullptr;     // postings: weight
  double* traw = nullptr;                                  // [2 tail_cap][cols] the tail's rows (its lists are rebuilt from them)
  double* acc = nullptr;                                   // [chunk][max_sigs] fp64 accumulators of one match chunk
  int* counts = nullptr;                                   // [n_words] per-word counts of a build
  u64* cursor = nullptr;                                   // [n_words + 1] scatter cursor
  u64* tsum = nullptr;                                     // scan tile sums
  u64* stat = nullptr;                                     // [2]: [0] postings counted, [1] (int) first non-conforming row
};

namespace {

using pr::fail;

constexpr size_t SCRATCH_BYTES = (size_t)512 << 20;   // accumulators of one chunk
constexpr int MAX_WORDS = 1 << 26;                   // vocabulary size limit (64-bit offsets: 512 MB per offset array)

int env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}

template <typename T>
hipError_t dalloc(T*& p, size_t count) { return hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)); }

void release(pr_bow_db* db) {
  void* ps[] = {db->moff, db->moff2, db->toff, db->mrow, db->mrow2, db->trow, db->mw, db->mw2, db->tw, db->traw, db->acc, db->counts,
                db->cursor, db->tsum, db->stat};
  for (void* p : ps) if (p) (void)hipFree(p);
  delete db;
}

// the readable length of a row and whether it conforms (the kernels' rule, on the host)
int host_row_length(const double* ids, int cols) {
  int p = 0;
  while (p < cols - 1 && ids[p] > -1.0) p++;
  return p;
}
bool host_row_ok(const double* ids, int cols, int n_words) {
  const int L = host_row_length(ids, cols);
  for (int p = 0; p < L; p++) {
    const double x = ids[p];
    if (!(x == std::rint(x) && x < (double)n_words && (p == 0 || x > ids[p - 1]))) return false;
  }
  return true;
}

struct DevTmp {
  void* p = nullptr;
  ~DevTmp() { if (p) (void)hipFree(p); }
};

// validate (+ count into db->counts when `counts`) rows [2 n][cols] on the device; -> postings, first bad row (INT_MAX: none). Synchronises.
int check_rows(pr_ctx* ctx, pr_bow_db* db, const double* drows, int n, int row_name0, bool counts, int64_t* posts, int* bad) {
  hipStream_t st = pr::ctx_stream(ctx);
  const int none = INT_MAX;
  if (counts) PR_CHECK_HIP(ctx, hipMemsetAsync(db->counts, 0, (size_t)db->n_words * sizeof(int), st));
  PR_CHECK_HIP(ctx, hipMemsetAsync(db->stat, 0, sizeof(u64), st));
  PR_CHECK_HIP(ctx, hipMemcpyAsync(db->stat + 1, &none, sizeof(int), hipMemcpyHostToDevice, st));
  pr::launch_bow_rows_check(st, drows, n, db->cols, db->n_words, row_name0, counts ? db->counts : nullptr, db->stat,
                            reinterpret_cast<int*>(db->stat + 1));
  PR_CHECK_HIP(ctx, hipGetLastError());
  u64 h[2];
  PR_CHECK_HIP(ctx, hipMemcpyAsync(h, db->stat, sizeof h, hipMemcpyDeviceToHost, st));
  PR_CHECK_HIP(ctx, hipStreamSynchronize(st));
  *posts = (int64_t)h[0];
  int b;
  memcpy(&b, &h[1], sizeof b);
  *bad = b;
  return PR_OK;
}

// lists of rows [2 n][cols] (already validated and counted into db->counts) into (off, prow, pw), rows numbered from j0
int scatter_rows(pr_ctx* ctx, pr_bow_db* db, const double* drows, int n, int j0, u64* off, int* prow, double* pw) {
  hipStream_t st = pr::ctx_stream(ctx);
  pr::launch_bow_scan(st, db->counts, db->n_words, db->tsum, off, db->cursor);
  pr::launch_bow_scatter(st, drows, n, db->cols, j0, db->cursor, prow, pw);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int bad_row_error(pr_ctx* ctx, const char* fn, int row, int n_words) {
  return fail(ctx, PR_EINVAL, "%s: BoW row %d is not conforming (before its terminator every word id must be an integer in [0, %d), strictly "
              "ascending)", fn, row, n_words);
}

// the tail's lists from its rows [0, tail_rows)
int rebuild_tail(pr_ctx* ctx, pr_bow_db* db) {
  int64_t posts = 0;
  int bad = INT_MAX;
  if (int rc = check_rows(ctx, db, db->traw, db->tail_rows, 0, true, &posts, &bad)) return rc;
  if (bad != INT_MAX || posts > db->tail_post_cap) return fail(ctx, PR_EHIP, "pr_bow_db_append: tail rebuild failed (internal)");
  if (int rc = scatter_rows(ctx, db, db->traw, db->tail_rows, db->main_rows, db->toff, db->trow, db->tw)) return rc;
  db->tail_post = posts;
  return PR_OK;
}

int fold(pr_ctx* ctx, pr_bow_db* db) {
  hipStream_t st = pr::ctx_stream(ctx);
  if (db->tail_rows == 0) return PR_OK;
  pr::launch_bow_fold(st, db->n_words, db->moff, db->mrow, db->mw, db->toff, db->trow, db->tw, db->moff2, db->mrow2, db->mw2);
  PR_CHECK_HIP(ctx, hipGetLastError());
  std::swap(db->moff, db->moff2);
  std::swap(db->mrow, db->mrow2);
  std::swap(db->mw, db->mw2);
  db->main_rows += db->tail_rows;
  db->main_post += db->tail_post;
  db->tail_rows = 0;
  db->tail_post = 0;
  PR_CHECK_HIP(ctx, hipMemsetAsync(db->toff, 0, ((size_t)db->n_words + 1) * sizeof(u64), st));
  return PR_OK;
}

int launch_match(pr_ctx* ctx, const pr_bow_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0, int32_t mask_width, int32_t k,
                 int32_t* idx, double* score) {
  hipStream_t st = pr::ctx_stream(ctx);
  const int n = db->main_rows + db->tail_rows;
  for (int32_t c0 = 0; c0 < m; c0 += db->chunk) {
    const int mc = std::min(db->chunk, m - c0);
    pr::launch_bow_score(st, db->threads, q + (size_t)2 * c0 * db->cols, mc, db->cols, db->n_words, q_row0 + c0, db->moff, db->mrow, db->mw,
                         db->toff, db->trow, db->tw, n, db_row0, mask_width, k, db->acc, idx + (size_t)c0 * k, score + (size_t)c0 * k,
                         pr::ctx_bow_rows_flag(ctx));
  }
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

// vocabulary size implied by host rows (largest readable integer id + 1, ids beyond MAX_WORDS left to the conformance check), and postings
void host_scan(const double* h, int32_t n, int32_t cols, int* n_words, int64_t* posts) {
  for (int32_t r = 0; r < n; r++) {
    const double* ids = h + (size_t)2 * r * cols;
    const int L = host_row_length(ids, cols);
    if (posts) *posts += L;
    for (int p = 0; p < L; p++)
      if (ids[p] >= 0 && ids[p] < MAX_WORDS && ids[p] == std::rint(ids[p])) *n_words = std::max(*n_words, (int)ids[p] + 1);
  }
}

int create_db(pr_ctx* ctx, int32_t max_sigs, int32_t cols, int32_t n_words, int64_t max_postings, int max_chunk, bool growable,
              pr_bow_db** out);
int set_rows(pr_ctx* ctx, const char* fn, pr_bow_db* db, const double* rows, int where, int32_t n);

// a temporary database over host rows h2 (the host forms)
int host_db(pr_ctx* ctx, const char* fn, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, int chunk, pr_bow_db** out) {
  int n_words = 1;
  int64_t posts = 0;
  host_scan(h1, m, cols, &n_words, nullptr);
  host_scan(h2, n, cols, &n_words, &posts);
  for (int32_t i = 0; i < m; i++)
    if (!host_row_ok(h1 + (size_t)2 * i * cols, cols, n_words)) return fail(ctx, PR_EINVAL, "%s: query row %d is not conforming", fn, i);
  if (int rc = create_db(ctx, std::max(n, 1), cols, n_words, std::max<int64_t>(posts, 1), chunk, false, out)) return rc;
  if (int rc = set_rows(ctx, fn, *out, h2, PR_HOST, n)) {
    pr_bow_db_destroy(ctx, *out);
    *out = nullptr;
    return rc;
  }
  return PR_OK;
}

// max_chunk: queries per match chunk at most (the host forms: their m, so the scratch is no larger than the call)
int create_db(pr_ctx* ctx, int32_t max_sigs, int32_t cols, int32_t n_words, int64_t max_postings, int max_chunk, bool growable,
              pr_bow_db** out) {
  if (!ctx) return PR_EINVAL;
  if (!out || max_sigs < 1 || max_sigs > PR_MAX_SIGS || cols < 1 || n_words < 1 || n_words > MAX_WORDS || max_postings < 0)
    return fail(ctx, PR_EINVAL, "pr_bow_db_create: bad arguments (max_sigs=%d, cols=%d, n_words=%d, max_postings=%lld; 1 <= n_words <= %d)",
                max_sigs, cols, n_words, (long long)max_postings, MAX_WORDS);
  *out = nullptr;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_bow_db* db = new pr_bow_db;
  db->device = pr::ctx_device(ctx);
  db->max_sigs = max_sigs; db->cols = cols; db->n_words = n_words; db->max_postings = max_postings;
  db->tail_cap = growable ? std::max(1, std::min(env_int("PR_BOW_TAIL_ROWS", 1024), max_sigs)) : 0;
  const int dchunk = (int)std::max<size_t>(1, std::min<size_t>(std::max(max_chunk, 1), SCRATCH_BYTES / ((size_t)8 * max_sigs)));
  db->chunk = std::max(1, std::min(env_int("PR_BOW_CHUNK", dchunk), dchunk));
  db->threads = env_int("PR_BOW_THREADS", 256) == 64 ? 64 : 256;
  db->tail_post_cap = (int64_t)db->tail_cap * (cols - 1);
  const size_t nw1 = (size_t)n_words + 1;
  hipError_t e = hipSuccess;
  auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  A(dalloc(db->moff, nw1)); A(dalloc(db->toff, nw1)); A(dalloc(db->cursor, nw1));
  A(dalloc(db->mrow, max_postings)); A(dalloc(db->mw, max_postings));
  if (growable) { A(dalloc(db->moff2, nw1)); A(dalloc(db->mrow2, max_postings)); A(dalloc(db->mw2, max_postings)); }   // fold targets
  A(dalloc(db->trow, db->tail_post_cap)); A(dalloc(db->tw, db->tail_post_cap));
  A(dalloc(db->traw, (size_t)2 * db->tail_cap * cols));
  A(dalloc(db->acc, (size_t)db->chunk * max_sigs));
  A(dalloc(db->counts, n_words)); A(dalloc(db->tsum, pr::bow_scan_tiles(n_words) + 1)); A(dalloc(db->stat, 2));
  if (e == hipSuccess) e = hipMemset(db->moff, 0, nw1 * sizeof(u64));
  if (e == hipSuccess) e = hipMemset(db->toff, 0, nw1 * sizeof(u64));
  if (e != hipSuccess) {
    release(db);
    return fail(ctx, pr::hip_code(e), "pr_bow_db_create: device allocation failed (%s)", hipGetErrorString(e));
  }
  *out = db;
  return PR_OK;
}

}  // namespace

extern "C" {

int pr_bow_db_create(pr_ctx* ctx, int32_t max_sigs, int32_t cols, int32_t n_words, int64_t max_postings, pr_bow_db** out) {
  return create_db(ctx, max_sigs, cols, n_words, max_postings, 4096, true, out);
}

void pr_bow_db_destroy(pr_ctx* ctx, pr_bow_db* db) {
  if (!db) return;
  if (ctx) {
    (void)hipSetDevice(pr::ctx_device(ctx));
    (void)hipStreamSynchronize(pr::ctx_stream(ctx));
  }
  release(db);
}

int32_t pr_bow_db_count(const pr_bow_db* db) { return db ? db->main_rows + db->tail_rows : 0; }

int pr_bow_db_set(pr_ctx* ctx, pr_bow_db* db, const double* rows, int where, int32_t n) {
  if (!ctx) return PR_EINVAL;
  return set_rows(ctx, "pr_bow_db_set", db, rows, where, n);
}

}  // extern "C"

namespace {

// pr_bow_db_set under the name of the entry point that called it (the host forms' errors name their own function)
int set_rows(pr_ctx* ctx, const char* fn, pr_bow_db* db, const double* rows, int where, int32_t n) {
  if (!db || n < 0 || (n > 0 && !rows) || (where != PR_HOST && where != PR_DEVICE))
    return fail(ctx, PR_EINVAL, "%s: bad arguments (n=%d, where=%d)", fn, n, where);
  if (n > db->max_sigs) return fail(ctx, PR_ENOMEM, "%s: %d rows exceed the capacity of %d", fn, n, db->max_sigs);
  PR_CHECK_HIP(ctx, hipSetDevice(db->device));
  hipStream_t st = pr::ctx_stream(ctx);
  DevTmp tmp;
  const double* d = rows;
  if (where == PR_HOST && n > 0) {
    const size_t bytes = (size_t)2 * n * db->cols * sizeof(double);
    PR_CHECK_HIP(ctx, hipMalloc(&tmp.p, bytes));
    PR_CHECK_HIP(ctx, hipMemcpyAsync(tmp.p, rows, bytes, hipMemcpyHostToDevice, st));
    d = static_cast<const double*>(tmp.p);
  }
  int64_t posts = 0;
  int bad = INT_MAX;
  if (int rc = check_rows(ctx, db, d, n, 0, true, &posts, &bad)) return rc;
  if (bad != INT_MAX) return bad_row_error(ctx, fn, bad, db->n_words);
  if (posts > db->max_postings)
    return fail(ctx, PR_ENOMEM, "%s: %lld postings exceed the capacity of %lld", fn, (long long)posts, (long long)db->max_postings);
  if (int rc = scatter_rows(ctx, db, d, n, 0, db->moff, db->mrow, db->mw)) return rc;
  PR_CHECK_HIP(ctx, hipMemsetAsync(db->toff, 0, ((size_t)db->n_words + 1) * sizeof(u64), st));
  db->main_rows = n; db->main_post = posts;
  db->tail_rows = 0; db->tail_post = 0;
  PR_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return PR_OK;
}

}  // namespace

extern "C" {

int pr_bow_db_append(pr_ctx* ctx, pr_bow_db* db, const double* rows, int where, int32_t n_new) {
  if (!ctx) return PR_EINVAL;
  if (db && db->tail_cap == 0) return fail(ctx, PR_EINVAL, "pr_bow_db_append: this database was created fixed");
  if (!db || n_new < 0 || (n_new > 0 && !rows) || (where != PR_HOST && where != PR_DEVICE))
    return fail(ctx, PR_EINVAL, "pr_bow_db_append: bad arguments (n_new=%d, where=%d)", n_new, where);
  if (n_new == 0) return PR_OK;
  const int32_t count = db->main_rows + db->tail_rows;
  if (n_new > db->max_sigs - count)
    return fail(ctx, PR_ENOMEM, "pr_bow_db_append: %d + %d rows exceed the capacity of %d", count, n_new, db->max_sigs);
  PR_CHECK_HIP(ctx, hipSetDevice(db->device));
  hipStream_t st = pr::ctx_stream(ctx);
  const size_t row2 = (size_t)2 * db->cols;
  DevTmp tmp;
  const double* d = rows;
  if (where == PR_HOST) {
    PR_CHECK_HIP(ctx, hipMalloc(&tmp.p, row2 * n_new * sizeof(double)));
    PR_CHECK_HIP(ctx, hipMemcpyAsync(tmp.p, rows, row2 * n_new * sizeof(double), hipMemcpyHostToDevice, st));
    d = static_cast<const double*>(tmp.p);
  }
  int64_t posts = 0;
  int bad = INT_MAX;
  if (int rc = check_rows(ctx, db, d, n_new, count, false, &posts, &bad)) return rc;
  if (bad != INT_MAX) return bad_row_error(ctx, "pr_bow_db_append", bad, db->n_words);
  if (posts > db->max_postings - db->main_post - db->tail_post)
    return fail(ctx, PR_ENOMEM, "pr_bow_db_append: %lld + %lld postings exceed the capacity of %lld", (long long)(db->main_post + db->tail_post),
                (long long)posts, (long long)db->max_postings);
  for (int32_t r0 = 0; r0 < n_new;) {
    if (db->tail_rows == db->tail_cap)
      if (int rc = fold(ctx, db)) return rc;
    const int32_t piece = std::min(n_new - r0, db->tail_cap - db->tail_rows);
    PR_CHECK_HIP(ctx, hipMemcpyAsync(db->traw + row2 * db->tail_rows, d + row2 * r0, row2 * piece * sizeof(double), hipMemcpyDeviceToDevice, st));
    db->tail_rows += piece;
    r0 += piece;
    if (int rc = rebuild_tail(ctx, db)) return rc;
  }
  PR_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return PR_OK;
}

int pr_bow_match_topk_dev(pr_ctx* ctx, const pr_bow_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0, int32_t mask_width,
                          int32_t k, int32_t* idx, double* score) {
  if (!ctx) return PR_EINVAL;
  if (!db || m < 0 || k < 1 || k > 128 || (m > 0 && (!q || !idx || !score)))
    return fail(ctx, PR_EINVAL, "pr_bow_match_topk_dev: bad arguments (m=%d, k=%d; 1 <= k <= 128)", m, k);
  if (m == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(db->device));
  return launch_match(ctx, db, q, m, q_row0, db_row0, mask_width, k, idx, score);
}

int pr_bow_match_topk_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, int32_t mask_width, int32_t k,
                          int32_t* idx, double* score) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || cols < 1 || k < 1 || k > 128 || (m > 0 && (!h1 || !idx || !score)) || (n > 0 && !h2) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_bow_match_topk_f64: bad arguments (m=%d, n=%d, cols=%d, k=%d; 1 <= k <= 128)", m, n, cols, k);
  if (m == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_bow_db* db = nullptr;
  if (int rc = host_db(ctx, "pr_bow_match_topk_f64", h1, m, h2, n, cols, m, &db)) return rc;
  const int rc = pr::resident::host_topk(ctx, "pr_bow_match_topk_f64", h1, (size_t)2 * m * cols * sizeof(double), m, k, idx, score,
                                        [&](const double* dq, int32_t* di, double* ds) { return launch_match(ctx, db, dq, m, 0, 0, mask_width, k, di, ds); });
  pr_bow_db_destroy(ctx, db);
  return rc;
}

int pr_bow_distance_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, double* dist) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || cols < 1 || (m > 0 && !h1) || (n > 0 && !h2) || (m > 0 && n > 0 && !dist) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_bow_distance_f64: bad arguments (m=%d, n=%d, cols=%d)", m, n, cols);
  if (m == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_bow_db* db = nullptr;
  if (int rc = host_db(ctx, "pr_bow_distance_f64", h1, m, h2, n, cols, 1 /* its matrix is the scratch */, &db)) return rc;
  if (n == 0) { pr_bow_db_destroy(ctx, db); return PR_OK; }
  hipStream_t st = pr::ctx_stream(ctx);
  void *dq = nullptr, *dd = nullptr;
  int rc = PR_OK;
  const size_t qb = (size_t)2 * m * cols * sizeof(double);
  hipError_t e = hipMalloc(&dq, qb);
  if (e == hipSuccess) e = hipMalloc(&dd, (size_t)m * n * sizeof(double));
  if (e == hipSuccess) e = hipMemcpyAsync(dq, h1, qb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    // k = 0: every query row's d stays in its accumulator row, here the rows of the output matrix (one launch over all m)
    pr::launch_bow_score(st, db->threads, static_cast<double*>(dq), m, cols, db->n_words, 0, db->moff, db->mrow, db->mw, db->toff, db->trow,
                         db->tw, n, 0, 0, 0, static_cast<double*>(dd), nullptr, nullptr, pr::ctx_bow_rows_flag(ctx));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(dist, dd, (size_t)m * n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) rc = fail(ctx, pr::hip_code(e), "pr_bow_distance_f64: %s", hipGetErrorString(e));
  (void)hipStreamSynchronize(st);
  for (void* p : {dq, dd}) if (p) (void)hipFree(p);
  pr_bow_db_destroy(ctx, db);
  return rc;
}

}  // extern "C"
