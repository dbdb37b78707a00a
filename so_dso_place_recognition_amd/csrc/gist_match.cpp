// gist_match.cpp — host side of the two-stage exact GIST matcher (gist_match.hip): the device-resident database (raw rows, f16 image,
// norms), the stream-ordered top-k and the two host forms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "../../include/place_recognition.h"
#include "kernels.hpp"

struct pr_gist_db {
  int device = -1;
  int32_t max_sigs = 0, cols = 0, KP = 0, KS = 0, count = 0;
  int32_t qcap = 0, xcap = 0;                  // queries per match chunk, exact rows per pass
  bool exact = false, mu_set = false, centre = true;
  int64_t bytes = 0;                           // device memory held
  double* raw = nullptr;                       // [max_sigs][cols]
  void* img = nullptr;                         // f16 operand image, tiles of 32 rows
  float *nd = nullptr, *rs = nullptr;          // [max_sigs] |a'|^2, residual norm
  unsigned* stat = nullptr;                    // [2] max nd, max rs (float bits)
  double* mu = nullptr;                        // [cols] the vector the pack subtracts
  void* qimg = nullptr;                        // scratch of one chunk: query image, norms, lists, flags, exact rows
  float *qn = nullptr, *qr = nullptr, *wout = nullptr;
  int *cand = nullptr, *flags = nullptr, *list = nullptr, *cnt = nullptr;
  double* xrows = nullptr;                     // [xcap][max_sigs]
};

namespace {

int fail(pr_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int fail(pr_ctx* ctx, int code, const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  pr::ctx_set_error(ctx, b);
  return code;
}

#define GM_HIP(ctx, call)                                                                                         \
  do {                                                                                                            \
    hipError_t _e = (call);                                                                                       \
    if (_e != hipSuccess)                                                                                         \
      return fail(ctx, _e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
  } while (0)

constexpr int MAX_CAND = 2048;                 // S * C of one query (gist_match.hip: GM_MAX_CAND)
constexpr int MAX_SLABS = 256;
constexpr int MEAN_ROWS = 1024;
constexpr size_t MAX_LDS = 160 * 1024;

// the last match call of every context (pr_gist_flagged_count): its database's count word and its query count
struct LastCall { const pr_gist_db* db; int32_t m; };
std::mutex g_last_mu;
std::map<const pr_ctx*, LastCall> g_last;

void release(pr_gist_db* db) {
  {
    std::lock_guard<std::mutex> lk(g_last_mu);
    for (auto it = g_last.begin(); it != g_last.end();) it = it->second.db == db ? g_last.erase(it) : std::next(it);
  }
  void* ps[] = {db->raw, db->img, db->nd, db->rs, db->stat, db->mu, db->qimg, db->qn, db->qr, db->wout, db->cand, db->flags, db->list,
                db->cnt, db->xrows};
  for (void* p : ps) if (p) (void)hipFree(p);
  delete db;
}

int create_db(pr_ctx* ctx, int32_t max_sigs, int32_t cols, int32_t qcap, pr_gist_db** out) {
  if (!ctx) return PR_EINVAL;
  if (!out || max_sigs < 1 || max_sigs > PR_MAX_SIGS || cols < 1 || cols > (1 << 20))
    return fail(ctx, PR_EINVAL, "pr_gist_db_create: bad arguments (max_sigs=%d, cols=%d)", max_sigs, cols);
  *out = nullptr;
  GM_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_gist_db* db = new pr_gist_db;
  db->device = pr::ctx_device(ctx);
  db->max_sigs = max_sigs; db->cols = cols;
  db->KP = ((cols + 63) / 64) * 64; db->KS = db->KP / 16;
  db->qcap = std::max(1, qcap);
  db->xcap = std::min(256, db->qcap);
  { const char* s = getenv("PR_GIST_EXACT"); db->exact = s && atoi(s) == 1; }
  { const char* s = getenv("PR_GIST_CENTRE"); db->centre = !(s && *s && atoi(s) == 0); }   // PR_GIST_CENTRE=0: mu = 0 (A/B runs of the bound)
  hipError_t e = hipSuccess;
  auto A = [&](void** p, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (e == hipSuccess) { e = hipMalloc(p, bytes); if (e == hipSuccess) db->bytes += (int64_t)bytes; }
  };
  const size_t tiles = ((size_t)max_sigs + 31) / 32, qtiles = ((size_t)db->qcap + 31) / 32, tile_bytes = (size_t)db->KP * 64;
  A((void**)&db->raw, (size_t)max_sigs * cols * 8);
  A(&db->img, tiles * tile_bytes);
  A((void**)&db->nd, tiles * 32 * 4); A((void**)&db->rs, tiles * 32 * 4);
  A((void**)&db->stat, 8); A((void**)&db->mu, (size_t)cols * 8);
  A(&db->qimg, qtiles * tile_bytes);
  A((void**)&db->qn, qtiles * 32 * 4); A((void**)&db->qr, qtiles * 32 * 4);
  A((void**)&db->wout, (size_t)db->qcap * MAX_SLABS * 4);
  A((void**)&db->cand, (size_t)db->qcap * MAX_CAND * 4);
  A((void**)&db->flags, (size_t)db->qcap * 4); A((void**)&db->list, (size_t)db->qcap * 4); A((void**)&db->cnt, 8);
  A((void**)&db->xrows, (size_t)db->xcap * max_sigs * 8);
  if (e == hipSuccess) e = hipMemset(db->stat, 0, 8);
  if (e == hipSuccess) e = hipMemset(db->cnt, 0, 8);
  if (e == hipSuccess) e = hipMemset(db->mu, 0, (size_t)cols * 8);
  if (e != hipSuccess) {
    release(db);
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_gist_db_create: device allocation failed (%s)", hipGetErrorString(e));
  }
  *out = db;
  return PR_OK;
}

// rows [n_new][cols] (host or device) become rows count .. count + n_new - 1
int add_rows(pr_ctx* ctx, pr_gist_db* db, const double* rows, int where, int32_t n_new) {
  hipStream_t st = pr::ctx_stream(ctx);
  if (n_new > 0) {
    double* dst = db->raw + (size_t)db->count * db->cols;
    GM_HIP(ctx, hipMemcpyAsync(dst, rows, (size_t)n_new * db->cols * sizeof(double), where == PR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    if (!db->mu_set) {         // fixed by the first rows the database receives after a set; never re-derived
      if (db->centre) pr::launch_gist_mean(st, dst, std::min(n_new, MEAN_ROWS), db->cols, db->mu);
      db->mu_set = true;
    }
    pr::launch_gist_pack(st, dst, n_new, db->cols, db->KS, db->mu, db->count, db->img, db->nd, db->rs, db->stat);
    GM_HIP(ctx, hipGetLastError());
    db->count += n_new;
  }
  GM_HIP(ctx, hipStreamSynchronize(st));
  return PR_OK;
}

int launch_match(pr_ctx* ctx, const pr_gist_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0, int32_t mask_width, int32_t k,
                 int32_t* idx, double* score) {
  hipStream_t st = pr::ctx_stream(ctx);
  const int n = db->count, C = k + 8;
  const bool coarse = !db->exact && pr::gist_coarse_lds_bytes(db->KS, C) <= MAX_LDS;   // otherwise every query takes the exact-row path
  GM_HIP(ctx, hipMemsetAsync(db->cnt + 1, 0, sizeof(int), st));
  for (int32_t c0 = 0; c0 < m; c0 += db->qcap) {
    const int mc = std::min(db->qcap, m - c0);
    const double* qc = q + (size_t)c0 * db->cols;
    int32_t* ic = idx + (size_t)c0 * k;
    double* sc = score + (size_t)c0 * k;
    if (coarse) {
      const int qtiles = (mc + 31) / 32, DT = (n + 31) / 32;
      int S = std::max(4, (1536 + qtiles - 1) / qtiles);
      S = std::min(S, std::min(MAX_CAND / C, MAX_SLABS));
      S = std::max(1, std::min(S, DT));
      pr::launch_gist_pack(st, qc, mc, db->cols, db->KS, db->mu, 0, db->qimg, db->qn, db->qr, nullptr);
      pr::launch_gist_coarse(st, db->qimg, db->qn, mc, db->img, db->nd, n, db->KS, S, C, q_row0 + c0, db_row0, mask_width, db->cand, db->wout);
      pr::launch_gist_rerank(st, qc, db->raw, db->cols, db->KP, mc, S, C, db->cand, db->wout, db->qn, db->qr, db->stat, db_row0, k, ic, sc,
                             db->flags);
    } else {
      pr::launch_gist_fill(st, db->flags, mc, 1);
    }
    pr::launch_gist_compact(st, db->flags, mc, db->list, db->cnt);
    for (int off = 0; off < mc; off += db->xcap) {
      const int cap = std::min(db->xcap, mc - off);
      pr::launch_gist_xdist(st, qc, db->raw, db->cols, n, db->list, db->cnt, off, 0, cap, db->xrows, (size_t)db->max_sigs, q_row0 + c0, db_row0,
                            mask_width);
      pr::launch_gist_xselect(st, db->xrows, (size_t)db->max_sigs, n, db->list, db->cnt, off, cap, db_row0, k, ic, sc);
    }
  }
  GM_HIP(ctx, hipGetLastError());
  {
    std::lock_guard<std::mutex> lk(g_last_mu);
    g_last[ctx] = LastCall{db, m};
  }
  return PR_OK;
}

}  // namespace

extern "C" {

int pr_gist_db_create(pr_ctx* ctx, int32_t max_sigs, int32_t cols, pr_gist_db** out) { return create_db(ctx, max_sigs, cols, 4096, out); }

void pr_gist_db_destroy(pr_ctx* ctx, pr_gist_db* db) {
  if (!db) return;
  if (ctx) {
    (void)hipSetDevice(pr::ctx_device(ctx));
    (void)hipStreamSynchronize(pr::ctx_stream(ctx));
  }
  release(db);
}

int32_t pr_gist_db_count(const pr_gist_db* db) { return db ? db->count : 0; }
int64_t pr_gist_db_bytes(const pr_gist_db* db) { return db ? db->bytes : 0; }
void pr_gist_db_set_exact(pr_gist_db* db, int on) { if (db) db->exact = on != 0; }

int pr_gist_db_set(pr_ctx* ctx, pr_gist_db* db, const double* rows, int where, int32_t n) {
  if (!ctx) return PR_EINVAL;
  if (!db || n < 0 || (n > 0 && !rows) || (where != PR_HOST && where != PR_DEVICE))
    return fail(ctx, PR_EINVAL, "pr_gist_db_set: bad arguments (n=%d, where=%d)", n, where);
  if (n > db->max_sigs) return fail(ctx, PR_ENOMEM, "pr_gist_db_set: %d rows exceed the capacity of %d", n, db->max_sigs);
  GM_HIP(ctx, hipSetDevice(db->device));
  hipStream_t st = pr::ctx_stream(ctx);
  GM_HIP(ctx, hipMemsetAsync(db->stat, 0, 8, st));
  GM_HIP(ctx, hipMemsetAsync(db->mu, 0, (size_t)db->cols * 8, st));
  db->count = 0;
  db->mu_set = false;
  return add_rows(ctx, db, rows, where, n);
}

int pr_gist_db_append(pr_ctx* ctx, pr_gist_db* db, const double* rows, int where, int32_t n_new) {
  if (!ctx) return PR_EINVAL;
  if (!db || n_new < 0 || (n_new > 0 && !rows) || (where != PR_HOST && where != PR_DEVICE))
    return fail(ctx, PR_EINVAL, "pr_gist_db_append: bad arguments (n_new=%d, where=%d)", n_new, where);
  if (n_new > db->max_sigs - db->count)
    return fail(ctx, PR_ENOMEM, "pr_gist_db_append: %d + %d rows exceed the capacity of %d", db->count, n_new, db->max_sigs);
  GM_HIP(ctx, hipSetDevice(db->device));
  return add_rows(ctx, db, rows, where, n_new);
}

int pr_gist_match_topk_dev(pr_ctx* ctx, const pr_gist_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0, int32_t mask_width,
                           int32_t k, int32_t* idx, double* score) {
  if (!ctx) return PR_EINVAL;
  if (!db || m < 0 || k < 1 || k > 128 || (m > 0 && (!q || !idx || !score)))
    return fail(ctx, PR_EINVAL, "pr_gist_match_topk_dev: bad arguments (m=%d, k=%d; 1 <= k <= 128)", m, k);
  if (m == 0) return PR_OK;
  GM_HIP(ctx, hipSetDevice(db->device));
  return launch_match(ctx, db, q, m, q_row0, db_row0, mask_width, k, idx, score);
}

int pr_gist_flagged_count(pr_ctx* ctx, int32_t m, int32_t* count) {
  if (!ctx) return PR_EINVAL;
  LastCall last{nullptr, 0};
  {
    std::lock_guard<std::mutex> lk(g_last_mu);
    auto it = g_last.find(ctx);
    if (it != g_last.end()) last = it->second;
  }
  if (!count || !last.db || m != last.m)
    return fail(ctx, PR_EINVAL, "pr_gist_flagged_count: m=%d is not the query count of this context's last pr_gist_match_topk_dev (%d)", m,
                last.db ? last.m : -1);
  GM_HIP(ctx, hipSetDevice(last.db->device));
  hipStream_t st = pr::ctx_stream(ctx);
  int c = 0;
  GM_HIP(ctx, hipMemcpyAsync(&c, last.db->cnt + 1, sizeof(int), hipMemcpyDeviceToHost, st));
  GM_HIP(ctx, hipStreamSynchronize(st));
  *count = c;
  return PR_OK;
}

int pr_gist_match_topk_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, int32_t mask_width, int32_t k,
                           int32_t* idx, double* score) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || cols < 1 || k < 1 || k > 128 || (m > 0 && (!h1 || !idx || !score)) || (n > 0 && !h2) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_gist_match_topk_f64: bad arguments (m=%d, n=%d, cols=%d, k=%d; 1 <= k <= 128)", m, n, cols, k);
  if (m == 0) return PR_OK;
  GM_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_gist_db* db = nullptr;
  if (int rc = create_db(ctx, std::max(n, 1), cols, std::min(m, 4096), &db)) return rc;
  int rc = pr_gist_db_set(ctx, db, h2, PR_HOST, n);
  hipStream_t st = pr::ctx_stream(ctx);
  void *dq = nullptr, *di = nullptr, *ds = nullptr;
  if (rc == PR_OK) {
    const size_t qb = (size_t)m * cols * sizeof(double);
    hipError_t e = hipMalloc(&dq, qb);
    if (e == hipSuccess) e = hipMalloc(&di, (size_t)m * k * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&ds, (size_t)m * k * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(dq, h1, qb, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
      rc = launch_match(ctx, db, static_cast<double*>(dq), m, 0, 0, mask_width, k, static_cast<int32_t*>(di), static_cast<double*>(ds));
      if (rc == PR_OK) {
        e = hipMemcpyAsync(idx, di, (size_t)m * k * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(score, ds, (size_t)m * k * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
      }
    }
    if (e != hipSuccess && rc == PR_OK)
      rc = fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_gist_match_topk_f64: %s", hipGetErrorString(e));
  }
  (void)hipStreamSynchronize(st);
  for (void* p : {dq, di, ds}) if (p) (void)hipFree(p);
  pr_gist_db_destroy(ctx, db);
  return rc;
}

int pr_gist_distance_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, double* dist) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || cols < 1 || (m > 0 && !h1) || (n > 0 && !h2) || (m > 0 && n > 0 && !dist) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_gist_distance_f64: bad arguments (m=%d, n=%d, cols=%d)", m, n, cols);
  if (m == 0 || n == 0) return PR_OK;
  GM_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  void *dq = nullptr, *db = nullptr, *dd = nullptr;
  int rc = PR_OK;
  const size_t qb = (size_t)m * cols * sizeof(double), bb = (size_t)n * cols * sizeof(double), ob = (size_t)m * n * sizeof(double);
  hipError_t e = hipMalloc(&dq, qb);
  if (e == hipSuccess) e = hipMalloc(&db, bb);
  if (e == hipSuccess) e = hipMalloc(&dd, ob);
  if (e == hipSuccess) e = hipMemcpyAsync(dq, h1, qb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(db, h2, bb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    constexpr int PASS = 1 << 16;
    for (int off = 0; off < m; off += PASS) {
      const int cap = std::min(PASS, m - off);
      pr::launch_gist_xdist(st, static_cast<double*>(dq), static_cast<double*>(db), cols, n, nullptr, nullptr, off, cap, cap,
                            static_cast<double*>(dd) + (size_t)off * n, (size_t)n, 0, 0, 0);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(dist, dd, ob, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_gist_distance_f64: %s", hipGetErrorString(e));
  (void)hipStreamSynchronize(st);
  for (void* p : {dq, db, dd}) if (p) (void)hipFree(p);
  return rc;
}

}  // extern "C"
