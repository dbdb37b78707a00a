// delight_match.cpp — host side of the two-stage exact DELIGHT matcher (delight_match.hip): the device-resident database (raw rows,
// fp32 image, empty-bin masks, coarse-exact flags), the stream-ordered top-k and the two host forms.
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

struct pr_delight_db {
  int device = -1;
  int32_t max_sigs = 0, count = 0;
  int32_t qcap = 0, xcap = 0;                  // queries per match chunk, exact rows per pass
  bool exact = false;
  int64_t bytes = 0;                           // device memory held
  double* raw = nullptr;                       // [max_sigs][16][256]
  float* img = nullptr;                        // [max_sigs][16][256] fp32 image (zero for a row that is not coarse-exact)
  unsigned* mask = nullptr;                    // [max_sigs][128] empty-bin masks in the matcher's lane layout
  int* ok = nullptr;                           // [max_sigs] coarse-exact flags
  unsigned* stat = nullptr;                    // [1] rows that are not coarse-exact
  float* qimg = nullptr;                       // scratch of one chunk: query image, masks, flags, lists, exact rows
  unsigned* qmask = nullptr;
  int* qok = nullptr;
  float *ckey = nullptr, *wout = nullptr;
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

#define DM_HIP(ctx, call)                                                                                         \
  do {                                                                                                            \
    hipError_t _e = (call);                                                                                       \
    if (_e != hipSuccess)                                                                                         \
      return fail(ctx, _e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
  } while (0)

constexpr int SIG = 4096;                      // doubles per signature
constexpr int MAX_CAND = 2048;                 // S * C of one query (delight_match.hip: DM_MAX_CAND)
constexpr int MAX_SLABS = 256;

// the last match call of every context (pr_delight_flagged_count): its database's count word and its query count
struct LastCall { const pr_delight_db* db; int32_t m; };
std::mutex g_last_mu;
std::map<const pr_ctx*, LastCall> g_last;

void release(pr_delight_db* db) {
  {
    std::lock_guard<std::mutex> lk(g_last_mu);
    for (auto it = g_last.begin(); it != g_last.end();) it = it->second.db == db ? g_last.erase(it) : std::next(it);
  }
  void* ps[] = {db->raw, db->img, db->mask, db->ok, db->stat, db->qimg, db->qmask, db->qok, db->ckey, db->wout, db->cand, db->flags,
                db->list, db->cnt, db->xrows};
  for (void* p : ps) if (p) (void)hipFree(p);
  delete db;
}

int create_db(pr_ctx* ctx, int32_t max_sigs, int32_t qcap, pr_delight_db** out) {
  if (!ctx) return PR_EINVAL;
  if (!out || max_sigs < 1 || max_sigs > PR_MAX_SIGS) return fail(ctx, PR_EINVAL, "pr_delight_db_create: bad arguments (max_sigs=%d)", max_sigs);
  *out = nullptr;
  DM_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_delight_db* db = new pr_delight_db;
  db->device = pr::ctx_device(ctx);
  db->max_sigs = max_sigs;
  db->qcap = std::max(1, qcap);
  db->xcap = std::min(256, db->qcap);
  { const char* s = getenv("PR_DELIGHT_EXACT"); db->exact = s && atoi(s) == 1; }
  hipError_t e = hipSuccess;
  auto A = [&](void** p, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (e == hipSuccess) { e = hipMalloc(p, bytes); if (e == hipSuccess) db->bytes += (int64_t)bytes; }
  };
  A((void**)&db->raw, (size_t)max_sigs * SIG * 8);
  A((void**)&db->img, (size_t)max_sigs * SIG * 4);
  A((void**)&db->mask, (size_t)max_sigs * 128 * 4);
  A((void**)&db->ok, (size_t)max_sigs * 4);
  A((void**)&db->stat, 4);
  A((void**)&db->qimg, (size_t)db->qcap * SIG * 4);
  A((void**)&db->qmask, (size_t)db->qcap * 128 * 4);
  A((void**)&db->qok, (size_t)db->qcap * 4);
  A((void**)&db->wout, (size_t)db->qcap * MAX_SLABS * 4);
  A((void**)&db->cand, (size_t)db->qcap * MAX_CAND * 4);
  A((void**)&db->ckey, (size_t)db->qcap * MAX_CAND * 4);
  A((void**)&db->flags, (size_t)db->qcap * 4); A((void**)&db->list, (size_t)db->qcap * 4); A((void**)&db->cnt, 8);
  A((void**)&db->xrows, (size_t)db->xcap * max_sigs * 8);
  if (e == hipSuccess) e = hipMemset(db->stat, 0, 4);
  if (e == hipSuccess) e = hipMemset(db->cnt, 0, 8);
  if (e != hipSuccess) {
    release(db);
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_delight_db_create: device allocation failed (%s)", hipGetErrorString(e));
  }
  *out = db;
  return PR_OK;
}

// rows [16 n_new][256] (host or device) become signatures count .. count + n_new - 1
int add_rows(pr_ctx* ctx, pr_delight_db* db, const double* rows, int where, int32_t n_new) {
  hipStream_t st = pr::ctx_stream(ctx);
  if (n_new > 0) {
    double* dst = db->raw + (size_t)db->count * SIG;
    DM_HIP(ctx, hipMemcpyAsync(dst, rows, (size_t)n_new * SIG * sizeof(double), where == PR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    pr::launch_delight_dpack(st, dst, n_new, db->count, db->img, db->mask, db->ok, db->stat);
    DM_HIP(ctx, hipGetLastError());
    db->count += n_new;
  }
  DM_HIP(ctx, hipStreamSynchronize(st));
  return PR_OK;
}

int launch_match(pr_ctx* ctx, const pr_delight_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0, int32_t mask_width, int32_t k,
                 int32_t* idx, double* score) {
  hipStream_t st = pr::ctx_stream(ctx);
  const int n = db->count, C = k + 8;
  const bool coarse = !db->exact && n > 0;     // otherwise every query takes the exact-row path
  DM_HIP(ctx, hipMemsetAsync(db->cnt + 1, 0, sizeof(int), st));
  for (int32_t c0 = 0; c0 < m; c0 += db->qcap) {
    const int mc = std::min(db->qcap, m - c0);
    const double* qc = q + (size_t)c0 * SIG;
    int32_t* ic = idx + (size_t)c0 * k;
    double* sc = score + (size_t)c0 * k;
    if (coarse) {
      const int qb = (mc + 3) / 4;
      int S = (2048 + qb - 1) / qb;                           // delight.hip: >= 4 rounds of 2 workgroups per CU
      S = std::min(S, std::min(MAX_CAND / C, MAX_SLABS));
      S = std::max(1, std::min(S, (n + 7) / 8));              // >= 8 entries per workgroup
      pr::launch_delight_dpack(st, qc, mc, 0, db->qimg, db->qmask, db->qok, nullptr);
      pr::launch_delight_coarse(st, db->qimg, mc, db->img, db->mask, n, S, C, q_row0 + c0, db_row0, mask_width, db->cand, db->ckey, db->wout);
      pr::launch_delight_rerank(st, qc, db->raw, mc, S, C, db->cand, db->ckey, db->wout, db->qok, db->stat, db_row0, k, ic, sc, db->flags);
    } else {
      pr::launch_gist_fill(st, db->flags, mc, 1);
    }
    pr::launch_gist_compact(st, db->flags, mc, db->list, db->cnt);
    for (int off = 0; off < mc; off += db->xcap) {
      const int cap = std::min(db->xcap, mc - off);
      pr::launch_delight_xdist(st, qc, db->raw, n, db->list, db->cnt, off, 0, cap, db->xrows, (size_t)db->max_sigs, q_row0 + c0, db_row0,
                               mask_width);
      pr::launch_gist_xselect(st, db->xrows, (size_t)db->max_sigs, n, db->list, db->cnt, off, cap, db_row0, k, ic, sc);
    }
  }
  DM_HIP(ctx, hipGetLastError());
  {
    std::lock_guard<std::mutex> lk(g_last_mu);
    g_last[ctx] = LastCall{db, m};
  }
  return PR_OK;
}

}  // namespace

extern "C" {

int pr_delight_db_create(pr_ctx* ctx, int32_t max_sigs, pr_delight_db** out) { return create_db(ctx, max_sigs, 4096, out); }

void pr_delight_db_destroy(pr_ctx* ctx, pr_delight_db* db) {
  if (!db) return;
  if (ctx) {
    (void)hipSetDevice(pr::ctx_device(ctx));
    (void)hipStreamSynchronize(pr::ctx_stream(ctx));
  }
  release(db);
}

int32_t pr_delight_db_count(const pr_delight_db* db) { return db ? db->count : 0; }
int64_t pr_delight_db_bytes(const pr_delight_db* db) { return db ? db->bytes : 0; }
void pr_delight_db_set_exact(pr_delight_db* db, int on) { if (db) db->exact = on != 0; }

int pr_delight_db_set(pr_ctx* ctx, pr_delight_db* db, const double* rows, int where, int32_t n) {
  if (!ctx) return PR_EINVAL;
  if (!db || n < 0 || (n > 0 && !rows) || (where != PR_HOST && where != PR_DEVICE))
    return fail(ctx, PR_EINVAL, "pr_delight_db_set: bad arguments (n=%d, where=%d)", n, where);
  if (n > db->max_sigs) return fail(ctx, PR_ENOMEM, "pr_delight_db_set: %d signatures exceed the capacity of %d", n, db->max_sigs);
  DM_HIP(ctx, hipSetDevice(db->device));
  DM_HIP(ctx, hipMemsetAsync(db->stat, 0, 4, pr::ctx_stream(ctx)));
  db->count = 0;
  return add_rows(ctx, db, rows, where, n);
}

int pr_delight_db_append(pr_ctx* ctx, pr_delight_db* db, const double* rows, int where, int32_t n_new) {
  if (!ctx) return PR_EINVAL;
  if (!db || n_new < 0 || (n_new > 0 && !rows) || (where != PR_HOST && where != PR_DEVICE))
    return fail(ctx, PR_EINVAL, "pr_delight_db_append: bad arguments (n_new=%d, where=%d)", n_new, where);
  if (n_new > db->max_sigs - db->count)
    return fail(ctx, PR_ENOMEM, "pr_delight_db_append: %d + %d signatures exceed the capacity of %d", db->count, n_new, db->max_sigs);
  DM_HIP(ctx, hipSetDevice(db->device));
  return add_rows(ctx, db, rows, where, n_new);
}

int pr_delight_match_topk_dev(pr_ctx* ctx, const pr_delight_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0,
                              int32_t mask_width, int32_t k, int32_t* idx, double* score) {
  if (!ctx) return PR_EINVAL;
  if (!db || m < 0 || k < 1 || k > 128 || (m > 0 && (!q || !idx || !score)))
    return fail(ctx, PR_EINVAL, "pr_delight_match_topk_dev: bad arguments (m=%d, k=%d; 1 <= k <= 128)", m, k);
  if (m == 0) return PR_OK;
  DM_HIP(ctx, hipSetDevice(db->device));
  return launch_match(ctx, db, q, m, q_row0, db_row0, mask_width, k, idx, score);
}

int pr_delight_flagged_count(pr_ctx* ctx, int32_t m, int32_t* count) {
  if (!ctx) return PR_EINVAL;
  LastCall last{nullptr, 0};
  {
    std::lock_guard<std::mutex> lk(g_last_mu);
    auto it = g_last.find(ctx);
    if (it != g_last.end()) last = it->second;
  }
  if (!count || !last.db || m != last.m)
    return fail(ctx, PR_EINVAL, "pr_delight_flagged_count: m=%d is not the query count of this context's last pr_delight_match_topk_dev (%d)", m,
                last.db ? last.m : -1);
  DM_HIP(ctx, hipSetDevice(last.db->device));
  hipStream_t st = pr::ctx_stream(ctx);
  int c = 0;
  DM_HIP(ctx, hipMemcpyAsync(&c, last.db->cnt + 1, sizeof(int), hipMemcpyDeviceToHost, st));
  DM_HIP(ctx, hipStreamSynchronize(st));
  *count = c;
  return PR_OK;
}

int pr_delight_match_topk_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t mask_width, int32_t k, int32_t* idx,
                              double* score) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || k < 1 || k > 128 || (m > 0 && (!h1 || !idx || !score)) || (n > 0 && !h2) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_delight_match_topk_f64: bad arguments (m=%d, n=%d, k=%d; 1 <= k <= 128)", m, n, k);
  if (m == 0) return PR_OK;
  DM_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_delight_db* db = nullptr;
  if (int rc = create_db(ctx, std::max(n, 1), std::min(m, 4096), &db)) return rc;
  int rc = pr_delight_db_set(ctx, db, h2, PR_HOST, n);
  hipStream_t st = pr::ctx_stream(ctx);
  void *dq = nullptr, *di = nullptr, *ds = nullptr;
  if (rc == PR_OK) {
    const size_t qb = (size_t)m * SIG * sizeof(double);
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
      rc = fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_delight_match_topk_f64: %s", hipGetErrorString(e));
  }
  (void)hipStreamSynchronize(st);
  for (void* p : {dq, di, ds}) if (p) (void)hipFree(p);
  pr_delight_db_destroy(ctx, db);
  return rc;
}

int pr_delight_distance_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, double* dist) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || (m > 0 && !h1) || (n > 0 && !h2) || (m > 0 && n > 0 && !dist) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_delight_distance_f64: bad arguments (m=%d, n=%d)", m, n);
  if (m == 0 || n == 0) return PR_OK;
  DM_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  void *dq = nullptr, *db = nullptr, *dd = nullptr;
  int rc = PR_OK;
  const size_t qb = (size_t)m * SIG * sizeof(double), bb = (size_t)n * SIG * sizeof(double), ob = (size_t)m * n * sizeof(double);
  hipError_t e = hipMalloc(&dq, qb);
  if (e == hipSuccess) e = hipMalloc(&db, bb);
  if (e == hipSuccess) e = hipMalloc(&dd, ob);
  if (e == hipSuccess) e = hipMemcpyAsync(dq, h1, qb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(db, h2, bb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    constexpr int PASS = 1 << 15;              // slots of one launch
    for (int off = 0; off < m; off += PASS) {
      const int cap = std::min(PASS, m - off);
      pr::launch_delight_xdist(st, static_cast<double*>(dq), static_cast<double*>(db), n, nullptr, nullptr, off, cap, cap,
                               static_cast<double*>(dd) + (size_t)off * n, (size_t)n, 0, 0, 0);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(dist, dd, ob, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_delight_distance_f64: %s", hipGetErrorString(e));
  (void)hipStreamSynchronize(st);
  for (void* p : {dq, db, dd}) if (p) (void)hipFree(p);
  return rc;
}

}  // extern "C"
