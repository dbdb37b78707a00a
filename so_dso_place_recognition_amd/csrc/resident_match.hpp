// resident_match.hpp — the host code the device-resident exact matchers share.
//   BoW, GIST, DELIGHT: the host forms of a top-k (host_topk) and of a distance matrix through an xdist kernel (host_distance).
//   GIST, DELIGHT: the two-stage database - a coarse pass lists candidates per (query, DB slab), their distances are re-evaluated in
//   fp64, and a query whose list is not provably complete is answered from its exact row.  What a kind adds (its operand image, its pack,
//   its slab geometry, its coarse / rerank / xdist launches) comes in as a traits struct K:
//     using Db = the kind's struct (derived from resident::Db);  static constexpr Kind kind;
//     static constexpr const char *prefix ("pr_gist"), *unit ("rows": what the capacity messages count);
//     static size_t sig_doubles(const Db*)                                doubles per signature
//     static hipError_t reset(hipStream_t, Db*)                           set: what the kind clears in front of the first rows
//     static void pack(hipStream_t, Db*, const double* dst, int32_t n)    rows dst (in db->raw already) become signatures count ..
//     static bool coarse(const Db*, int n, int C)                         whether the coarse stage can run at all
//     static void launch_coarse(...)                                      query pack + coarse + rerank of one chunk: idx / score / flags
//     static void launch_xdist(...)                                       the exact rows of list slots [off, off + cap) into db->xrows
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "host_common.hpp"

namespace pr {
namespace resident {

// m queries of q_bytes (host) -> idx / score [m][k] (host) through `match(dq, di, ds)`, the kind's stream-ordered top-k on device buffers
template <class Match>
int host_topk(pr_ctx* ctx, const char* fn, const double* h1, size_t q_bytes, int32_t m, int32_t k, int32_t* idx, double* score, Match match) {
  hipStream_t st = ctx_stream(ctx);
  void *dq = nullptr, *di = nullptr, *ds = nullptr;
  int rc = PR_OK;
  hipError_t e = hipMalloc(&dq, q_bytes);
  if (e == hipSuccess) e = hipMalloc(&di, (size_t)m * k * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc(&ds, (size_t)m * k * sizeof(double));
  if (e == hipSuccess) e = hipMemcpyAsync(dq, h1, q_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    rc = match(static_cast<double*>(dq), static_cast<int32_t*>(di), static_cast<double*>(ds));
    if (rc == PR_OK) {
      e = hipMemcpyAsync(idx, di, (size_t)m * k * sizeof(int32_t), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipMemcpyAsync(score, ds, (size_t)m * k * sizeof(double), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
  }
  if (e != hipSuccess && rc == PR_OK) rc = fail(ctx, hip_code(e), "%s: %s", fn, hipGetErrorString(e));
  (void)hipStreamSynchronize(st);
  for (void* p : {dq, di, ds}) if (p) (void)hipFree(p);
  return rc;
}

// dist [m][n] (host) of host signatures of sig_bytes each; xdist(st, dq, db, off, cap, out): rows [off, off + cap) of it, `pass` at most
template <class XDist>
int host_distance(pr_ctx* ctx, const char* fn, const double* h1, int32_t m, const double* h2, int32_t n, size_t sig_bytes, int pass,
                  double* dist, XDist xdist) {
  hipStream_t st = ctx_stream(ctx);
  void *dq = nullptr, *db = nullptr, *dd = nullptr;
  int rc = PR_OK;
  const size_t qb = (size_t)m * sig_bytes, bb = (size_t)n * sig_bytes, ob = (size_t)m * n * sizeof(double);
  hipError_t e = hipMalloc(&dq, qb);
  if (e == hipSuccess) e = hipMalloc(&db, bb);
  if (e == hipSuccess) e = hipMalloc(&dd, ob);
  if (e == hipSuccess) e = hipMemcpyAsync(dq, h1, qb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(db, h2, bb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    for (int off = 0; off < m; off += pass) {
      const int cap = std::min(pass, m - off);
      xdist(st, static_cast<double*>(dq), static_cast<double*>(db), off, cap, static_cast<double*>(dd) + (size_t)off * n);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(dist, dd, ob, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) rc = fail(ctx, hip_code(e), "%s: %s", fn, hipGetErrorString(e));
  (void)hipStreamSynchronize(st);
  for (void* p : {dq, db, dd}) if (p) (void)hipFree(p);
  return rc;
}

// ------------------------------------------------------------------ the two-stage databases
constexpr int MAX_CAND = 2048;                 // S * C of one query (gist_match.hip: GM_MAX_CAND, delight_match.hip: DM_MAX_CAND)
constexpr int MAX_SLABS = 256;
constexpr int QCAP = 4096;                     // queries per match chunk of a database made by *_db_create

enum Kind { GIST, DELIGHT };

struct Db {
  int device = -1;
  int32_t max_sigs = 0, count = 0;
  int32_t qcap = 0, xcap = 0;                  // queries per match chunk, exact rows per pass
  bool exact = false;
  int64_t bytes = 0;                           // device memory held
  std::vector<void*> held;                     // every allocation, for release
  double* raw = nullptr;                       // [max_sigs] signatures
  float* wout = nullptr;                       // scratch of one chunk: the slabs' worst kept keys, candidate lists, flags, exact rows
  int *cand = nullptr, *flags = nullptr, *list = nullptr, *cnt = nullptr;
  double* xrows = nullptr;                     // [xcap][max_sigs]
};

// the last match call of every (kind, context) (pr_*_flagged_count): its database's count word and its query count
// (resident_match.cpp; forget() drops the entries of a database that goes away)
struct LastCall { const Db* db; int32_t m; };
void remember(Kind kind, const pr_ctx* ctx, const Db* db, int32_t m);
LastCall last_call(Kind kind, const pr_ctx* ctx);
void forget(const Db* db);

// device allocations of a database under construction: the first failure sticks, the rest are skipped
struct Alloc {
  Db* db;
  hipError_t e = hipSuccess;
  template <class T>
  void operator()(T*& p, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (e == hipSuccess) e = hipMalloc((void**)&p, bytes);
    if (e == hipSuccess) { db->held.push_back(p); db->bytes += (int64_t)bytes; }
  }
  void zero(void* p, size_t bytes) { if (e == hipSuccess) e = hipMemset(p, 0, bytes); }
};

template <class DB>
void release(DB* db) {
  forget(db);
  for (void* p : db->held) (void)hipFree(p);
  delete db;
}

// the caller has checked its arguments; own(db, A): the kind's fields (what sig_doubles() reads among them), buffers and their memsets
template <class K, class Own>
int create(pr_ctx* ctx, int32_t max_sigs, int32_t qcap, const char* exact_env, typename K::Db** out, Own own) {
  *out = nullptr;
  PR_CHECK_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  typename K::Db* db = new typename K::Db;
  db->device = ctx_device(ctx);
  db->max_sigs = max_sigs;
  db->qcap = std::max(1, qcap);
  db->xcap = std::min(256, db->qcap);
  { const char* s = getenv(exact_env); db->exact = s && atoi(s) == 1; }
  Alloc A{db};
  own(db, A);
  A(db->raw, (size_t)max_sigs * K::sig_doubles(db) * 8);
  A(db->wout, (size_t)db->qcap * MAX_SLABS * 4);
  A(db->cand, (size_t)db->qcap * MAX_CAND * 4);
  A(db->flags, (size_t)db->qcap * 4); A(db->list, (size_t)db->qcap * 4); A(db->cnt, 8);
  A(db->xrows, (size_t)db->xcap * max_sigs * 8);
  A.zero(db->cnt, 8);
  if (A.e != hipSuccess) {
    release(db);
    return fail(ctx, hip_code(A.e), "%s_db_create: device allocation failed (%s)", K::prefix, hipGetErrorString(A.e));
  }
  *out = db;
  return PR_OK;
}

template <class DB>
void destroy(pr_ctx* ctx, DB* db) {
  if (!db) return;
  if (ctx) {
    (void)hipSetDevice(ctx_device(ctx));
    (void)hipStreamSynchronize(ctx_stream(ctx));
  }
  release(db);
}

// rows [n_new] signatures (host or device) become signatures count .. count + n_new - 1
template <class K>
int add_rows(pr_ctx* ctx, typename K::Db* db, const double* rows, int where, int32_t n_new) {
  hipStream_t st = ctx_stream(ctx);
  if (n_new > 0) {
    const size_t sig = K::sig_doubles(db);
    double* dst = db->raw + (size_t)db->count * sig;
    PR_CHECK_HIP(ctx, hipMemcpyAsync(dst, rows, (size_t)n_new * sig * sizeof(double), where == PR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    K::pack(st, db, dst, n_new);
    PR_CHECK_HIP(ctx, hipGetLastError());
    db->count += n_new;
  }
  PR_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return PR_OK;
}

template <class K>
int set(pr_ctx* ctx, typename K::Db* db, const double* rows, int where, int32_t n) {
  if (!ctx) return PR_EINVAL;
  if (!db || n < 0 || (n > 0 && !rows) || (where != PR_HOST && where != PR_DEVICE))
    return fail(ctx, PR_EINVAL, "%s_db_set: bad arguments (n=%d, where=%d)", K::prefix, n, where);
  if (n > db->max_sigs) return fail(ctx, PR_ENOMEM, "%s_db_set: %d %s exceed the capacity of %d", K::prefix, n, K::unit, db->max_sigs);
  PR_CHECK_HIP(ctx, hipSetDevice(db->device));
  PR_CHECK_HIP(ctx, K::reset(ctx_stream(ctx), db));
  db->count = 0;
  return add_rows<K>(ctx, db, rows, where, n);
}

template <class K>
int append(pr_ctx* ctx, typename K::Db* db, const double* rows, int where, int32_t n_new) {
  if (!ctx) return PR_EINVAL;
  if (!db || n_new < 0 || (n_new > 0 && !rows) || (where != PR_HOST && where != PR_DEVICE))
    return fail(ctx, PR_EINVAL, "%s_db_append: bad arguments (n_new=%d, where=%d)", K::prefix, n_new, where);
  if (n_new > db->max_sigs - db->count)
    return fail(ctx, PR_ENOMEM, "%s_db_append: %d + %d %s exceed the capacity of %d", K::prefix, db->count, n_new, K::unit, db->max_sigs);
  PR_CHECK_HIP(ctx, hipSetDevice(db->device));
  return add_rows<K>(ctx, db, rows, where, n_new);
}

// the caller has checked its arguments and set the device
template <class K>
int launch_match(pr_ctx* ctx, const typename K::Db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0, int32_t mask_width,
                 int32_t k, int32_t* idx, double* score) {
  hipStream_t st = ctx_stream(ctx);
  const int n = db->count, C = k + 8;
  const bool coarse = !db->exact && K::coarse(db, n, C);   // otherwise every query takes the exact-row path
  PR_CHECK_HIP(ctx, hipMemsetAsync(db->cnt + 1, 0, sizeof(int), st));
  for (int32_t c0 = 0; c0 < m; c0 += db->qcap) {
    const int mc = std::min(db->qcap, m - c0);
    const double* qc = q + (size_t)c0 * K::sig_doubles(db);
    int32_t* ic = idx + (size_t)c0 * k;
    double* sc = score + (size_t)c0 * k;
    if (coarse) K::launch_coarse(st, db, qc, mc, n, C, q_row0 + c0, db_row0, mask_width, k, ic, sc);
    else launch_gist_fill(st, db->flags, mc, 1);
    launch_gist_compact(st, db->flags, mc, db->list, db->cnt);
    for (int off = 0; off < mc; off += db->xcap) {
      const int cap = std::min(db->xcap, mc - off);
      K::launch_xdist(st, db, qc, n, off, cap, q_row0 + c0, db_row0, mask_width);
      launch_gist_xselect(st, db->xrows, (size_t)db->max_sigs, n, db->list, db->cnt, off, cap, db_row0, k, ic, sc);
    }
  }
  PR_CHECK_HIP(ctx, hipGetLastError());
  remember(K::kind, ctx, db, m);
  return PR_OK;
}

template <class K>
int match_topk_dev(pr_ctx* ctx, const typename K::Db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0, int32_t mask_width,
                   int32_t k, int32_t* idx, double* score) {
  if (!ctx) return PR_EINVAL;
  if (!db || m < 0 || k < 1 || k > 128 || (m > 0 && (!q || !idx || !score)))
    return fail(ctx, PR_EINVAL, "%s_match_topk_dev: bad arguments (m=%d, k=%d; 1 <= k <= 128)", K::prefix, m, k);
  if (m == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(db->device));
  return launch_match<K>(ctx, db, q, m, q_row0, db_row0, mask_width, k, idx, score);
}

template <class K>
int flagged_count(pr_ctx* ctx, int32_t m, int32_t* count) {
  if (!ctx) return PR_EINVAL;
  const LastCall last = last_call(K::kind, ctx);
  if (!count || !last.db || m != last.m)
    return fail(ctx, PR_EINVAL, "%s_flagged_count: m=%d is not the query count of this context's last %s_match_topk_dev (%d)", K::prefix, m,
                K::prefix, last.db ? last.m : -1);
  PR_CHECK_HIP(ctx, hipSetDevice(last.db->device));
  hipStream_t st = ctx_stream(ctx);
  int c = 0;
  PR_CHECK_HIP(ctx, hipMemcpyAsync(&c, last.db->cnt + 1, sizeof(int), hipMemcpyDeviceToHost, st));
  PR_CHECK_HIP(ctx, hipStreamSynchronize(st));
  *count = c;
  return PR_OK;
}

}  // namespace resident
}  // namespace pr
