// gist_match.cpp — host side of the two-stage exact GIST matcher (gist_match.hip): what the kind adds to the two-stage database of
// resident_match.hpp (f16 image, norms, the centring vector, its slab geometry and launches) and the pr_gist_* entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "resident_match.hpp"

namespace rm = pr::resident;
using pr::fail;
using rm::MAX_CAND;
using rm::MAX_SLABS;
using rm::QCAP;

struct pr_gist_db : rm::Db {                   // raw: [max_sigs][cols]
  int32_t cols = 0, KP = 0, KS = 0;
  bool mu_set = false, centre = true;
  void* img = nullptr;                         // f16 operand image, tiles of 32 rows
  float *nd = nullptr, *rs = nullptr;          // [max_sigs] |a'|^2, residual norm
  unsigned* stat = nullptr;                    // [2] max nd, max rs (float bits)
  double* mu = nullptr;                        // [cols] the vector the pack subtracts
  void* qimg = nullptr;                        // scratch of one chunk: query image, norms
  float *qn = nullptr, *qr = nullptr;
};

namespace {

constexpr int MEAN_ROWS = 1024;
constexpr size_t MAX_LDS = 160 * 1024;

struct Gist {
  using Db = pr_gist_db;
  static constexpr rm::Kind kind = rm::GIST;
  static constexpr const char *prefix = "pr_gist", *unit = "rows";

  static size_t sig_doubles(const Db* db) { return (size_t)db->cols; }

  static hipError_t reset(hipStream_t st, Db* db) {
    db->mu_set = false;
    hipError_t e = hipMemsetAsync(db->stat, 0, 8, st);
    return e != hipSuccess ? e : hipMemsetAsync(db->mu, 0, (size_t)db->cols * 8, st);
  }

  static void pack(hipStream_t st, Db* db, const double* dst, int32_t n_new) {
    if (!db->mu_set) {         // fixed by the first rows the database receives after a set; never re-derived
      if (db->centre) pr::launch_gist_mean(st, dst, std::min(n_new, MEAN_ROWS), db->cols, db->mu);
      db->mu_set = true;
    }
    pr::launch_gist_pack(st, dst, n_new, db->cols, db->KS, db->mu, db->count, db->img, db->nd, db->rs, db->stat);
  }

  static bool coarse(const Db* db, int, int C) { return pr::gist_coarse_lds_bytes(db->KS, C) <= MAX_LDS; }

  static void launch_coarse(hipStream_t st, const Db* db, const double* qc, int mc, int n, int C, int32_t q_row0, int32_t db_row0,
                            int32_t mask_width, int32_t k, int32_t* ic, double* sc) {
    const int qtiles = (mc + 31) / 32, DT = (n + 31) / 32;
    int S = std::max(4, (1536 + qtiles - 1) / qtiles);
    S = std::min(S, std::min(MAX_CAND / C, MAX_SLABS));
    S = std::max(1, std::min(S, DT));
    pr::launch_gist_pack(st, qc, mc, db->cols, db->KS, db->mu, 0, db->qimg, db->qn, db->qr, nullptr);
    pr::launch_gist_coarse(st, db->qimg, db->qn, mc, db->img, db->nd, n, db->KS, S, C, q_row0, db_row0, mask_width, db->cand, db->wout);
    pr::launch_gist_rerank(st, qc, db->raw, db->cols, db->KP, mc, S, C, db->cand, db->wout, db->qn, db->qr, db->stat, db_row0, k, ic, sc,
                           db->flags);
  }

  static void launch_xdist(hipStream_t st, const Db* db, const double* qc, int n, int off, int cap, int32_t q_row0, int32_t db_row0,
                           int32_t mask_width) {
    pr::launch_gist_xdist(st, qc, db->raw, db->cols, n, db->list, db->cnt, off, 0, cap, db->xrows, (size_t)db->max_sigs, q_row0, db_row0,
                          mask_width);
  }
};

int create_db(pr_ctx* ctx, int32_t max_sigs, int32_t cols, int32_t qcap, pr_gist_db** out) {
  if (!ctx) return PR_EINVAL;
  if (!out || max_sigs < 1 || max_sigs > PR_MAX_SIGS || cols < 1 || cols > (1 << 20))
    return fail(ctx, PR_EINVAL, "pr_gist_db_create: bad arguments (max_sigs=%d, cols=%d)", max_sigs, cols);
  return rm::create<Gist>(ctx, max_sigs, qcap, "PR_GIST_EXACT", out, [&](pr_gist_db* db, rm::Alloc& A) {
    db->cols = cols;
    db->KP = ((cols + 63) / 64) * 64; db->KS = db->KP / 16;
    { const char* s = getenv("PR_GIST_CENTRE"); db->centre = !(s && *s && atoi(s) == 0); }   // PR_GIST_CENTRE=0: mu = 0 (A/B runs of the bound)
    const size_t tiles = ((size_t)max_sigs + 31) / 32, qtiles = ((size_t)db->qcap + 31) / 32, tile_bytes = (size_t)db->KP * 64;
    A(db->img, tiles * tile_bytes);
    A(db->nd, tiles * 32 * 4); A(db->rs, tiles * 32 * 4);
    A(db->stat, 8); A(db->mu, (size_t)cols * 8);
    A(db->qimg, qtiles * tile_bytes);
    A(db->qn, qtiles * 32 * 4); A(db->qr, qtiles * 32 * 4);
    A.zero(db->stat, 8);
    A.zero(db->mu, (size_t)cols * 8);
  });
}

}  // namespace

extern "C" {

int pr_gist_db_create(pr_ctx* ctx, int32_t max_sigs, int32_t cols, pr_gist_db** out) { return create_db(ctx, max_sigs, cols, QCAP, out); }
void pr_gist_db_destroy(pr_ctx* ctx, pr_gist_db* db) { rm::destroy(ctx, db); }
int32_t pr_gist_db_count(const pr_gist_db* db) { return db ? db->count : 0; }
int64_t pr_gist_db_bytes(const pr_gist_db* db) { return db ? db->bytes : 0; }
void pr_gist_db_set_exact(pr_gist_db* db, int on) { if (db) db->exact = on != 0; }

int pr_gist_db_set(pr_ctx* ctx, pr_gist_db* db, const double* rows, int where, int32_t n) { return rm::set<Gist>(ctx, db, rows, where, n); }

int pr_gist_db_append(pr_ctx* ctx, pr_gist_db* db, const double* rows, int where, int32_t n_new) {
  return rm::append<Gist>(ctx, db, rows, where, n_new);
}

int pr_gist_match_topk_dev(pr_ctx* ctx, const pr_gist_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0, int32_t mask_width,
                           int32_t k, int32_t* idx, double* score) {
  return rm::match_topk_dev<Gist>(ctx, db, q, m, q_row0, db_row0, mask_width, k, idx, score);
}

int pr_gist_flagged_count(pr_ctx* ctx, int32_t m, int32_t* count) { return rm::flagged_count<Gist>(ctx, m, count); }

int pr_gist_match_topk_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, int32_t mask_width, int32_t k,
                           int32_t* idx, double* score) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || cols < 1 || k < 1 || k > 128 || (m > 0 && (!h1 || !idx || !score)) || (n > 0 && !h2) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_gist_match_topk_f64: bad arguments (m=%d, n=%d, cols=%d, k=%d; 1 <= k <= 128)", m, n, cols, k);
  if (m == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_gist_db* db = nullptr;
  if (int rc = create_db(ctx, std::max(n, 1), cols, std::min(m, QCAP), &db)) return rc;
  int rc = pr_gist_db_set(ctx, db, h2, PR_HOST, n);
  if (rc == PR_OK)
    rc = rm::host_topk(ctx, "pr_gist_match_topk_f64", h1, (size_t)m * cols * sizeof(double), m, k, idx, score,
                       [&](const double* dq, int32_t* di, double* ds) { return rm::launch_match<Gist>(ctx, db, dq, m, 0, 0, mask_width, k, di, ds); });
  pr_gist_db_destroy(ctx, db);
  return rc;
}

int pr_gist_distance_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t cols, double* dist) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || cols < 1 || (m > 0 && !h1) || (n > 0 && !h2) || (m > 0 && n > 0 && !dist) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_gist_distance_f64: bad arguments (m=%d, n=%d, cols=%d)", m, n, cols);
  if (m == 0 || n == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  return rm::host_distance(ctx, "pr_gist_distance_f64", h1, m, h2, n, (size_t)cols * sizeof(double), 1 << 16 /* slots of one launch */, dist,
                           [&](hipStream_t st, const double* dq, const double* db, int off, int cap, double* out) {
                             pr::launch_gist_xdist(st, dq, db, cols, n, nullptr, nullptr, off, cap, cap, out, (size_t)n, 0, 0, 0);
                           });
}

}  // extern "C"
