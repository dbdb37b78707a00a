// delight_match.cpp — host side of the two-stage exact DELIGHT matcher (delight_match.hip): what the kind adds to the two-stage database
// of resident_match.hpp (fp32 image, empty-bin masks, coarse-exact flags, its slab geometry and launches) and the pr_delight_* entry points.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "resident_match.hpp"

namespace rm = pr::resident;
using pr::fail;
using rm::MAX_CAND;
using rm::MAX_SLABS;
using rm::QCAP;

struct pr_delight_db : rm::Db {                // raw: [max_sigs][16][256]
  float* img = nullptr;                        // [max_sigs][16][256] fp32 image (zero for a row that is not coarse-exact)
  unsigned* mask = nullptr;                    // [max_sigs][128] empty-bin masks in the matcher's lane layout
  int* ok = nullptr;                           // [max_sigs] coarse-exact flags
  unsigned* stat = nullptr;                    // [1] rows that are not coarse-exact
  float* qimg = nullptr;                       // scratch of one chunk: query image, masks, flags, candidate keys
  unsigned* qmask = nullptr;
  int* qok = nullptr;
  float* ckey = nullptr;
};

namespace {

constexpr int SIG = 4096;                      // doubles per signature

struct Delight {
  using Db = pr_delight_db;
  static constexpr rm::Kind kind = rm::DELIGHT;
  static constexpr const char *prefix = "pr_delight", *unit = "signatures";

  static size_t sig_doubles(const Db*) { return SIG; }

  static hipError_t reset(hipStream_t st, Db* db) { return hipMemsetAsync(db->stat, 0, 4, st); }

  static void pack(hipStream_t st, Db* db, const double* dst, int32_t n_new) {
    pr::launch_delight_dpack(st, dst, n_new, db->count, db->img, db->mask, db->ok, db->stat);
  }

  static bool coarse(const Db*, int n, int) { return n > 0; }

  static void launch_coarse(hipStream_t st, const Db* db, const double* qc, int mc, int n, int C, int32_t q_row0, int32_t db_row0,
                            int32_t mask_width, int32_t k, int32_t* ic, double* sc) {
    const int qb = (mc + 3) / 4;
    int S = (2048 + qb - 1) / qb;                           // delight.hip: >= 4 rounds of 2 workgroups per CU
    S = std::min(S, std::min(MAX_CAND / C, MAX_SLABS));
    S = std::max(1, std::min(S, (n + 7) / 8));              // >= 8 entries per workgroup
    pr::launch_delight_dpack(st, qc, mc, 0, db->qimg, db->qmask, db->qok, nullptr);
    pr::launch_delight_coarse(st, db->qimg, mc, db->img, db->mask, n, S, C, q_row0, db_row0, mask_width, db->cand, db->ckey, db->wout);
    pr::launch_delight_rerank(st, qc, db->raw, mc, S, C, db->cand, db->ckey, db->wout, db->qok, db->stat, db_row0, k, ic, sc, db->flags);
  }

  static void launch_xdist(hipStream_t st, const Db* db, const double* qc, int n, int off, int cap, int32_t q_row0, int32_t db_row0,
                           int32_t mask_width) {
    pr::launch_delight_xdist(st, qc, db->raw, n, db->list, db->cnt, off, 0, cap, db->xrows, (size_t)db->max_sigs, q_row0, db_row0, mask_width);
  }
};

int create_db(pr_ctx* ctx, int32_t max_sigs, int32_t qcap, pr_delight_db** out) {
  if (!ctx) return PR_EINVAL;
  if (!out || max_sigs < 1 || max_sigs > PR_MAX_SIGS) return fail(ctx, PR_EINVAL, "pr_delight_db_create: bad arguments (max_sigs=%d)", max_sigs);
  return rm::create<Delight>(ctx, max_sigs, qcap, "PR_DELIGHT_EXACT", out, [&](pr_delight_db* db, rm::Alloc& A) {
    A(db->img, (size_t)max_sigs * SIG * 4);
    A(db->mask, (size_t)max_sigs * 128 * 4);
    A(db->ok, (size_t)max_sigs * 4);
    A(db->stat, 4);
    A(db->qimg, (size_t)db->qcap * SIG * 4);
    A(db->qmask, (size_t)db->qcap * 128 * 4);
    A(db->qok, (size_t)db->qcap * 4);
    A(db->ckey, (size_t)db->qcap * MAX_CAND * 4);
    A.zero(db->stat, 4);
  });
}

}  // namespace

extern "C" {

int pr_delight_db_create(pr_ctx* ctx, int32_t max_sigs, pr_delight_db** out) { return create_db(ctx, max_sigs, QCAP, out); }
void pr_delight_db_destroy(pr_ctx* ctx, pr_delight_db* db) { rm::destroy(ctx, db); }
int32_t pr_delight_db_count(const pr_delight_db* db) { return db ? db->count : 0; }
int64_t pr_delight_db_bytes(const pr_delight_db* db) { return db ? db->bytes : 0; }
void pr_delight_db_set_exact(pr_delight_db* db, int on) { if (db) db->exact = on != 0; }

int pr_delight_db_set(pr_ctx* ctx, pr_delight_db* db, const double* rows, int where, int32_t n) {
  return rm::set<Delight>(ctx, db, rows, where, n);
}

int pr_delight_db_append(pr_ctx* ctx, pr_delight_db* db, const double* rows, int where, int32_t n_new) {
  return rm::append<Delight>(ctx, db, rows, where, n_new);
}

int pr_delight_match_topk_dev(pr_ctx* ctx, const pr_delight_db* db, const double* q, int32_t m, int32_t q_row0, int32_t db_row0,
                              int32_t mask_width, int32_t k, int32_t* idx, double* score) {
  return rm::match_topk_dev<Delight>(ctx, db, q, m, q_row0, db_row0, mask_width, k, idx, score);
}

int pr_delight_flagged_count(pr_ctx* ctx, int32_t m, int32_t* count) { return rm::flagged_count<Delight>(ctx, m, count); }

int pr_delight_match_topk_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, int32_t mask_width, int32_t k, int32_t* idx,
                              double* score) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || k < 1 || k > 128 || (m > 0 && (!h1 || !idx || !score)) || (n > 0 && !h2) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_delight_match_topk_f64: bad arguments (m=%d, n=%d, k=%d; 1 <= k <= 128)", m, n, k);
  if (m == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_delight_db* db = nullptr;
  if (int rc = create_db(ctx, std::max(n, 1), std::min(m, QCAP), &db)) return rc;
  int rc = pr_delight_db_set(ctx, db, h2, PR_HOST, n);
  if (rc == PR_OK)
    rc = rm::host_topk(ctx, "pr_delight_match_topk_f64", h1, (size_t)m * SIG * sizeof(double), m, k, idx, score,
                       [&](const double* dq, int32_t* di, double* ds) { return rm::launch_match<Delight>(ctx, db, dq, m, 0, 0, mask_width, k, di, ds); });
  pr_delight_db_destroy(ctx, db);
  return rc;
}

int pr_delight_distance_f64(pr_ctx* ctx, const double* h1, int32_t m, const double* h2, int32_t n, double* dist) {
  if (!ctx) return PR_EINVAL;
  if (m < 0 || n < 0 || (m > 0 && !h1) || (n > 0 && !h2) || (m > 0 && n > 0 && !dist) || m > PR_MAX_SIGS || n > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_delight_distance_f64: bad arguments (m=%d, n=%d)", m, n);
  if (m == 0 || n == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  return rm::host_distance(ctx, "pr_delight_distance_f64", h1, m, h2, n, SIG * sizeof(double), 1 << 15 /* slots of one launch */, dist,
                           [&](hipStream_t st, const double* dq, const double* db, int off, int cap, double* out) {
                             pr::launch_delight_xdist(st, dq, db, n, nullptr, nullptr, off, cap, cap, out, (size_t)n, 0, 0, 0);
                           });
}

}  // extern "C"
