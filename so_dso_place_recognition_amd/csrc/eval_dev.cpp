// eval_dev.cpp — host side of the device evaluation (eval.hip): launch geometry, the context's grow-only scratch, the stream-ordered
// entry points pr_ground_truth_pairs_dev / pr_precision_recall_dev / pr_trapz_dev and their host-buffer forms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/place_recognition.h"
#include "host_common.hpp"
#include "kernels.hpp"

namespace {

struct Buf { void* p = nullptr; size_t cap = 0; };

struct EvalState {
  int split_mode = 0;            // pr_set_eval_path: 0 = by shape, 1 = one launch over all of gt2, 2 = per-split partials + combine
  int rq_mode = 0;               // 0 = by shape, 1 | 4 queries per lane
  Buf part_d, part_j, min_d, min_j, loc, bsum, cnt, rank, bidx, cls, prec, rec, term;
};

using pr::fail;

EvalState* state(pr_ctx* ctx) {
  void*& slot = pr::ctx_eval(ctx);
  if (!slot) slot = new EvalState;
  return static_cast<EvalState*>(slot);
}

// grow-only: a call whose shapes an earlier call covered allocates nothing (and can be captured)
int grow(pr_ctx* ctx, Buf& b, size_t bytes) {
  bytes = std::max<size_t>(bytes, 64);
  if (b.cap >= bytes) return PR_OK;
  if (b.p) {
    PR_CHECK_HIP(ctx, hipStreamSynchronize(pr::ctx_stream(ctx)));
    (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
  }
  PR_CHECK_HIP(ctx, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return PR_OK;
}

template <class T> T* ptr(const Buf& b) { return static_cast<T*>(b.p); }

struct GtGeometry { int rq, nsplit, chunk; bool direct; };

// 256 rq queries per workgroup; gt2 cut into nsplit ranges of whole tiles until about four workgroups per CU are in flight
GtGeometry gt_geometry(const EvalState* S, int m, int n, int cols) {
  GtGeometry g;
  g.rq = S->rq_mode ? S->rq_mode : (m > 16384 ? 4 : 1);
  if (cols > 3) g.rq = 1;
  const int qb = std::max(1, (m + 256 * g.rq - 1) / (256 * g.rq)), tiles = std::max(1, (n + pr::EVAL_TILE - 1) / pr::EVAL_TILE);
  int split = std::min(tiles, std::max(1, (1024 + qb - 1) / qb));
  if (S->split_mode == 1) split = 1;
  if (S->split_mode == 2) split = std::min(tiles, std::max(2, split));
  const int per = (tiles + split - 1) / split;
  g.nsplit = (tiles + per - 1) / per;
  g.chunk = per * pr::EVAL_TILE;
  g.direct = S->split_mode == 2 ? false : g.nsplit == 1;
  return g;
}

int clamp_mask(int32_t mask_width) { return mask_width < 0 ? 0 : mask_width; }

// run_test.m:3-22 on the stream; min_j / min_d may be null (scratch is used), lp_gt / n_gt may be null
int gt_run(pr_ctx* ctx, EvalState* S, const double* gt1, int m, const double* gt2, int n, int cols, double thr, int mw, int32_t* min_j,
           double* min_d, int32_t* lp_gt, int32_t* n_gt) {
  hipStream_t st = pr::ctx_stream(ctx);
  if (!min_d) { if (int rc = grow(ctx, S->min_d, (size_t)m * 8)) return rc; min_d = ptr<double>(S->min_d); }
  if (!min_j) { if (int rc = grow(ctx, S->min_j, (size_t)m * 4)) return rc; min_j = ptr<int32_t>(S->min_j); }
  const GtGeometry g = gt_geometry(S, m, n, cols);
  if (g.direct) {
    pr::launch_eval_gt(st, gt1, m, gt2, n, cols, mw, g.chunk, 1, g.rq, min_d, min_j);
  } else {
    if (int rc = grow(ctx, S->part_d, (size_t)g.nsplit * m * 8)) return rc;
    if (int rc = grow(ctx, S->part_j, (size_t)g.nsplit * m * 4)) return rc;
    pr::launch_eval_gt(st, gt1, m, gt2, n, cols, mw, g.chunk, g.nsplit, g.rq, ptr<double>(S->part_d), ptr<int>(S->part_j));
    pr::launch_eval_gt_combine(st, ptr<double>(S->part_d), ptr<int>(S->part_j), m, g.nsplit, min_d, min_j);
  }
  if (lp_gt || n_gt) {
    const size_t nb = ((size_t)m + pr::EVAL_SCAN - 1) / pr::EVAL_SCAN;
    if (int rc = grow(ctx, S->loc, (size_t)m * 4)) return rc;
    if (int rc = grow(ctx, S->bsum, (2 * nb + 2) * 4)) return rc;
    pr::launch_eval_gt_pairs(st, min_d, min_j, m, thr, ptr<int>(S->loc), ptr<int>(S->bsum), lp_gt, n_gt);
  }
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int check_shapes(pr_ctx* ctx, const char* fn, int32_t m, int32_t n, int32_t cols) {
  if (m < 0 || n < 0) return fail(ctx, PR_EINVAL, "%s: negative size (m=%d, n=%d)", fn, m, n);
  if (cols < 1 || cols > pr::EVAL_MAX_COLS) return fail(ctx, PR_EINVAL, "%s: cols=%d outside 1..%d", fn, cols, pr::EVAL_MAX_COLS);
  if (m > PR_MAX_SIGS || n > PR_MAX_SIGS) return fail(ctx, PR_EINVAL, "%s: more than %d rows (m=%d, n=%d)", fn, PR_MAX_SIGS, m, n);
  return PR_OK;
}

// device copies of host buffers for the two host forms: freed together
struct Staging {
  std::vector<void*> all;
  hipError_t e = hipSuccess;
  void* get(size_t bytes) {
    void* p = nullptr;
    if (e == hipSuccess) e = hipMalloc(&p, std::max<size_t>(bytes, 16));
    if (p) all.push_back(p);
    return p;
  }
  void* up(const void* h, size_t bytes, hipStream_t st) {
    void* p = get(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, st);
    return p;
  }
  void down(void* h, const void* d, size_t bytes, hipStream_t st) {
    if (e == hipSuccess && h && bytes) e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st);
  }
  ~Staging() { for (void* p : all) (void)hipFree(p); }
};

}  // namespace

namespace pr {
void eval_release(void* p) {
  if (!p) return;
  EvalState* S = static_cast<EvalState*>(p);
  for (Buf* b : {&S->part_d, &S->part_j, &S->min_d, &S->min_j, &S->loc, &S->bsum, &S->cnt, &S->rank, &S->bidx, &S->cls, &S->prec, &S->rec,
                 &S->term})
    if (b->p) (void)hipFree(b->p);
  delete S;
}
}  // namespace pr

extern "C" {

int32_t pr_eval_tile_rows(void) { return pr::EVAL_TILE; }

int pr_set_eval_path(pr_ctx* ctx, int split, int queries_per_lane) {
  if (!ctx) return PR_EINVAL;
  if (split < 0 || split > 2 || (queries_per_lane != 0 && queries_per_lane != 1 && queries_per_lane != 4))
    return fail(ctx, PR_EINVAL, "pr_set_eval_path: split=%d (0..2), queries_per_lane=%d (0, 1 or 4)", split, queries_per_lane);
  EvalState* S = state(ctx);
  S->split_mode = split;
  S->rq_mode = queries_per_lane;
  return PR_OK;
}

int pr_ground_truth_pairs_dev(pr_ctx* ctx, const double* d_gt1, int32_t m, const double* d_gt2, int32_t n, int32_t cols, double loop_diff,
                              int32_t mask_width, int32_t* d_min_j, double* d_min_d, int32_t* d_lp_gt, int32_t* d_n_gt) {
  if (int rc = check_shapes(ctx, "pr_ground_truth_pairs_dev", m, n, cols)) return rc;
  if ((m > 0 && !d_gt1) || (m > 0 && n > 0 && !d_gt2)) return fail(ctx, PR_EINVAL, "pr_ground_truth_pairs_dev: gt1 / gt2 is NULL");
  if (!ctx) return fail(ctx, PR_EINVAL, "pr_ground_truth_pairs_dev: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  return gt_run(ctx, state(ctx), d_gt1, m, d_gt2, n, cols, loop_diff * loop_diff, clamp_mask(mask_width), d_min_j, d_min_d, d_lp_gt, d_n_gt);
}

int pr_precision_recall_dev(pr_ctx* ctx, const double* d_diff_v, const int32_t* d_diff_idx, int32_t ld, int32_t m, const double* d_gt1,
                            const double* d_gt2, int32_t n, int32_t cols, double loop_diff, int32_t mask_width, void* d_scalars,
                            int32_t* d_lp_gt, int32_t* d_lp_detected, double* d_precision, double* d_recall) {
  if (int rc = check_shapes(ctx, "pr_precision_recall_dev", m, n, cols)) return rc;
  if (ld < 1) return fail(ctx, PR_EINVAL, "pr_precision_recall_dev: ld=%d < 1", ld);
  if (!d_scalars || (m > 0 && (!d_diff_v || !d_diff_idx || !d_gt1)) || (m > 0 && n > 0 && !d_gt2))
    return fail(ctx, PR_EINVAL, "pr_precision_recall_dev: a required pointer is NULL");
  if (!ctx) return fail(ctx, PR_EINVAL, "pr_precision_recall_dev: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  EvalState* S = state(ctx);
  pr::EvalScalars* scal = static_cast<pr::EvalScalars*>(d_scalars);
  const double thr = loop_diff * loop_diff;
  const size_t nb = ((size_t)m + pr::EVAL_SCAN - 1) / pr::EVAL_SCAN, mi = (size_t)m * 4, md = (size_t)m * 8;
  for (Buf* b : {&S->cnt, &S->rank, &S->bidx, &S->cls, &S->loc}) if (int rc = grow(ctx, *b, mi)) return rc;
  if (int rc = grow(ctx, S->bsum, (2 * nb + 2) * 4)) return rc;
  if (int rc = grow(ctx, S->term, md)) return rc;
  if (!d_precision) { if (int rc = grow(ctx, S->prec, md)) return rc; d_precision = ptr<double>(S->prec); }
  if (!d_recall) { if (int rc = grow(ctx, S->rec, md)) return rc; d_recall = ptr<double>(S->rec); }
  if (int rc = gt_run(ctx, S, d_gt1, m, d_gt2, n, cols, thr, clamp_mask(mask_width), nullptr, nullptr, d_lp_gt, &scal->n_gt)) return rc;
  pr::launch_eval_sweep(pr::ctx_stream(ctx), d_diff_v, d_diff_idx, ld, m, d_gt1, d_gt2, n, cols, thr, ptr<int>(S->cnt), ptr<int>(S->rank),
                        ptr<int>(S->bidx), ptr<int>(S->cls), ptr<int>(S->loc), ptr<int>(S->bsum), d_precision, d_recall, ptr<double>(S->term),
                        scal, d_lp_detected);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_trapz_dev(pr_ctx* ctx, const double* d_recall, const double* d_precision, int32_t m, double* d_auc) {
  if (m < 0 || m > PR_MAX_SIGS) return fail(ctx, PR_EINVAL, "pr_trapz_dev: m=%d outside 0..%d", m, PR_MAX_SIGS);
  if (!d_auc || (m > 0 && (!d_recall || !d_precision))) return fail(ctx, PR_EINVAL, "pr_trapz_dev: a required pointer is NULL");
  if (!ctx) return fail(ctx, PR_EINVAL, "pr_trapz_dev: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  EvalState* S = state(ctx);
  if (int rc = grow(ctx, S->term, (size_t)m * 8)) return rc;
  pr::launch_eval_trapz(pr::ctx_stream(ctx), d_recall, d_precision, m, ptr<double>(S->term), d_auc);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_ground_truth_pairs(pr_ctx* ctx, const double* gt1, int32_t m, const double* gt2, int32_t n, int32_t cols, double loop_diff,
                          int32_t mask_width, int32_t* min_j, double* min_d, int32_t* lp_gt, int32_t* n_gt) {
  if (int rc = check_shapes(ctx, "pr_ground_truth_pairs", m, n, cols)) return rc;
  if ((m > 0 && !gt1) || (n > 0 && !gt2)) return fail(ctx, PR_EINVAL, "pr_ground_truth_pairs: gt1 / gt2 is NULL");
  if (!ctx) return fail(ctx, PR_EINVAL, "pr_ground_truth_pairs: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  Staging s;
  const size_t mc = (size_t)m * cols * 8, nc = (size_t)n * cols * 8;
  double* dg1 = static_cast<double*>(s.up(gt1, mc, st));
  double* dg2 = static_cast<double*>(s.up(gt2, nc, st));
  int32_t* dj = static_cast<int32_t*>(s.get((size_t)m * 4));
  double* dd = static_cast<double*>(s.get((size_t)m * 8));
  int32_t* dl = static_cast<int32_t*>(s.get((size_t)m * 8));
  int32_t* dn = static_cast<int32_t*>(s.get(4));
  int rc = PR_OK;
  if (s.e == hipSuccess) rc = pr_ground_truth_pairs_dev(ctx, dg1, m, dg2, n, cols, loop_diff, mask_width, dj, dd, dl, dn);
  if (rc == PR_OK) {
    s.down(min_j, dj, (size_t)m * 4, st);
    s.down(min_d, dd, (size_t)m * 8, st);
    s.down(lp_gt, dl, (size_t)m * 8, st);     // (the first n_gt pairs are defined)
    s.down(n_gt, dn, 4, st);
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (s.e == hipSuccess) s.e = es;
  if (rc == PR_OK && s.e != hipSuccess) rc = fail(ctx, s.e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_ground_truth_pairs: %s", hipGetErrorString(s.e));
  return rc;
}

int pr_precision_recall_gpu(pr_ctx* ctx, const double* diff_v, const int32_t* diff_idx, int32_t m, const double* gt1, const double* gt2,
                            int32_t n, int32_t cols, double loop_diff, int32_t mask_width, double* auc, double* top_recall, int32_t* lp_gt,
                            int32_t* n_gt, int32_t* lp_detected, int32_t* n_detected, double* precision, double* recall) {
  if (int rc = check_shapes(ctx, "pr_precision_recall_gpu", m, n, cols)) return rc;
  if ((m > 0 && (!diff_v || !diff_idx || !gt1)) || (n > 0 && !gt2) || !auc || !top_recall)
    return fail(ctx, PR_EINVAL, "pr_precision_recall_gpu: a required pointer is NULL");
  if (!ctx) return fail(ctx, PR_EINVAL, "pr_precision_recall_gpu: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  Staging s;
  double* dv = static_cast<double*>(s.up(diff_v, (size_t)m * 8, st));
  int32_t* di = static_cast<int32_t*>(s.up(diff_idx, (size_t)m * 4, st));
  double* dg1 = static_cast<double*>(s.up(gt1, (size_t)m * cols * 8, st));
  double* dg2 = static_cast<double*>(s.up(gt2, (size_t)n * cols * 8, st));
  void* dsc = s.get(sizeof(pr::EvalScalars));
  int32_t* dlg = static_cast<int32_t*>(s.get((size_t)m * 8));
  int32_t* dld = static_cast<int32_t*>(s.get((size_t)m * 8));
  double* dp = static_cast<double*>(s.get((size_t)m * 8));
  double* dr = static_cast<double*>(s.get((size_t)m * 8));
  int rc = PR_OK;
  if (s.e == hipSuccess)
    rc = pr_precision_recall_dev(ctx, dv, di, 1, m, dg1, dg2, n, cols, loop_diff, mask_width, dsc, dlg, dld, dp, dr);
  pr::EvalScalars sc{0.0, 0.0, 0, 0};
  if (rc == PR_OK) {
    s.down(&sc, dsc, sizeof sc, st);
    s.down(lp_gt, dlg, (size_t)m * 8, st);
    s.down(lp_detected, dld, (size_t)m * 8, st);   // (the first n_detected pairs are defined)
    s.down(precision, dp, (size_t)m * 8, st);
    s.down(recall, dr, (size_t)m * 8, st);
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (s.e == hipSuccess) s.e = es;
  if (rc == PR_OK && s.e != hipSuccess) rc = fail(ctx, s.e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_precision_recall_gpu: %s", hipGetErrorString(s.e));
  if (rc == PR_OK) {
    *auc = sc.auc;
    *top_recall = sc.top_recall;
    if (n_gt) *n_gt = sc.n_gt;
    if (n_detected) *n_detected = sc.n_detected;
  }
  return rc;
}

}  // extern "C"
