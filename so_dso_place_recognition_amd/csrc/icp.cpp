// icp.cpp — host side of the ICP refinement (icp.hip): launch geometry, the context's grow-only scratch, the stream-ordered entry points
// pr_icp_nn_dev / pr_icp_nn_radius_dev / pr_icp_pairs_dev and their host-buffer forms, the search mode (pr_set_icp_search) and the plan and
// scratch of the uniform grid (icp_grid.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/place_recognition.h"
#include "host_common.hpp"
#include "kernels.hpp"

static_assert(sizeof(pr::IcpStats) == sizeof(pr_icp_stats), "stats record");
static_assert(PR_ICP_SEARCH_BRUTE == 0 && PR_ICP_SEARCH_GRID == 1, "search modes");
static_assert(pr::ICP_CONVERGED == PR_ICP_CONVERGED && pr::ICP_MAX_ITER == PR_ICP_MAX_ITER && pr::ICP_TOO_FEW == PR_ICP_TOO_FEW &&
              pr::ICP_DEGENERATE == PR_ICP_DEGENERATE && pr::ICP_NO_PAIR == PR_ICP_NO_PAIR, "status codes");

namespace {

struct Buf { void* p = nullptr; size_t cap = 0; };

struct IcpState {
  int split_mode = 0;            // pr_set_icp_path: 0 = by shape, 1 = every workgroup scans the whole target, 2 = split target + combine
  int search = PR_ICP_SEARCH_BRUTE;   // pr_set_icp_search
  Buf slot_d, slot_j, nn_d, nn_j, part, done, prev;
  Buf g_box, g_ends, g_sorted;   // the grid: a box per pair slot, cells words and max_dst indices per pair slot
};

constexpr size_t GRID_CELL_BUDGET = (size_t)256 << 20;   // bytes of cell words a call may hold

using pr::fail;

IcpState* state(pr_ctx* ctx) {
  void*& slot = pr::ctx_icp(ctx);
  if (!slot) slot = new IcpState;
  return static_cast<IcpState*>(slot);
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

// 256 rq source points per workgroup: 4 per lane once one per lane would give more than 4096 workgroups; the target cut into ranges of
// whole tiles until about four workgroups per CU exist
pr::IcpGeometry geometry(const IcpState* S, int c, int max_src, int max_dst) {
  pr::IcpGeometry g;
  const long long b1 = (long long)std::max(c, 1) * std::max(1, (max_src + 255) / 256);
  g.rq = b1 > 4096 ? 4 : 1;
  const long long blocks = (long long)std::max(c, 1) * std::max(1, (max_src + 256 * g.rq - 1) / (256 * g.rq));
  const int tiles = std::max(1, (max_dst + pr::ICP_TILE - 1) / pr::ICP_TILE);
  int split = (int)std::min<long long>(tiles, std::max<long long>(1, (1024 + blocks - 1) / blocks));
  if (S->split_mode == 1) split = 1;
  if (S->split_mode == 2) split = std::min(tiles, std::max(2, split));
  const int per = (tiles + split - 1) / split;
  g.nsplit = (tiles + per - 1) / per;
  g.ld = std::max(max_src, 1);
  g.chunk_pts = g.nsplit > 1 ? 256 : 256 * g.rq;
  g.nchunks = std::max(1, (max_src + g.chunk_pts - 1) / g.chunk_pts);
  return g;
}

// the grid's plan: cells per pair slot = the power of two >= 2 max_dst, halved until c slots fit the budget (never below 8); the axes get
// G = floor(cbrt(cells)) - 1 cells from the host, so that the device's n <= G + 1 per axis fits
void grid_plan(int c, int max_dst, int* cells, int* G) {
  size_t n = 8;
  while (n < 2 * (size_t)std::max(max_dst, 1)) n <<= 1;
  while (n > 8 && (size_t)std::max(c, 1) * n * sizeof(int) > GRID_CELL_BUDGET) n >>= 1;
  int gc = 2;
  while ((size_t)(gc + 1) * (gc + 1) * (gc + 1) <= n) gc++;
  *cells = (int)n;
  *G = gc - 1;
}

int check_sets(pr_ctx* ctx, const char* fn, const void* xyz_q, const void* offs_q, int32_t Nq, const void* xyz_d, const void* offs_d, int32_t Nd,
               const void* pair_src, const void* pair_dst, int32_t c, int64_t max_src, int64_t max_dst, bool need_pairs = true) {
  if (Nq < 0 || Nd < 0 || c < 0 || max_src < 0 || max_dst < 0)
    return fail(ctx, PR_EINVAL, "%s: negative size (Nq=%d, Nd=%d, c=%d, max_src_pts=%lld, max_dst_pts=%lld)", fn, Nq, Nd, c, (long long)max_src,
                (long long)max_dst);
  if (c > 65535 || max_src > (1 << 26) || max_dst > (1 << 26))
    return fail(ctx, PR_EINVAL, "%s: more than 65535 pairs or 2^26 points per cloud (c=%d, max_src_pts=%lld, max_dst_pts=%lld)", fn, c,
                (long long)max_src, (long long)max_dst);
  if (!offs_q || !offs_d || (c > 0 && need_pairs && (!pair_src || !pair_dst)) || (c > 0 && max_src > 0 && !xyz_q) || (c > 0 && max_dst > 0 && !xyz_d))
    return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  return PR_OK;
}

int check_params(pr_ctx* ctx, const char* fn, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers) {
  if (max_iter < 0) return fail(ctx, PR_EINVAL, "%s: max_iter=%d < 0", fn, max_iter);
  if (!(max_corr > 0.0) || !std::isfinite(max_corr)) return fail(ctx, PR_EINVAL, "%s: max_corr=%g must be positive and finite", fn, max_corr);
  if (min_inliers < 3) return fail(ctx, PR_EINVAL, "%s: min_inliers=%d < 3", fn, min_inliers);
  if (std::isnan(tol_rmse) || std::isnan(tol_fitness)) return fail(ctx, PR_EINVAL, "%s: tol_rmse / tol_fitness is NaN", fn);
  return PR_OK;
}

// the grid's scratch for c pair slots (grow-only) and its build on the context's stream
int grid_build(pr_ctx* ctx, IcpState* S, const pr::IcpClouds& A, double max_corr, pr::IcpGrid* gr) {
  grid_plan(A.c, A.max_dst, &gr->cells, &gr->G);
  if (int rc = grow(ctx, S->g_box, (size_t)A.c * sizeof(pr::IcpGridBox))) return rc;
  if (int rc = grow(ctx, S->g_ends, (size_t)A.c * gr->cells * sizeof(int))) return rc;
  if (int rc = grow(ctx, S->g_sorted, (size_t)A.c * std::max(A.max_dst, 1) * sizeof(int))) return rc;
  gr->box = ptr<pr::IcpGridBox>(S->g_box);
  gr->ends = ptr<int>(S->g_ends);
  gr->sorted = ptr<int>(S->g_sorted);
  pr::launch_icp_grid_build(pr::ctx_stream(ctx), A, *gr, max_corr);
  return PR_OK;
}

pr::IcpClouds clouds(const double* xyz_q, const int64_t* offs_q, int32_t Nq, const double* xyz_d, const int64_t* offs_d, int32_t Nd,
                     const int32_t* pair_src, const int32_t* pair_dst, int32_t c, int32_t max_src, int32_t max_dst) {
  return pr::IcpClouds{xyz_q, offs_q, Nq, xyz_d, offs_d, Nd, pair_src, pair_dst, c, max_src, max_dst};
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

// what the host forms learn from the host arrays: offsets ascending from 0 .. , pairs in range, the largest clouds of the pairs, the prefix
int host_shapes(pr_ctx* ctx, const char* fn, const int64_t* offs_q, int32_t Nq, const int64_t* offs_d, int32_t Nd, const int32_t* pair_src,
                const int32_t* pair_dst, int32_t c, int64_t* max_src, int64_t* max_dst, std::vector<int64_t>* prefix) {
  for (int32_t i = 0; i < Nq; i++) if (offs_q[i + 1] < offs_q[i] || offs_q[0] < 0) return fail(ctx, PR_EINVAL, "%s: offs_q is not ascending", fn);
  for (int32_t i = 0; i < Nd; i++) if (offs_d[i + 1] < offs_d[i] || offs_d[0] < 0) return fail(ctx, PR_EINVAL, "%s: offs_d is not ascending", fn);
  *max_src = *max_dst = 0;
  prefix->assign((size_t)c + 1, 0);
  for (int32_t i = 0; i < c; i++) {
    const int32_t s = pair_src[i], d = pair_dst[i];
    if (s >= Nq || d >= Nd) return fail(ctx, PR_EINVAL, "%s: pair %d = (%d, %d) outside the cloud sets (Nq=%d, Nd=%d)", fn, i, s, d, Nq, Nd);
    int64_t ns = 0;
    if (s >= 0 && d >= 0) {
      ns = offs_q[s + 1] - offs_q[s];
      *max_src = std::max(*max_src, ns);
      *max_dst = std::max(*max_dst, offs_d[d + 1] - offs_d[d]);
    }
    (*prefix)[(size_t)i + 1] = (*prefix)[i] + ns;
  }
  return PR_OK;
}

}  // namespace

namespace pr {
int icp_check_pairs_args(pr_ctx* ctx, const char* fn, const void* xyz_q, const void* offs_q, int32_t Nq, const void* xyz_d, const void* offs_d,
                         int32_t Nd, int32_t c, int64_t max_src, int64_t max_dst, int32_t max_iter, double max_corr, double tol_rmse,
                         double tol_fitness, int32_t min_inliers) {
  if (int rc = check_sets(ctx, fn, xyz_q, offs_q, Nq, xyz_d, offs_d, Nd, nullptr, nullptr, c, max_src, max_dst, /*need_pairs=*/false)) return rc;
  return check_params(ctx, fn, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers);
}

void icp_release(void* p) {
  if (!p) return;
  IcpState* S = static_cast<IcpState*>(p);
  for (Buf* b : {&S->slot_d, &S->slot_j, &S->nn_d, &S->nn_j, &S->part, &S->done, &S->prev, &S->g_box, &S->g_ends, &S->g_sorted})
    if (b->p) (void)hipFree(b->p);
  delete S;
}
}  // namespace pr

extern "C" {

int32_t pr_icp_tile_rows(void) { return pr::ICP_TILE; }

int pr_set_icp_path(pr_ctx* ctx, int split) {
  if (!ctx) return PR_EINVAL;
  if (split < 0 || split > 2) return fail(ctx, PR_EINVAL, "pr_set_icp_path: split=%d (0..2)", split);
  state(ctx)->split_mode = split;
  return PR_OK;
}

int pr_set_icp_search(pr_ctx* ctx, int mode) {
  if (!ctx) return PR_EINVAL;
  if (mode != PR_ICP_SEARCH_BRUTE && mode != PR_ICP_SEARCH_GRID) return fail(ctx, PR_EINVAL, "pr_set_icp_search: mode=%d (0..1)", mode);
  state(ctx)->search = mode;
  return PR_OK;
}

int pr_get_icp_search(pr_ctx* ctx) {
  if (!ctx) return PR_EINVAL;
  return state(ctx)->search;
}

int pr_icp_nn_radius_dev(pr_ctx* ctx, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_xyz_db, const int64_t* d_offs_db,
                         int32_t Ndb, const int32_t* d_pair_src, const int32_t* d_pair_dst, int32_t c, const double* d_T, int32_t max_src_pts,
                         int32_t max_dst_pts, double max_corr, int64_t* d_out_offs, int32_t* d_nn_idx, double* d_nn_d2) {
  const char* fn = "pr_icp_nn_radius_dev";
  if (int rc = check_sets(ctx, fn, d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, d_pair_src, d_pair_dst, c, max_src_pts, max_dst_pts)) return rc;
  if (int rc = check_params(ctx, fn, 0, max_corr, 0.0, 0.0, 3)) return rc;
  if (!d_out_offs || (c > 0 && !d_T) || (c > 0 && max_src_pts > 0 && (!d_nn_idx || !d_nn_d2)))
    return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  IcpState* S = state(ctx);
  const double mc2 = max_corr * max_corr;
  if (S->search == PR_ICP_SEARCH_BRUTE) {            // the existing scan, then the mask
    if (int rc = pr_icp_nn_dev(ctx, d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, d_pair_src, d_pair_dst, c, d_T, max_src_pts, max_dst_pts,
                               d_out_offs, d_nn_idx, d_nn_d2))
      return rc;
    const pr::IcpClouds A = clouds(d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, d_pair_src, d_pair_dst, c, max_src_pts, max_dst_pts);
    pr::launch_icp_radius_mask(pr::ctx_stream(ctx), A, reinterpret_cast<const long long*>(d_out_offs), d_nn_d2, d_nn_idx, mc2);
    PR_CHECK_HIP(ctx, hipGetLastError());
    return PR_OK;
  }
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const pr::IcpClouds A = clouds(d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, d_pair_src, d_pair_dst, c, max_src_pts, max_dst_pts);
  pr::launch_icp_offsets(st, A, reinterpret_cast<long long*>(d_out_offs));
  if (c > 0) {
    pr::IcpGrid gr;
    if (int rc = grid_build(ctx, S, A, max_corr, &gr)) return rc;
    pr::launch_icp_grid_probe(st, A, gr, d_T, nullptr, std::max(max_src_pts, 1), reinterpret_cast<const long long*>(d_out_offs), d_nn_d2, d_nn_idx,
                              mc2, nullptr, 1);
  }
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_icp_nn_dev(pr_ctx* ctx, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_xyz_db, const int64_t* d_offs_db,
                  int32_t Ndb, const int32_t* d_pair_src, const int32_t* d_pair_dst, int32_t c, const double* d_T, int32_t max_src_pts,
                  int32_t max_dst_pts, int64_t* d_out_offs, int32_t* d_nn_idx, double* d_nn_d2) {
  const char* fn = "pr_icp_nn_dev";
  if (int rc = check_sets(ctx, fn, d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, d_pair_src, d_pair_dst, c, max_src_pts, max_dst_pts)) return rc;
  if (!d_out_offs || (c > 0 && !d_T) || (c > 0 && max_src_pts > 0 && (!d_nn_idx || !d_nn_d2)))
    return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  IcpState* S = state(ctx);
  hipStream_t st = pr::ctx_stream(ctx);
  const pr::IcpClouds A = clouds(d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, d_pair_src, d_pair_dst, c, max_src_pts, max_dst_pts);
  const pr::IcpGeometry g = geometry(S, c, max_src_pts, max_dst_pts);
  if (g.nsplit > 1) {
    if (int rc = grow(ctx, S->slot_d, (size_t)g.nsplit * c * g.ld * 8)) return rc;
    if (int rc = grow(ctx, S->slot_j, (size_t)g.nsplit * c * g.ld * 4)) return rc;
  }
  pr::launch_icp_offsets(st, A, reinterpret_cast<long long*>(d_out_offs));
  pr::launch_icp_nn(st, A, g, d_T, nullptr, ptr<double>(S->slot_d), ptr<int>(S->slot_j), reinterpret_cast<const long long*>(d_out_offs), d_nn_d2,
                    d_nn_idx, 0.0, nullptr);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_icp_pairs_dev(pr_ctx* ctx, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_xyz_db, const int64_t* d_offs_db,
                     int32_t Ndb, const int32_t* d_pair_src, const int32_t* d_pair_dst, int32_t c, const double* d_T0, int32_t max_src_pts,
                     int32_t max_dst_pts, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers,
                     double* d_T_out, pr_icp_stats* d_stats) {
  const char* fn = "pr_icp_pairs_dev";
  if (int rc = check_sets(ctx, fn, d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, d_pair_src, d_pair_dst, c, max_src_pts, max_dst_pts)) return rc;
  if (int rc = check_params(ctx, fn, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers)) return rc;
  if (c > 0 && (!d_T0 || !d_T_out || !d_stats)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  if (c == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  IcpState* S = state(ctx);
  hipStream_t st = pr::ctx_stream(ctx);
  const pr::IcpClouds A = clouds(d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, d_pair_src, d_pair_dst, c, max_src_pts, max_dst_pts);
  const bool grid = S->search == PR_ICP_SEARCH_GRID;
  pr::IcpGeometry g = geometry(S, c, max_src_pts, max_dst_pts);
  if (grid) {                                        // chunks of 256 source points: the split path's chunk geometry, whatever the shape
    g.rq = 1; g.nsplit = 1; g.chunk_pts = 256;
    g.nchunks = std::max(1, (max_src_pts + 255) / 256);
  }
  if (g.nsplit > 1) {
    if (int rc = grow(ctx, S->slot_d, (size_t)g.nsplit * c * g.ld * 8)) return rc;
    if (int rc = grow(ctx, S->slot_j, (size_t)g.nsplit * c * g.ld * 4)) return rc;
  }
  if (int rc = grow(ctx, S->nn_d, (size_t)c * g.ld * 8)) return rc;
  if (int rc = grow(ctx, S->nn_j, (size_t)c * g.ld * 4)) return rc;
  if (int rc = grow(ctx, S->part, (size_t)c * g.nchunks * pr::ICP_PARTIAL * 8)) return rc;
  if (int rc = grow(ctx, S->done, (size_t)c * 4)) return rc;
  if (int rc = grow(ctx, S->prev, (size_t)c * 16)) return rc;
  pr::IcpStats* stats = reinterpret_cast<pr::IcpStats*>(d_stats);
  const pr::IcpParams P{tol_rmse, tol_fitness, min_inliers};
  const double mc2 = max_corr * max_corr;
  int* done = ptr<int>(S->done);
  pr::launch_icp_init(st, A, d_T0, d_T_out, stats, done, ptr<double>(S->prev));
  pr::IcpGrid gr{};
  if (grid)                                          // once per call: the target does not move; all max_iter + 1 passes probe it
    if (int rc = grid_build(ctx, S, A, max_corr, &gr)) return rc;
  // max_iter x (correspondence, finish) and the final pass: a fixed launch count; a finished pair's launches return at once
  for (int32_t it = 0; it <= max_iter; it++) {
    const bool last = it == max_iter;
    if (grid)
      pr::launch_icp_grid_probe(st, A, gr, d_T_out, last ? nullptr : done, g.ld, nullptr, ptr<double>(S->nn_d), ptr<int>(S->nn_j), mc2,
                                ptr<double>(S->part), g.nchunks);
    else
      pr::launch_icp_nn(st, A, g, d_T_out, last ? nullptr : done, ptr<double>(S->slot_d), ptr<int>(S->slot_j), nullptr, ptr<double>(S->nn_d),
                        ptr<int>(S->nn_j), mc2, ptr<double>(S->part));
    pr::launch_icp_finish(st, A, g, ptr<double>(S->part), P, last ? 1 : 0, d_T_out, stats, done, ptr<double>(S->prev));
  }
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

// the host-buffer form of a correspondence pass: radius = false pr_icp_nn, true pr_icp_nn_radius
static int nn_host(pr_ctx* ctx, const char* fn, bool radius, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const double* xyz_db,
                   const int64_t* offs_db, int32_t Ndb, const int32_t* pair_src, const int32_t* pair_dst, int32_t c, const double* T, double max_corr,
                   int64_t* out_offs, int32_t* nn_idx, double* nn_d2) {
  if (int rc = check_sets(ctx, fn, xyz_q, offs_q, Nq, xyz_db, offs_db, Ndb, pair_src, pair_dst, c, 0, 0)) return rc;
  if (radius)
    if (int rc = check_params(ctx, fn, 0, max_corr, 0.0, 0.0, 3)) return rc;
  if (!out_offs || (c > 0 && !T)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  int64_t ms = 0, md = 0;
  std::vector<int64_t> prefix;
  if (int rc = host_shapes(ctx, fn, offs_q, Nq, offs_db, Ndb, pair_src, pair_dst, c, &ms, &md, &prefix)) return rc;
  if (int rc = check_sets(ctx, fn, xyz_q, offs_q, Nq, xyz_db, offs_db, Ndb, pair_src, pair_dst, c, ms, md)) return rc;
  const int64_t total = prefix[(size_t)c];
  if (total > 0 && (!nn_idx || !nn_d2)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  Staging s;
  double* dxq = static_cast<double*>(s.up(xyz_q, (size_t)offs_q[Nq] * 24, st));
  int64_t* doq = static_cast<int64_t*>(s.up(offs_q, ((size_t)Nq + 1) * 8, st));
  double* dxd = static_cast<double*>(s.up(xyz_db, (size_t)offs_db[Ndb] * 24, st));
  int64_t* dod = static_cast<int64_t*>(s.up(offs_db, ((size_t)Ndb + 1) * 8, st));
  int32_t* dps = static_cast<int32_t*>(s.up(pair_src, (size_t)c * 4, st));
  int32_t* dpd = static_cast<int32_t*>(s.up(pair_dst, (size_t)c * 4, st));
  double* dT = static_cast<double*>(s.up(T, (size_t)c * 96, st));
  int64_t* doo = static_cast<int64_t*>(s.get(((size_t)c + 1) * 8));
  int32_t* dj = static_cast<int32_t*>(s.get((size_t)total * 4));
  double* dd = static_cast<double*>(s.get((size_t)total * 8));
  int rc = PR_OK;
  if (s.e == hipSuccess)
    rc = radius ? pr_icp_nn_radius_dev(ctx, dxq, doq, Nq, dxd, dod, Ndb, dps, dpd, c, dT, (int32_t)ms, (int32_t)md, max_corr, doo, dj, dd)
                : pr_icp_nn_dev(ctx, dxq, doq, Nq, dxd, dod, Ndb, dps, dpd, c, dT, (int32_t)ms, (int32_t)md, doo, dj, dd);
  if (rc == PR_OK) {
    s.down(out_offs, doo, ((size_t)c + 1) * 8, st);
    s.down(nn_idx, dj, (size_t)total * 4, st);
    s.down(nn_d2, dd, (size_t)total * 8, st);
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (s.e == hipSuccess) s.e = es;
  if (rc == PR_OK && s.e != hipSuccess) rc = fail(ctx, s.e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "%s: %s", fn, hipGetErrorString(s.e));
  return rc;
}

int pr_icp_nn(pr_ctx* ctx, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const double* xyz_db, const int64_t* offs_db, int32_t Ndb,
              const int32_t* pair_src, const int32_t* pair_dst, int32_t c, const double* T, int64_t* out_offs, int32_t* nn_idx, double* nn_d2) {
  return nn_host(ctx, "pr_icp_nn", false, xyz_q, offs_q, Nq, xyz_db, offs_db, Ndb, pair_src, pair_dst, c, T, 0.0, out_offs, nn_idx, nn_d2);
}

int pr_icp_nn_radius(pr_ctx* ctx, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const double* xyz_db, const int64_t* offs_db, int32_t Ndb,
                     const int32_t* pair_src, const int32_t* pair_dst, int32_t c, const double* T, double max_corr, int64_t* out_offs,
                     int32_t* nn_idx, double* nn_d2) {
  return nn_host(ctx, "pr_icp_nn_radius", true, xyz_q, offs_q, Nq, xyz_db, offs_db, Ndb, pair_src, pair_dst, c, T, max_corr, out_offs, nn_idx, nn_d2);
}

int pr_icp_pairs(pr_ctx* ctx, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const double* xyz_db, const int64_t* offs_db, int32_t Ndb,
                 const int32_t* pair_src, const int32_t* pair_dst, int32_t c, const double* T0, int32_t max_iter, double max_corr,
                 double tol_rmse, double tol_fitness, int32_t min_inliers, double* T_out, pr_icp_stats* stats) {
  const char* fn = "pr_icp_pairs";
  if (int rc = check_sets(ctx, fn, xyz_q, offs_q, Nq, xyz_db, offs_db, Ndb, pair_src, pair_dst, c, 0, 0)) return rc;
  if (int rc = check_params(ctx, fn, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers)) return rc;
  if (c > 0 && (!T0 || !T_out || !stats)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  int64_t ms = 0, md = 0;
  std::vector<int64_t> prefix;
  if (int rc = host_shapes(ctx, fn, offs_q, Nq, offs_db, Ndb, pair_src, pair_dst, c, &ms, &md, &prefix)) return rc;
  if (int rc = check_sets(ctx, fn, xyz_q, offs_q, Nq, xyz_db, offs_db, Ndb, pair_src, pair_dst, c, ms, md)) return rc;
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  if (c == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  Staging s;
  double* dxq = static_cast<double*>(s.up(xyz_q, (size_t)offs_q[Nq] * 24, st));
  int64_t* doq = static_cast<int64_t*>(s.up(offs_q, ((size_t)Nq + 1) * 8, st));
  double* dxd = static_cast<double*>(s.up(xyz_db, (size_t)offs_db[Ndb] * 24, st));
  int64_t* dod = static_cast<int64_t*>(s.up(offs_db, ((size_t)Ndb + 1) * 8, st));
  int32_t* dps = static_cast<int32_t*>(s.up(pair_src, (size_t)c * 4, st));
  int32_t* dpd = static_cast<int32_t*>(s.up(pair_dst, (size_t)c * 4, st));
  double* dT0 = static_cast<double*>(s.up(T0, (size_t)c * 96, st));
  double* dT = static_cast<double*>(s.get((size_t)c * 96));
  pr_icp_stats* dst = static_cast<pr_icp_stats*>(s.get((size_t)c * sizeof(pr_icp_stats)));
  int rc = PR_OK;
  if (s.e == hipSuccess)
    rc = pr_icp_pairs_dev(ctx, dxq, doq, Nq, dxd, dod, Ndb, dps, dpd, c, dT0, (int32_t)ms, (int32_t)md, max_iter, max_corr, tol_rmse, tol_fitness,
                          min_inliers, dT, dst);
  if (rc == PR_OK) {
    s.down(T_out, dT, (size_t)c * 96, st);
    s.down(stats, dst, (size_t)c * sizeof(pr_icp_stats), st);
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (s.e == hipSuccess) s.e = es;
  if (rc == PR_OK && s.e != hipSuccess) rc = fail(ctx, s.e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "%s: %s", fn, hipGetErrorString(s.e));
  return rc;
}

}  // extern "C"
