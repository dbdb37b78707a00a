// mapplane.cpp — host side of the plane-metric map localiser (mapplane.hip): the opaque pr_mapplane over a pr_maploc,
// its ONE scratch allocation, the argument checks, the stream-ordered normals / refine and their host forms, on the shared handle core
// (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"

struct pr_mapplane : pr::Handle {    // scratch: the refinement's arrays and the staging of the host forms
  pr_maploc* ml = nullptr;
  const pr::MapLocView* v = nullptr;  // the localiser's: table, cell, out_capacity, world record, offs2 of the last index, the create sizes
  double* nn_d = nullptr;             // [pair_capacity][ld]
  int* nn_j = nullptr;                // [pair_capacity][ld]
  double* part = nullptr;             // [pair_capacity][nchunks][MAPPLANE_SUMS]
  int* done = nullptr;                // [pair_capacity]
  double* prev = nullptr;             // [pair_capacity][2]
  double* stage_xyz = nullptr;        // [pair_capacity * ld][3]
  int64_t* stage_offs = nullptr;      // [pair_capacity + 1]
  int32_t* stage_src = nullptr;       // [pair_capacity]
  double* stage_T = nullptr;          // [pair_capacity][12]
  int32_t* stage_excl = nullptr;      // [pair_capacity][2]
  pr_icp_stats* stage_stats = nullptr;  // [pair_capacity]
  double* stage_normals = nullptr;    // [pair_capacity * ld][3]
  int32_t* stage_ninfo = nullptr;     // [pair_capacity * ld]
};

namespace {

using pr::at;
using pr::fail;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena {
  size_t nn_d, nn_j, part, done, prev, s_xyz, s_offs, s_src, s_T, s_excl, s_stats, s_normals, s_ninfo;
};

Layout layout_of(int32_t pcap, int32_t max_src) {
  const size_t pc = (size_t)pcap, ld = (size_t)std::max(max_src, 1), nch = (ld + 255) / 256;
  Layout l;
  l.nn_d = l.take(8 * pc * ld); l.nn_j = l.take(4 * pc * ld); l.part = l.take(8 * pc * nch * pr::MAPPLANE_SUMS);
  l.done = l.take(4 * pc); l.prev = l.take(16 * pc);
  l.s_xyz = l.take(24 * pc * ld); l.s_offs = l.take(8 * (pc + 1)); l.s_src = l.take(4 * pc); l.s_T = l.take(96 * pc); l.s_excl = l.take(8 * pc);
  l.s_stats = l.take(32 * pc); l.s_normals = l.take(24 * pc * ld); l.s_ninfo = l.take(4 * pc * ld);
  return l;
}

bool sizes_ok(int32_t pcap, int32_t max_src) { return pcap >= 1 && pcap <= 65535 && max_src >= 0 && max_src <= (1 << 26); }

int check_normals(pr_mapplane* mp, const char* fn, double radius, int32_t min_nbrs, double max_ratio, const void* normals, const void* ninfo) {
  pr_ctx* ctx = mp ? mp->ctx : nullptr;
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(ctx, PR_EINVAL, "%s: radius=%g must be positive and finite", fn, radius);
  if (min_nbrs < 3 || min_nbrs > 27) return fail(ctx, PR_EINVAL, "%s: min_nbrs=%d outside 3 .. 27", fn, min_nbrs);
  if (!(max_ratio > 0.0) || !(max_ratio <= 1.0)) return fail(ctx, PR_EINVAL, "%s: max_ratio=%g outside (0, 1]", fn, max_ratio);
  if (!normals || !ninfo) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!mp) return fail(nullptr, PR_EINVAL, "%s: plane localiser is NULL", fn);
  if (radius * pr::MAPLOC_SLACK > mp->v->cell)
    return fail(ctx, PR_EINVAL, "%s: radius=%g (1 + 2^-10) exceeds the cell %g: the 27 voxels would not hold the ball", fn, radius, mp->v->cell);
  return PR_OK;
}

// check_params of maploc.cpp with the plane form's floor on min_inliers
int check_params(pr_mapplane* mp, const char* fn, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers) {
  pr_ctx* ctx = mp ? mp->ctx : nullptr;
  if (max_iter < 0) return fail(ctx, PR_EINVAL, "%s: max_iter=%d < 0", fn, max_iter);
  if (!(max_corr > 0.0) || !std::isfinite(max_corr)) return fail(ctx, PR_EINVAL, "%s: max_corr=%g must be positive and finite", fn, max_corr);
  if (min_inliers < 6) return fail(ctx, PR_EINVAL, "%s: min_inliers=%d < 6", fn, min_inliers);
  if (std::isnan(tol_rmse) || std::isnan(tol_fitness)) return fail(ctx, PR_EINVAL, "%s: tol_rmse / tol_fitness is NaN", fn);
  if (!mp) return fail(nullptr, PR_EINVAL, "%s: plane localiser is NULL", fn);
  if (max_corr * pr::MAPLOC_SLACK > mp->v->cell)
    return fail(ctx, PR_EINVAL, "%s: max_corr=%g (1 + 2^-10) exceeds the cell %g: the 27-voxel search would not be exact", fn, max_corr, mp->v->cell);
  return PR_OK;
}

int check_pairs(pr_mapplane* mp, const char* fn, const void* xyz_q, const void* offs_q, int32_t Nq, const void* pair_src, int32_t c) {
  pr_ctx* ctx = mp->ctx;
  const pr::MapLocView& v = *mp->v;
  if (Nq < 0) return fail(ctx, PR_EINVAL, "%s: Nq=%d < 0", fn, Nq);
  if (c < 0 || c > v.pair_cap) return fail(ctx, PR_EINVAL, "%s: c=%d outside 0 .. pair_capacity=%d", fn, c, v.pair_cap);
  if (!offs_q || (c > 0 && !pair_src) || (c > 0 && v.max_src > 0 && !xyz_q)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  return PR_OK;
}

// the world rows fit the staging of the host forms
int host_world(pr_mapplane* mp, const char* fn) {
  const pr::MapLocView& v = *mp->v;
  if (v.ocap > (int64_t)v.pair_cap * v.ld)
    return fail(mp->ctx, PR_EINVAL, "%s: out_capacity=%lld exceeds pair_capacity x max(max_src_pts, 1) (the staging of the host forms)", fn,
                (long long)v.ocap);
  return PR_OK;
}

}  // namespace

extern "C" {

int64_t pr_mapplane_scratch_bytes(int32_t pair_capacity, int32_t max_src_pts) {
  if (!sizes_ok(pair_capacity, max_src_pts)) return 0;
  return (int64_t)layout_of(pair_capacity, max_src_pts).total;
}

int pr_mapplane_create(pr_ctx* ctx, pr_maploc* ml, pr_mapplane** out) {
  if (!out) return fail(ctx, PR_EINVAL, "pr_mapplane_create: out is NULL");
  *out = nullptr;
  if (!ml) return fail(ctx, PR_EINVAL, "pr_mapplane_create: localiser is NULL");
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_mapplane_create: ctx is NULL");
  if (pr::maploc_ctx(ml) != ctx) return fail(ctx, PR_EINVAL, "pr_mapplane_create: the localiser belongs to another context");
  const pr::MapLocView* lv = pr::maploc_view(ml);
  const Layout l = layout_of(lv->pair_cap, lv->max_src);
  pr::Owned<pr_mapplane> mp;
  if (int rc = pr::make(ctx, "pr_mapplane_create", l.total, mp)) return rc;
  mp->ml = ml; mp->v = lv;
  void* b = mp->scratch;
  mp->nn_d = at<double>(b, l.nn_d); mp->nn_j = at<int>(b, l.nn_j); mp->part = at<double>(b, l.part); mp->done = at<int>(b, l.done);
  mp->prev = at<double>(b, l.prev);
  mp->stage_xyz = at<double>(b, l.s_xyz); mp->stage_offs = at<int64_t>(b, l.s_offs); mp->stage_src = at<int32_t>(b, l.s_src);
  mp->stage_T = at<double>(b, l.s_T); mp->stage_excl = at<int32_t>(b, l.s_excl); mp->stage_stats = at<pr_icp_stats>(b, l.s_stats);
  mp->stage_normals = at<double>(b, l.s_normals); mp->stage_ninfo = at<int32_t>(b, l.s_ninfo);
  pr::Transfer t(ctx);
  t.fill(b, 0, l.total);
  return pr::commit(mp, t, "pr_mapplane_create", out);
}

// the localiser and the world buffers are the caller's
void pr_mapplane_destroy(pr_mapplane* mp) { pr::destroy(mp); }

int pr_mapplane_normals_dev(pr_mapplane* mp, double radius, int32_t min_nbrs, double max_ratio, double* d_normals, int32_t* d_ninfo) {
  const char* fn = "pr_mapplane_normals_dev";
  if (int rc = check_normals(mp, fn, radius, min_nbrs, max_ratio, d_normals, d_ninfo)) return rc;
  pr_ctx* ctx = mp->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_mapplane_normals(pr::ctx_stream(ctx), *mp->v, radius * radius, min_nbrs, max_ratio, d_normals, d_ninfo);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_mapplane_refine_dev(pr_mapplane* mp, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                           const double* d_T0, const int32_t* d_excl, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness,
                           int32_t min_inliers, const double* d_normals, const int32_t* d_ninfo, double* d_T_out, pr_icp_stats* d_stats) {
  const char* fn = "pr_mapplane_refine_dev";
  if (int rc = check_params(mp, fn, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers)) return rc;
  if (int rc = check_pairs(mp, fn, d_xyz_q, d_offs_q, Nq, d_pair_src, c)) return rc;
  pr_ctx* ctx = mp->ctx;
  const pr::MapLocView& v = *mp->v;
  if (!d_normals || !d_ninfo || (c > 0 && (!d_T0 || !d_T_out || !d_stats))) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (c == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const pr::IcpClouds A = pr::maploc_clouds(v, d_xyz_q, d_offs_q, Nq, d_pair_src, c);
  pr::IcpStats* stats = reinterpret_cast<pr::IcpStats*>(d_stats);
  const pr::IcpParams P{tol_rmse, tol_fitness, min_inliers};
  const double mc2 = max_corr * max_corr;
  pr::launch_icp_init(st, A, d_T0, d_T_out, stats, mp->done, mp->prev);
  // max_iter x (probe, sums, update) and the final pass: a fixed launch count; a finished pair's launches return at once
  for (int32_t it = 0; it <= max_iter; it++) {
    const bool last = it == max_iter;
    const int* done = last ? nullptr : mp->done;
    pr::launch_maploc_probe(st, v, A, d_T_out, d_excl, done, nullptr, mp->nn_d, mp->nn_j, mc2, nullptr);
    pr::launch_mapplane_sums(st, A, d_T_out, done, mp->nn_d, mp->nn_j, v.ld, v.nchunks, mc2, d_normals, d_ninfo, mp->part);
    pr::launch_mapplane_update(st, A, mp->part, v.nchunks, P, last ? 1 : 0, d_T_out, stats, mp->done, mp->prev);
  }
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_mapplane_normals(pr_mapplane* mp, double radius, int32_t min_nbrs, double max_ratio, double* normals, int32_t* ninfo) {
  const char* fn = "pr_mapplane_normals";
  if (int rc = check_normals(mp, fn, radius, min_nbrs, max_ratio, normals, ninfo)) return rc;
  if (int rc = host_world(mp, fn)) return rc;
  pr_ctx* ctx = mp->ctx;
  const size_t oc = (size_t)mp->v->ocap;
  pr::Transfer t(ctx);
  t.run([&] { return pr_mapplane_normals_dev(mp, radius, min_nbrs, max_ratio, mp->stage_normals, mp->stage_ninfo); });
  t.down(normals, mp->stage_normals, oc * 24);
  t.down(ninfo, mp->stage_ninfo, oc * 4);
  return t.finish(ctx, fn);
}

int pr_mapplane_refine(pr_mapplane* mp, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c,
                       const double* T0, const int32_t* excl, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness,
                       int32_t min_inliers, const double* normals, const int32_t* ninfo, double* T_out, pr_icp_stats* stats) {
  const char* fn = "pr_mapplane_refine";
  if (int rc = check_params(mp, fn, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers)) return rc;
  if (int rc = check_pairs(mp, fn, xyz_q, offs_q, Nq, pair_src, c)) return rc;
  pr_ctx* ctx = mp->ctx;
  const pr::MapLocView& v = *mp->v;
  if (!normals || !ninfo || (c > 0 && (!T0 || !T_out || !stats))) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (int rc = host_world(mp, fn)) return rc;
  if (Nq > v.pair_cap) return fail(ctx, PR_EINVAL, "%s: Nq=%d exceeds pair_capacity=%d (the staging of the host forms)", fn, Nq, v.pair_cap);
  if (offs_q[0] < 0) return fail(ctx, PR_EINVAL, "%s: offs_q is not ascending from 0", fn);
  for (int32_t i = 0; i < Nq; i++) if (offs_q[i + 1] < offs_q[i]) return fail(ctx, PR_EINVAL, "%s: offs_q is not ascending", fn);
  if (offs_q[Nq] > (int64_t)v.pair_cap * v.ld)
    return fail(ctx, PR_EINVAL, "%s: %lld source points exceed pair_capacity x max(max_src_pts, 1) (the staging of the host forms)", fn, (long long)offs_q[Nq]);
  if (offs_q[Nq] > 0 && !xyz_q) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (c == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  const size_t oc = (size_t)v.ocap;
  pr::Transfer t(ctx);
  t.up(mp->stage_offs, offs_q, ((size_t)Nq + 1) * 8);
  t.up(mp->stage_xyz, xyz_q, (size_t)offs_q[Nq] * 24);
  t.up(mp->stage_src, pair_src, (size_t)c * 4);
  t.up(mp->stage_T, T0, (size_t)c * 96);
  t.up_opt(mp->stage_excl, excl, (size_t)c * 8);
  t.up(mp->stage_normals, normals, oc * 24);
  t.up(mp->stage_ninfo, ninfo, oc * 4);
  t.run([&] {                                                      // in place: d_T_out = d_T0
    return pr_mapplane_refine_dev(mp, mp->stage_xyz, mp->stage_offs, Nq, mp->stage_src, c, mp->stage_T, excl ? mp->stage_excl : nullptr, max_iter,
                                  max_corr, tol_rmse, tol_fitness, min_inliers, mp->stage_normals, mp->stage_ninfo, mp->stage_T, mp->stage_stats);
  });
  t.down(T_out, mp->stage_T, (size_t)c * 96);
  t.down(stats, mp->stage_stats, (size_t)c * sizeof(pr_icp_stats));
  return t.finish(ctx, fn);
}

}  // extern "C"
