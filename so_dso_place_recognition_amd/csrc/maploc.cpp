// maploc.cpp — host side of the map localiser (maploc.hip): the opaque pr_maploc over three of a world map's caller-owned
// buffers, its ONE scratch allocation, the argument checks, the stream-ordered index / seed / nn / refine and their host forms, on the
// shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"

static_assert(pr::MAPLOC_SKIPPED == PR_MAPLOC_SKIPPED && pr::MAPLOC_RANGE == PR_MAPLOC_RANGE && pr::MAPLOC_DUPLICATE == PR_MAPLOC_DUPLICATE &&
              pr::MAPLOC_TABLE == PR_MAPLOC_TABLE, "flag bits");
static_assert(sizeof(pr::IcpStats) == sizeof(pr_icp_stats), "stats record");

struct pr_maploc : pr::Handle {      // scratch: everything MapLocView names and the staging of the host forms
  pr::MapLocView v;
  double* stage_xyz = nullptr;        // [pair_capacity * ld][3]
  int64_t* stage_offs = nullptr;      // [pair_capacity + 1]
  int32_t* stage_src = nullptr;       // [pair_capacity]
  double* stage_T = nullptr;          // [pair_capacity][12]
  int32_t* stage_excl = nullptr;      // [pair_capacity][2]
  int64_t* stage_out_offs = nullptr;  // [pair_capacity + 1]
  pr_icp_stats* stage_stats = nullptr;  // [pair_capacity]
  int64_t* stage_info = nullptr;      // [4]
};

namespace {

using pr::at;
using pr::fail;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena {
  size_t table, ctl, offs2, pair_dst, nn_d, nn_j, part, done, prev;
  size_t s_xyz, s_offs, s_src, s_T, s_excl, s_out_offs, s_stats, s_info;
};

Layout layout_of(int64_t ocap, int32_t pcap, int32_t max_src) {
  const size_t T = (size_t)1 << pr::maploc_log2T(ocap), pc = (size_t)pcap, ld = (size_t)std::max(max_src, 1), nch = (ld + 255) / 256;
  Layout l;
  l.table = l.take(16 * T); l.ctl = l.take(16); l.offs2 = l.take(16); l.pair_dst = l.take(4 * pc);
  l.nn_d = l.take(8 * pc * ld); l.nn_j = l.take(4 * pc * ld); l.part = l.take(8 * pc * nch * pr::ICP_PARTIAL);
  l.done = l.take(4 * pc); l.prev = l.take(16 * pc);
  l.s_xyz = l.take(24 * pc * ld); l.s_offs = l.take(8 * (pc + 1)); l.s_src = l.take(4 * pc); l.s_T = l.take(96 * pc); l.s_excl = l.take(8 * pc);
  l.s_out_offs = l.take(8 * (pc + 1)); l.s_stats = l.take(32 * pc); l.s_info = l.take(32);
  return l;
}

bool sizes_ok(int64_t ocap, int32_t pcap, int32_t max_src) {
  return ocap >= 1 && ocap <= pr::MAPLOC_MAX_ROWS && pcap >= 1 && pcap <= 65535 && max_src >= 0 && max_src <= (1 << 26);
}

// check_params of icp.cpp and the contract that makes the 27-voxel search exact
int check_params(pr_maploc* ml, const char* fn, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers) {
  pr_ctx* ctx = ml ? ml->ctx : nullptr;
  if (max_iter < 0) return fail(ctx, PR_EINVAL, "%s: max_iter=%d < 0", fn, max_iter);
  if (!(max_corr > 0.0) || !std::isfinite(max_corr)) return fail(ctx, PR_EINVAL, "%s: max_corr=%g must be positive and finite", fn, max_corr);
  if (min_inliers < 3) return fail(ctx, PR_EINVAL, "%s: min_inliers=%d < 3", fn, min_inliers);
  if (std::isnan(tol_rmse) || std::isnan(tol_fitness)) return fail(ctx, PR_EINVAL, "%s: tol_rmse / tol_fitness is NaN", fn);
  if (!ml) return fail(nullptr, PR_EINVAL, "%s: localiser is NULL", fn);
  if (max_corr * pr::MAPLOC_SLACK > ml->v.cell)
    return fail(ctx, PR_EINVAL, "%s: max_corr=%g (1 + 2^-10) exceeds the cell %g: the 27-voxel search would not be exact", fn, max_corr, ml->v.cell);
  return PR_OK;
}

int check_pairs(pr_maploc* ml, const char* fn, const void* xyz_q, const void* offs_q, int32_t Nq, const void* pair_src, int32_t c) {
  pr_ctx* ctx = ml->ctx;
  if (Nq < 0) return fail(ctx, PR_EINVAL, "%s: Nq=%d < 0", fn, Nq);
  if (c < 0 || c > ml->v.pair_cap) return fail(ctx, PR_EINVAL, "%s: c=%d outside 0 .. pair_capacity=%d", fn, c, ml->v.pair_cap);
  if (!offs_q || (c > 0 && !pair_src) || (c > 0 && ml->v.max_src > 0 && !xyz_q)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  return PR_OK;
}

// what the host forms learn from the host arrays: offsets ascending from >= 0, everything inside the staging, the rows a pass writes
int host_shapes(pr_maploc* ml, const char* fn, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, int64_t* total) {
  pr_ctx* ctx = ml->ctx;
  const pr::MapLocView& v = ml->v;
  if (Nq > v.pair_cap) return fail(ctx, PR_EINVAL, "%s: Nq=%d exceeds pair_capacity=%d (the staging of the host forms)", fn, Nq, v.pair_cap);
  if (offs_q[0] < 0) return fail(ctx, PR_EINVAL, "%s: offs_q is not ascending from 0", fn);
  for (int32_t i = 0; i < Nq; i++) if (offs_q[i + 1] < offs_q[i]) return fail(ctx, PR_EINVAL, "%s: offs_q is not ascending", fn);
  if (offs_q[Nq] > (int64_t)v.pair_cap * v.ld)
    return fail(ctx, PR_EINVAL, "%s: %lld source points exceed pair_capacity x max(max_src_pts, 1) (the staging of the host forms)", fn, (long long)offs_q[Nq]);
  *total = 0;
  for (int32_t i = 0; i < c; i++) {
    const int32_t s = pair_src[i];
    if (s >= 0 && s < Nq) *total += std::min<int64_t>(offs_q[s + 1] - offs_q[s], v.max_src);
  }
  return PR_OK;
}

void upload_pairs(pr::Transfer& t, pr_maploc* ml, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c,
                  const double* T, const int32_t* excl) {
  t.up(ml->stage_offs, offs_q, ((size_t)Nq + 1) * 8);
  t.up(ml->stage_xyz, xyz_q, (size_t)offs_q[Nq] * 24);
  t.up(ml->stage_src, pair_src, (size_t)c * 4);
  t.up(ml->stage_T, T, (size_t)c * 96);
  t.up_opt(ml->stage_excl, excl, (size_t)c * 8);
}

}  // namespace

namespace pr {
const MapLocView* maploc_view(pr_maploc* ml) { return ml ? &ml->v : nullptr; }
pr_ctx* maploc_ctx(pr_maploc* ml) { return ml ? ml->ctx : nullptr; }
}  // namespace pr

extern "C" {

int64_t pr_maploc_scratch_bytes(int64_t out_capacity, int32_t pair_capacity, int32_t max_src_pts) {
  if (!sizes_ok(out_capacity, pair_capacity, max_src_pts)) return 0;
  return (int64_t)layout_of(out_capacity, pair_capacity, max_src_pts).total;
}

int pr_maploc_create(pr_ctx* ctx, const pr_worldmap_buffers* world, int64_t out_capacity, double cell, int32_t pair_capacity, int32_t max_src_pts,
                     pr_maploc** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_maploc_create: out is NULL");
  *out = nullptr;
  if (!world) return fail(ctx, PR_EINVAL, "pr_maploc_create: world is NULL");
  if (!world->xyz || !world->row || !world->state) return fail(ctx, PR_EINVAL, "pr_maploc_create: a buffer is NULL (xyz, row, state)");
  if (out_capacity < 1 || out_capacity > pr::MAPLOC_MAX_ROWS)
    return fail(ctx, PR_EINVAL, "pr_maploc_create: out_capacity=%lld outside 1 .. 2^29", (long long)out_capacity);
  if (!std::isfinite(cell) || !(cell > 0.0)) return fail(ctx, PR_EINVAL, "pr_maploc_create: cell must be finite and positive");
  if (pair_capacity < 1 || pair_capacity > 65535) return fail(ctx, PR_EINVAL, "pr_maploc_create: pair_capacity=%d outside 1 .. 65535", pair_capacity);
  if (max_src_pts < 0 || max_src_pts > (1 << 26)) return fail(ctx, PR_EINVAL, "pr_maploc_create: max_src_pts=%d outside 0 .. 2^26", max_src_pts);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_maploc_create: ctx is NULL");
  const Layout l = layout_of(out_capacity, pair_capacity, max_src_pts);
  pr::Owned<pr_maploc> ml;
  if (int rc = pr::make(ctx, "pr_maploc_create", l.total, ml)) return rc;
  pr::MapLocView& v = ml->v;
  memset(&v, 0, sizeof v);
  v.xyz = world->xyz; v.row = world->row; v.state = world->state;
  v.ocap = out_capacity; v.cell = cell;
  v.log2T = pr::maploc_log2T(out_capacity);
  v.pair_cap = pair_capacity; v.max_src = max_src_pts; v.ld = std::max(max_src_pts, 1); v.nchunks = (v.ld + 255) / 256;
  void* b = ml->scratch;
  v.table = at<unsigned long long>(b, l.table); v.ctl = at<int>(b, l.ctl); v.offs2 = at<int64_t>(b, l.offs2); v.pair_dst = at<int>(b, l.pair_dst);
  v.nn_d = at<double>(b, l.nn_d); v.nn_j = at<int>(b, l.nn_j); v.part = at<double>(b, l.part); v.done = at<int>(b, l.done);
  v.prev = at<double>(b, l.prev);
  ml->stage_xyz = at<double>(b, l.s_xyz); ml->stage_offs = at<int64_t>(b, l.s_offs); ml->stage_src = at<int32_t>(b, l.s_src);
  ml->stage_T = at<double>(b, l.s_T); ml->stage_excl = at<int32_t>(b, l.s_excl); ml->stage_out_offs = at<int64_t>(b, l.s_out_offs);
  ml->stage_stats = at<pr_icp_stats>(b, l.s_stats); ml->stage_info = at<int64_t>(b, l.s_info);
  // everything to zero (pair_dst stays zero for the handle's life; offs2 = {0, 0}: an empty target until the first index), the table empty
  pr::Transfer t(ctx);
  t.fill(b, 0, l.total);
  t.fill(v.table, 0xFF, 16 * ((size_t)1 << v.log2T));
  return pr::commit(ml, t, "pr_maploc_create", out);
}

void pr_maploc_destroy(pr_maploc* ml) { pr::destroy(ml); }      // the world buffers are the caller's

int pr_maploc_count(pr_maploc* ml, int64_t* rows_indexed, int32_t* flags) {
  if (!ml) return fail(nullptr, PR_EINVAL, "pr_maploc_count: localiser is NULL");
  if (!rows_indexed || !flags) return fail(ml->ctx, PR_EINVAL, "pr_maploc_count: a required pointer is NULL");
  int32_t s[4];
  if (int rc = pr::read_state(ml->ctx, "pr_maploc_count", ml->v.ctl, s)) return rc;
  *flags = s[0];
  *rows_indexed = s[1];
  return PR_OK;
}

int pr_maploc_index_dev(pr_maploc* ml, int64_t* d_info) {
  if (!ml) return fail(nullptr, PR_EINVAL, "pr_maploc_index_dev: localiser is NULL");
  pr_ctx* ctx = ml->ctx;
  if (!d_info) return fail(ctx, PR_EINVAL, "pr_maploc_index_dev: d_info is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  PR_CHECK_HIP(ctx, pr::launch_maploc_index(pr::ctx_stream(ctx), ml->v, d_info));
  return PR_OK;
}

int pr_maploc_index(pr_maploc* ml, int64_t* info) {
  if (!ml) return fail(nullptr, PR_EINVAL, "pr_maploc_index: localiser is NULL");
  pr_ctx* ctx = ml->ctx;
  if (!info) return fail(ctx, PR_EINVAL, "pr_maploc_index: info is NULL");
  pr::Transfer t(ctx);
  t.run([&] { return pr_maploc_index_dev(ml, ml->stage_info); });
  t.down(info, ml->stage_info, 4 * sizeof(int64_t));
  return t.finish(ctx, "pr_maploc_index");
}

int pr_maploc_seed_dev(pr_maploc* ml, const double* d_poses, const int32_t* d_n, int32_t keyframe_capacity, const int32_t* d_idx,
                       const uint8_t* d_accepted, const double* d_T_rel, const int32_t* d_src, int32_t c, double* d_T0, int32_t* d_pair_src) {
  const char* fn = "pr_maploc_seed_dev";
  pr_ctx* ctx = ml ? ml->ctx : nullptr;
  if (keyframe_capacity < 1) return fail(ctx, PR_EINVAL, "%s: keyframe_capacity=%d is below 1", fn, keyframe_capacity);
  if (!ml) return fail(nullptr, PR_EINVAL, "%s: localiser is NULL", fn);
  if (c < 0 || c > ml->v.pair_cap) return fail(ctx, PR_EINVAL, "%s: c=%d outside 0 .. pair_capacity=%d", fn, c, ml->v.pair_cap);
  if (!d_poses || !d_n || (c > 0 && (!d_idx || !d_T0 || !d_pair_src))) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_maploc_seed(pr::ctx_stream(ctx), d_poses, d_n, keyframe_capacity, d_idx, d_accepted, d_T_rel, d_src, c, d_T0, d_pair_src);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_maploc_nn_dev(pr_maploc* ml, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                     const double* d_T, const int32_t* d_excl, double max_corr, int64_t* d_out_offs, int32_t* d_nn_idx, double* d_nn_d2) {
  const char* fn = "pr_maploc_nn_dev";
  if (int rc = check_params(ml, fn, 0, max_corr, 0.0, 0.0, 3)) return rc;
  if (int rc = check_pairs(ml, fn, d_xyz_q, d_offs_q, Nq, d_pair_src, c)) return rc;
  pr_ctx* ctx = ml->ctx;
  const pr::MapLocView& v = ml->v;
  if (!d_out_offs || (c > 0 && !d_T) || (c > 0 && v.max_src > 0 && (!d_nn_idx || !d_nn_d2)))
    return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const pr::IcpClouds A = pr::maploc_clouds(v, d_xyz_q, d_offs_q, Nq, d_pair_src, c);
  pr::launch_icp_offsets(st, A, reinterpret_cast<long long*>(d_out_offs));
  pr::launch_maploc_probe(st, v, A, d_T, d_excl, nullptr, reinterpret_cast<const long long*>(d_out_offs), d_nn_d2, d_nn_idx, max_corr * max_corr,
                          nullptr);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_maploc_refine_dev(pr_maploc* ml, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                         const double* d_T0, const int32_t* d_excl, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness,
                         int32_t min_inliers, double* d_T_out, pr_icp_stats* d_stats) {
  const char* fn = "pr_maploc_refine_dev";
  if (int rc = check_params(ml, fn, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers)) return rc;
  if (int rc = check_pairs(ml, fn, d_xyz_q, d_offs_q, Nq, d_pair_src, c)) return rc;
  pr_ctx* ctx = ml->ctx;
  const pr::MapLocView& v = ml->v;
  if (c > 0 && (!d_T0 || !d_T_out || !d_stats)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (c == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const pr::IcpClouds A = pr::maploc_clouds(v, d_xyz_q, d_offs_q, Nq, d_pair_src, c);
  const pr::IcpGeometry g{1, 1, v.ld, 256, v.nchunks};             // chunks of 256 source points: the GRID search's geometry
  pr::IcpStats* stats = reinterpret_cast<pr::IcpStats*>(d_stats);
  const pr::IcpParams P{tol_rmse, tol_fitness, min_inliers};
  const double mc2 = max_corr * max_corr;
  pr::launch_icp_init(st, A, d_T0, d_T_out, stats, v.done, v.prev);
  // max_iter x (probe, finish) and the final pass: a fixed launch count; a finished pair's launches return at once
  for (int32_t it = 0; it <= max_iter; it++) {
    const bool last = it == max_iter;
    pr::launch_maploc_probe(st, v, A, d_T_out, d_excl, last ? nullptr : v.done, nullptr, v.nn_d, v.nn_j, mc2, v.part);
    pr::launch_icp_finish(st, A, g, v.part, P, last ? 1 : 0, d_T_out, stats, v.done, v.prev);
  }
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_maploc_nn(pr_maploc* ml, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T,
                 const int32_t* excl, double max_corr, int64_t* out_offs, int32_t* nn_idx, double* nn_d2) {
  const char* fn = "pr_maploc_nn";
  if (int rc = check_params(ml, fn, 0, max_corr, 0.0, 0.0, 3)) return rc;
  if (int rc = check_pairs(ml, fn, xyz_q, offs_q, Nq, pair_src, c)) return rc;
  pr_ctx* ctx = ml->ctx;
  if (!out_offs || (c > 0 && !T)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  int64_t total = 0;
  if (int rc = host_shapes(ml, fn, offs_q, Nq, pair_src, c, &total)) return rc;
  if (offs_q[Nq] > 0 && !xyz_q) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (total > 0 && (!nn_idx || !nn_d2)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::Transfer t(ctx);
  upload_pairs(t, ml, xyz_q, offs_q, Nq, pair_src, c, T, excl);
  // (the compacted rows fit the handle's own [pair_capacity][ld] arrays, which a pass of its own does not use)
  t.run([&] {
    return pr_maploc_nn_dev(ml, ml->stage_xyz, ml->stage_offs, Nq, ml->stage_src, c, ml->stage_T, excl ? ml->stage_excl : nullptr, max_corr,
                            ml->stage_out_offs, ml->v.nn_j, ml->v.nn_d);
  });
  t.down(out_offs, ml->stage_out_offs, ((size_t)c + 1) * 8);
  t.down(nn_idx, ml->v.nn_j, (size_t)total * 4);
  t.down(nn_d2, ml->v.nn_d, (size_t)total * 8);
  return t.finish(ctx, fn);
}

int pr_maploc_refine(pr_maploc* ml, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T0,
                     const int32_t* excl, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers,
                     double* T_out, pr_icp_stats* stats) {
  const char* fn = "pr_maploc_refine";
  if (int rc = check_params(ml, fn, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers)) return rc;
  if (int rc = check_pairs(ml, fn, xyz_q, offs_q, Nq, pair_src, c)) return rc;
  pr_ctx* ctx = ml->ctx;
  if (c > 0 && (!T0 || !T_out || !stats)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  int64_t total = 0;
  if (int rc = host_shapes(ml, fn, offs_q, Nq, pair_src, c, &total)) return rc;
  if (offs_q[Nq] > 0 && !xyz_q) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (c == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::Transfer t(ctx);
  upload_pairs(t, ml, xyz_q, offs_q, Nq, pair_src, c, T0, excl);
  t.run([&] {                                                      // in place: d_T_out = d_T0
    return pr_maploc_refine_dev(ml, ml->stage_xyz, ml->stage_offs, Nq, ml->stage_src, c, ml->stage_T, excl ? ml->stage_excl : nullptr, max_iter,
                                max_corr, tol_rmse, tol_fitness, min_inliers, ml->stage_T, ml->stage_stats);
  });
  t.down(T_out, ml->stage_T, (size_t)c * 96);
  t.down(stats, ml->stage_stats, (size_t)c * sizeof(pr_icp_stats));
  return t.finish(ctx, fn);
}

}  // extern "C"
