// mapgrow.cpp — host side of the incremental world map (mapgrow.hip): the opaque pr_mapgrow over a pr_worldmap and the
// pr_maploc created over the same world buffer record, its ONE scratch allocation, the argument checks, the stream-ordered sync / extend /
// normals and their host forms, on the shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"

static_assert(pr::MAPGROW_ORDER == PR_MAPGROW_ORDER && pr::MAPGROW_STALE == PR_MAPGROW_STALE && pr::MAPGROW_FULL == PR_MAPGROW_FULL, "flag bits");

struct pr_mapgrow : pr::Handle {     // scratch: everything MapGrowView names of its own and the staging of the host forms
  pr::MapGrowView v;
  double* stage_pose = nullptr;       // [12]: the call's pose row
  int32_t* stage_row = nullptr;       // [4]
  int64_t* stage_info = nullptr;      // [4]
  double* stage_normals = nullptr;    // [27 mcp][3]: the compact form of the host normals
  int32_t* stage_ninfo = nullptr;     // [27 mcp]
  int32_t* stage_rows = nullptr;      // [27 mcp]
};

namespace {

using pr::at;
using pr::fail;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena { size_t ctl, slot_of, blk, s_pose, s_row, s_info, s_normals, s_ninfo, s_rows; };

Layout layout_of(int32_t mcp) {
  const size_t m = (size_t)mcp, nblk = (m + 255) / 256;
  Layout l;
  l.ctl = l.take(64); l.slot_of = l.take(4 * m); l.blk = l.take(8 * nblk);
  l.s_pose = l.take(96); l.s_row = l.take(16); l.s_info = l.take(32);
  l.s_normals = l.take(648 * m); l.s_ninfo = l.take(108 * m); l.s_rows = l.take(108 * m);
  return l;
}

bool sizes_ok(int32_t mcp) { return mcp >= 1 && mcp <= pr::MAPGROW_MAX_CLOUD; }

// pr_mapplane_normals_dev's refusals
int check_normals(pr_mapgrow* mg, const char* fn, double radius, int32_t min_nbrs, double max_ratio, const void* normals, const void* ninfo) {
  pr_ctx* ctx = mg ? mg->ctx : nullptr;
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(ctx, PR_EINVAL, "%s: radius=%g must be positive and finite", fn, radius);
  if (min_nbrs < 3 || min_nbrs > 27) return fail(ctx, PR_EINVAL, "%s: min_nbrs=%d outside 3 .. 27", fn, min_nbrs);
  if (!(max_ratio > 0.0) || !(max_ratio <= 1.0)) return fail(ctx, PR_EINVAL, "%s: max_ratio=%g outside (0, 1]", fn, max_ratio);
  if (!normals || !ninfo) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!mg) return fail(nullptr, PR_EINVAL, "%s: grower is NULL", fn);
  if (radius * pr::MAPLOC_SLACK > mg->v.cell)
    return fail(ctx, PR_EINVAL, "%s: radius=%g (1 + 2^-10) exceeds the cell %g: the 27 voxels would not hold the ball", fn, radius, mg->v.cell);
  return PR_OK;
}

}  // namespace

extern "C" {

int64_t pr_mapgrow_scratch_bytes(int32_t max_cloud_points) {
  if (!sizes_ok(max_cloud_points)) return 0;
  return (int64_t)layout_of(max_cloud_points).total;
}

int pr_mapgrow_create(pr_ctx* ctx, pr_worldmap* wm, pr_maploc* ml, pr_mapgrow** out) {
  if (!out) return fail(ctx, PR_EINVAL, "pr_mapgrow_create: out is NULL");
  *out = nullptr;
  if (!wm) return fail(ctx, PR_EINVAL, "pr_mapgrow_create: world map is NULL");
  if (!ml) return fail(ctx, PR_EINVAL, "pr_mapgrow_create: localiser is NULL");
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_mapgrow_create: ctx is NULL");
  if (pr::worldmap_ctx(wm) != ctx) return fail(ctx, PR_EINVAL, "pr_mapgrow_create: the world map belongs to another context");
  if (pr::maploc_ctx(ml) != ctx) return fail(ctx, PR_EINVAL, "pr_mapgrow_create: the localiser belongs to another context");
  const pr::WorldMapView& w = *pr::worldmap_view(wm);
  const pr::MapLocView& l = *pr::maploc_view(ml);
  if (w.xyz != l.xyz || w.row != l.row || w.state != l.state || w.ocap != l.ocap)
    return fail(ctx, PR_EINVAL, "pr_mapgrow_create: the localiser was created over another world buffer record or out_capacity");
  const int32_t mcp = pr::worldmap_max_cloud(wm);
  if (!sizes_ok(mcp)) return fail(ctx, PR_EINVAL, "pr_mapgrow_create: the map's max_cloud_points=%d outside 1 .. 2^26", mcp);
  const Layout lay = layout_of(mcp);
  pr::Owned<pr_mapgrow> mg;
  if (int rc = pr::make(ctx, "pr_mapgrow_create", lay.total, mg)) return rc;
  pr::MapGrowView& v = mg->v;
  memset(&v, 0, sizeof v);
  v.w = w;
  v.table = l.table; v.ml_ctl = l.ctl; v.offs2 = l.offs2;
  v.cell = l.cell; v.log2T = l.log2T;
  v.mcp = mcp; v.nblk = (mcp + 255) / 256;
  void* b = mg->scratch;
  v.ctl = at<int>(b, lay.ctl); v.slot_of = at<int>(b, lay.slot_of); v.blk = at<int>(b, lay.blk);
  mg->stage_pose = at<double>(b, lay.s_pose); mg->stage_row = at<int32_t>(b, lay.s_row); mg->stage_info = at<int64_t>(b, lay.s_info);
  mg->stage_normals = at<double>(b, lay.s_normals); mg->stage_ninfo = at<int32_t>(b, lay.s_ninfo); mg->stage_rows = at<int32_t>(b, lay.s_rows);
  pr::Transfer t(ctx);
  t.fill(b, 0, lay.total);
  return pr::commit(mg, t, "pr_mapgrow_create", out);
}

// the world map, the localiser and the world buffers are the caller's
void pr_mapgrow_destroy(pr_mapgrow* mg) { pr::destroy(mg); }

int pr_mapgrow_count(pr_mapgrow* mg, int32_t* fused, int64_t* rows, int32_t* flags) {
  if (!mg) return fail(nullptr, PR_EINVAL, "pr_mapgrow_count: grower is NULL");
  if (!fused || !rows || !flags) return fail(mg->ctx, PR_EINVAL, "pr_mapgrow_count: a required pointer is NULL");
  PR_CHECK_HIP(mg->ctx, hipSetDevice(pr::ctx_device(mg->ctx)));
  int32_t s[8];
  pr::Transfer t(mg->ctx);
  t.down(s, mg->v.ctl, sizeof s);
  if (int rc = t.finish(mg->ctx, "pr_mapgrow_count")) return rc;
  *fused = s[pr::MG_FUSED];
  *rows = s[pr::MG_SEEN];
  *flags = s[pr::MG_LAST];
  return PR_OK;
}

int pr_mapgrow_sync_dev(pr_mapgrow* mg, const int32_t* d_n) {
  if (!mg) return fail(nullptr, PR_EINVAL, "pr_mapgrow_sync_dev: grower is NULL");
  pr_ctx* ctx = mg->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_mapgrow_sync(pr::ctx_stream(ctx), mg->v, d_n ? d_n : mg->v.w.m_state);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_mapgrow_extend_dev(pr_mapgrow* mg, const double* d_poses, const int32_t* d_row, int64_t* d_info) {
  pr_ctx* ctx = mg ? mg->ctx : nullptr;
  if (!d_row || !d_info) return fail(ctx, PR_EINVAL, "pr_mapgrow_extend_dev: a required pointer is NULL (d_row, d_info)");
  if (!mg) return fail(nullptr, PR_EINVAL, "pr_mapgrow_extend_dev: grower is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_mapgrow_extend(pr::ctx_stream(ctx), mg->v, d_poses ? d_poses : mg->v.w.m_poses, 0, d_row, d_info);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_mapgrow_normals_dev(pr_mapgrow* mg, double radius, int32_t min_nbrs, double max_ratio, double* d_normals, int32_t* d_ninfo) {
  const char* fn = "pr_mapgrow_normals_dev";
  if (int rc = check_normals(mg, fn, radius, min_nbrs, max_ratio, d_normals, d_ninfo)) return rc;
  pr_ctx* ctx = mg->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_mapgrow_normals(pr::ctx_stream(ctx), mg->v, radius * radius, min_nbrs, max_ratio, d_normals, d_ninfo, nullptr);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_mapgrow_extend(pr_mapgrow* mg, const double* poses, int32_t row, int64_t* info) {
  const char* fn = "pr_mapgrow_extend";
  pr_ctx* ctx = mg ? mg->ctx : nullptr;
  if (!info) return fail(ctx, PR_EINVAL, "%s: info is NULL", fn);
  if (!mg) return fail(nullptr, PR_EINVAL, "%s: grower is NULL", fn);
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  const pr::MapGrowView& v = mg->v;
  // the staging holds ONE pose row: the call's (a row outside the map is refused on the device and its pose never read)
  const bool own = poses && row >= 0 && row < v.w.kcap;
  pr::Transfer t(ctx);
  t.up(mg->stage_row, &row, sizeof row);
  if (own) t.up(mg->stage_pose, poses + 12 * (size_t)row, 96);
  if (t.ok()) {
    pr::launch_mapgrow_extend(t.st, v, poses ? mg->stage_pose : v.w.m_poses, poses ? 1 : 0, mg->stage_row, mg->stage_info);
    t.note(hipGetLastError());
  }
  t.down(info, mg->stage_info, 4 * sizeof(int64_t));
  return t.finish(ctx, fn);
}

int pr_mapgrow_normals(pr_mapgrow* mg, double radius, int32_t min_nbrs, double max_ratio, double* normals, int32_t* ninfo) {
  const char* fn = "pr_mapgrow_normals";
  if (int rc = check_normals(mg, fn, radius, min_nbrs, max_ratio, normals, ninfo)) return rc;
  pr_ctx* ctx = mg->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  const pr::MapGrowView& v = mg->v;
  pr::Transfer t(ctx);
  pr::launch_mapgrow_normals(t.st, v, radius * radius, min_nbrs, max_ratio, mg->stage_normals, mg->stage_ninfo, mg->stage_rows);
  t.note(hipGetLastError());
  int32_t s[4];
  int32_t state[4];
  t.down(s, v.ctl, sizeof s);
  t.down(state, v.w.state, sizeof state);
  if (int rc = t.finish(ctx, fn)) return rc;
  // the kernel's own clamps: the range lies inside 0 .. R and holds at most max_cloud_points rows
  const int64_t R = std::min<int64_t>(std::max<int64_t>(state[0], 0), v.w.ocap);
  const int64_t a = std::min<int64_t>(std::max<int64_t>(s[pr::MG_A], 0), R), b = std::min<int64_t>(std::max<int64_t>(s[pr::MG_B], a), R);
  const size_t lanes = 27 * (size_t)std::min<int64_t>(b - a, v.mcp);
  if (!lanes) return PR_OK;
  std::vector<int32_t> rows(lanes), inf(lanes);
  std::vector<double> nrm(3 * lanes);
  t.down(rows.data(), mg->stage_rows, lanes * 4);
  t.down(inf.data(), mg->stage_ninfo, lanes * 4);
  t.down(nrm.data(), mg->stage_normals, lanes * 24);
  if (int rc = t.finish(ctx, fn)) return rc;
  for (size_t L = 0; L < lanes; L++) {
    const int32_t j = rows[L];
    if (j < 0 || j >= v.w.ocap) continue;
    memcpy(normals + 3 * (size_t)j, nrm.data() + 3 * L, 24);
    ninfo[j] = inf[L];
  }
  return PR_OK;
}

}  // extern "C"
