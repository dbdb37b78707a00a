// submap.cpp — host side of the local submaps (submap.hip): the opaque pr_submap, its ONE scratch allocation, the argument
// checks, the stream-ordered build and its host form (which stages in an allocation of its own for the call), on the shared handle core
// (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"
#include "submap.hpp"

static_assert(pr::SUBMAP_TRUNCATED == PR_SUBMAP_TRUNCATED && pr::SUBMAP_NO_CENTER == PR_SUBMAP_NO_CENTER && pr::SUBMAP_OVERFLOW == PR_SUBMAP_OVERFLOW,
              "flag bits");
static_assert(sizeof(pr_submap_params) == 16, "four int32, no padding");

struct pr_submap : pr::Handle {      // scratch: everything SubmapView names
  pr::SubmapView v;
};

namespace {

using pr::at;
using pr::fail;

constexpr int32_t MAX_SLOTS = 65535, MAX_CLOUD = 1 << 26, MAX_KEYFRAMES = 1 << 24;
constexpr int64_t MAX_POINTS = (int64_t)1 << 40;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena { size_t row, dst, len, src, tot, flags, taken, base; };

Layout layout_of(int32_t slot_capacity, int32_t w_max) {
  const size_t S = (size_t)slot_capacity, SL = S * (size_t)(2 * w_max + 1);
  Layout l;
  l.row = l.take(4 * SL); l.dst = l.take(4 * SL); l.len = l.take(4 * SL); l.src = l.take(8 * SL);
  l.tot = l.take(4 * S); l.flags = l.take(4 * S); l.taken = l.take(4 * S); l.base = l.take(8 * S);
  return l;
}

bool sizes_ok(int32_t slot_capacity, int32_t w_max) { return slot_capacity >= 1 && slot_capacity <= MAX_SLOTS && w_max >= 0 && w_max <= pr::SUBMAP_MAX_W; }

// the value checks of a build, before any device is touched; 0 when acceptable.  Without a handle the limits are create's widest.
int check_build(pr_ctx* ctx, const pr_submap* g, int32_t c, const pr_submap_params* p, const char* who) {
  if (!p) return fail(ctx, PR_EINVAL, "%s: params is NULL", who);
  const int32_t cmax = g ? g->v.slot_capacity : MAX_SLOTS, wmax = g ? g->v.w_max : pr::SUBMAP_MAX_W;
  if (c < 0 || c > cmax) return fail(ctx, PR_EINVAL, "%s: c=%d outside 0 .. slot_capacity=%d", who, c, cmax);
  if (p->half_window < 0 || p->half_window > wmax) return fail(ctx, PR_EINVAL, "%s: half_window=%d outside 0 .. w_max=%d", who, p->half_window, wmax);
  if (p->max_pts < 1) return fail(ctx, PR_EINVAL, "%s: max_pts=%d is below 1", who, p->max_pts);
  if (p->avoid_gap < 0) return fail(ctx, PR_EINVAL, "%s: avoid_gap=%d is negative", who, p->avoid_gap);
  return PR_OK;
}

}  // namespace

extern "C" {

int64_t pr_submap_scratch_bytes(int32_t slot_capacity, int32_t w_max) {
  if (!sizes_ok(slot_capacity, w_max)) return 0;
  return (int64_t)layout_of(slot_capacity, w_max).total;
}

int pr_submap_create(pr_ctx* ctx, int32_t slot_capacity, int32_t w_max, int64_t point_capacity, int32_t max_cloud_points, int32_t keyframe_capacity,
                     pr_submap** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_submap_create: out is NULL");
  *out = nullptr;
  if (slot_capacity < 1 || slot_capacity > MAX_SLOTS)
    return fail(ctx, PR_EINVAL, "pr_submap_create: slot_capacity=%d outside 1 .. %d", slot_capacity, MAX_SLOTS);
  if (w_max < 0 || w_max > pr::SUBMAP_MAX_W) return fail(ctx, PR_EINVAL, "pr_submap_create: w_max=%d outside 0 .. %d", w_max, pr::SUBMAP_MAX_W);
  if (point_capacity < 1 || point_capacity > MAX_POINTS)
    return fail(ctx, PR_EINVAL, "pr_submap_create: point_capacity=%lld outside 1 .. 2^40", (long long)point_capacity);
  if (max_cloud_points < 1 || max_cloud_points > MAX_CLOUD)
    return fail(ctx, PR_EINVAL, "pr_submap_create: max_cloud_points=%d outside 1 .. %d", max_cloud_points, MAX_CLOUD);
  if (keyframe_capacity < 1 || keyframe_capacity > MAX_KEYFRAMES)
    return fail(ctx, PR_EINVAL, "pr_submap_create: keyframe_capacity=%d outside 1 .. %d", keyframe_capacity, MAX_KEYFRAMES);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_submap_create: ctx is NULL");
  const Layout l = layout_of(slot_capacity, w_max);
  pr::Owned<pr_submap> g;
  if (int rc = pr::make(ctx, "pr_submap_create", l.total, g)) return rc;
  pr::SubmapView& v = g->v;
  memset(&v, 0, sizeof v);
  v.slot_capacity = slot_capacity; v.w_max = w_max; v.L = 2 * w_max + 1; v.max_cloud_points = max_cloud_points;
  v.keyframe_capacity = keyframe_capacity; v.chunks = pr::submap_chunks(max_cloud_points); v.point_capacity = point_capacity;
  void* b = g->scratch;
  v.row = at<int>(b, l.row); v.dst = at<int>(b, l.dst); v.len = at<int>(b, l.len); v.src = at<long long>(b, l.src);
  v.total = at<int>(b, l.tot); v.flags = at<int>(b, l.flags); v.taken = at<int>(b, l.taken); v.base = at<long long>(b, l.base);
  pr::Transfer t(ctx);
  t.fill(b, 0, l.total);
  return pr::commit(g, t, "pr_submap_create", out);
}

void pr_submap_destroy(pr_submap* g) { pr::destroy(g); }

int pr_submap_build_dev(pr_submap* g, const pr_map_buffers* map, const double* d_poses, const int32_t* d_n, const int32_t* d_center,
                        const int32_t* d_avoid, int32_t c, const pr_submap_params* params, double* out_xyz, int64_t* out_offs, int32_t* out_rows,
                        int32_t* d_info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (int rc = check_build(ctx, g, c, params, "pr_submap_build_dev")) return rc;
  if (!g) return fail(nullptr, PR_EINVAL, "pr_submap_build_dev: handle is NULL");
  if (!map || !map->xyz || !map->offs) return fail(ctx, PR_EINVAL, "pr_submap_build_dev: the map record or one of its buffers is NULL (xyz, offs)");
  if (!d_poses || !d_n || (!d_center && c > 0) || !out_xyz || !out_offs || !out_rows || !d_info)
    return fail(ctx, PR_EINVAL, "pr_submap_build_dev: a required pointer is NULL (d_poses, d_n, d_center, out_xyz, out_offs, out_rows, d_info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::SubmapIn in;
  in.xyz = map->xyz; in.offs = reinterpret_cast<const long long*>(map->offs); in.poses = d_poses; in.n = d_n; in.center = d_center; in.avoid = d_avoid;
  in.c = c;
  pr::SubmapParams prm;
  prm.w = params->half_window; prm.past_only = params->past_only; prm.avoid_gap = params->avoid_gap; prm.max_pts = params->max_pts;
  pr::SubmapOut o;
  o.xyz = out_xyz; o.offs = reinterpret_cast<long long*>(out_offs); o.rows = out_rows; o.info = d_info;
  pr::launch_submap(pr::ctx_stream(ctx), g->v, in, prm, o);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_submap_build(pr_submap* g, const pr_map_buffers* map, const double* d_poses, const int32_t* d_n, const int32_t* center, const int32_t* avoid,
                    int32_t c, const pr_submap_params* params, double* out_xyz, int64_t* out_offs, int32_t* out_rows, int32_t* info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (int rc = check_build(ctx, g, c, params, "pr_submap_build")) return rc;
  if (!g) return fail(nullptr, PR_EINVAL, "pr_submap_build: handle is NULL");
  if (!map || !map->xyz || !map->offs) return fail(ctx, PR_EINVAL, "pr_submap_build: the map record or one of its buffers is NULL (xyz, offs)");
  if (!d_poses || !d_n || (!center && c > 0) || !out_xyz || !out_offs || !out_rows || !info)
    return fail(ctx, PR_EINVAL, "pr_submap_build: a required pointer is NULL (d_poses, d_n, center, out_xyz, out_offs, out_rows, info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  const size_t S = (size_t)g->v.slot_capacity, CB = ((size_t)c * 4 + 15) & ~(size_t)15;
  // the staging of this call: centre, avoid, offs, rows, info, then the points
  const size_t o_cen = 0, o_avoid = o_cen + CB, o_offs = o_avoid + CB, o_rows = o_offs + (((S + 1) * 8 + 15) & ~(size_t)15), o_info = o_rows + S * 8 + 8,
               o_xyz = o_info + 16, bytes = o_xyz + (size_t)g->v.point_capacity * 24;
  void* b = nullptr;
  hipError_t e = hipMalloc(&b, bytes);
  if (e != hipSuccess) return fail(ctx, pr::hip_code(e), "pr_submap_build: staging of %zu bytes: %s", bytes, hipGetErrorString(e));
  pr::Transfer t(ctx);
  t.up(at<int32_t>(b, o_cen), center, (size_t)c * 4);
  t.up_opt(at<int32_t>(b, o_avoid), avoid, (size_t)c * 4);
  t.run([&] {
    return pr_submap_build_dev(g, map, d_poses, d_n, at<int32_t>(b, o_cen), avoid ? at<int32_t>(b, o_avoid) : nullptr, c, params,
                               at<double>(b, o_xyz), at<int64_t>(b, o_offs), at<int32_t>(b, o_rows), at<int32_t>(b, o_info));
  });
  t.down(out_offs, at<int64_t>(b, o_offs), (S + 1) * 8);
  t.down(out_rows, at<int32_t>(b, o_rows), S * 8);
  t.down(info, at<int32_t>(b, o_info), 16);
  t.sync();                                                      // out_offs[c] says how many rows of out_xyz were written
  if (t.ok() && out_offs[c] > 0) t.down(out_xyz, at<double>(b, o_xyz), (size_t)out_offs[c] * 24);
  const int rc = t.finish(ctx, "pr_submap_build");
  (void)hipFree(b);
  return rc;
}

}  // extern "C"
