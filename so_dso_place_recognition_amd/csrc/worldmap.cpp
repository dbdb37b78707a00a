// worldmap.cpp — host side of the world map (worldmap.hip): the opaque pr_worldmap over the caller's six output buffers and
// a pr_map, its ONE scratch allocation, the argument checks, the stream-ordered fuse and its host form, on the shared handle core
// (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"

static_assert(pr::WORLDMAP_OVERFLOW == PR_WORLDMAP_OVERFLOW && pr::WORLDMAP_SKIPPED == PR_WORLDMAP_SKIPPED &&
              pr::WORLDMAP_RANGE == PR_WORLDMAP_RANGE && pr::WORLDMAP_TABLE == PR_WORLDMAP_TABLE, "flag bits");

// The map's handle as map.cpp defines it, token for token (one definition per translation unit is what the language allows for a class
// that several of them use): the world map reads the map's buffers and capacities and shares its context.
struct pr_map {
  pr_ctx* ctx = nullptr;
  pr::MapView v;
};

struct pr_worldmap : pr::Handle {    // scratch: everything WorldMapView names and the staging of the host form
  pr::WorldMapView v;
  double* stage_poses = nullptr;      // [keyframe_capacity][12]
  int32_t* stage_n = nullptr;         // [4]
  int64_t* stage_info = nullptr;      // [4]
  int32_t max_cloud = 0;              // the map's max_cloud_points (what a pr_mapgrow sizes its launches by)
};

namespace {

using pr::at;
using pr::fail;

// the value checks of a fuse, shared by both forms; they need no device
int check_fuse(pr_worldmap* wm, const char* who, double cell, int32_t min_count, int32_t keep) {
  pr_ctx* ctx = wm ? wm->ctx : nullptr;
  if (!std::isfinite(cell) || !(cell > 0.0)) return fail(ctx, PR_EINVAL, "%s: cell must be finite and positive", who);
  if (min_count < 1) return fail(ctx, PR_EINVAL, "%s: min_count=%d is below 1", who, min_count);
  if (keep != 0 && keep != 1) return fail(ctx, PR_EINVAL, "%s: keep=%d is neither 0 (first) nor 1 (last)", who, keep);
  if (!wm) return fail(nullptr, PR_EINVAL, "%s: world map is NULL", who);
  return PR_OK;
}

// where the parts of the one scratch allocation lie (each on a 16-byte boundary): 20 T + 4 point_capacity + 8 nblk4 + 96 keyframe_capacity
// + 64 bytes and what the rounding adds
struct Layout : pr::Arena { size_t slots, cnt, slot_of, blk, poses, n, info; };

Layout layout_of(int32_t kcap, int64_t pcap) {
  const size_t T = (size_t)1 << pr::worldmap_log2T(pcap), pc = (size_t)pcap, nblk4 = (((pc + 255) / 256) + 3) & ~(size_t)3;
  Layout l;
  l.slots = l.take(16 * T); l.cnt = l.take(4 * T + 16); l.slot_of = l.take(4 * pc); l.blk = l.take(8 * nblk4);
  l.poses = l.take(96 * (size_t)kcap); l.n = l.take(16); l.info = l.take(32);
  return l;
}

}  // namespace

namespace pr {
const WorldMapView* worldmap_view(pr_worldmap* wm) { return wm ? &wm->v : nullptr; }
int worldmap_max_cloud(pr_worldmap* wm) { return wm ? wm->max_cloud : 0; }
pr_ctx* worldmap_ctx(pr_worldmap* wm) { return wm ? wm->ctx : nullptr; }
}  // namespace pr

extern "C" {

int64_t pr_worldmap_scratch_bytes(int32_t keyframe_capacity, int64_t point_capacity) {
  if (keyframe_capacity < 1 || point_capacity < 1 || point_capacity > pr::WORLDMAP_MAX_POINTS) return 0;
  return (int64_t)layout_of(keyframe_capacity, point_capacity).total;
}

int pr_worldmap_create(pr_ctx* ctx, pr_map* map, const pr_worldmap_buffers* buffers, int64_t out_capacity, pr_worldmap** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_worldmap_create: out is NULL");
  *out = nullptr;
  if (!buffers) return fail(ctx, PR_EINVAL, "pr_worldmap_create: buffers is NULL");
  if (!buffers->xyz || !buffers->inten || !buffers->src || !buffers->row || !buffers->count || !buffers->state)
    return fail(ctx, PR_EINVAL, "pr_worldmap_create: a buffer is NULL (xyz, inten, src, row, count, state)");
  if (out_capacity < 1) return fail(ctx, PR_EINVAL, "pr_worldmap_create: out_capacity=%lld is below 1", (long long)out_capacity);
  if (!map) return fail(ctx, PR_EINVAL, "pr_worldmap_create: map is NULL");
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_worldmap_create: ctx is NULL");
  if (map->ctx != ctx) return fail(ctx, PR_EINVAL, "pr_worldmap_create: the map belongs to another context");
  const pr::MapView& m = map->v;
  if (m.pcap > pr::WORLDMAP_MAX_POINTS)
    return fail(ctx, PR_EINVAL, "pr_worldmap_create: the map's point_capacity=%lld exceeds 2^29 (slot indices are int32)", (long long)m.pcap);
  const Layout l = layout_of(m.kcap, m.pcap);
  pr::Owned<pr_worldmap> wm;
  if (int rc = pr::make(ctx, "pr_worldmap_create", l.total, wm)) return rc;
  wm->max_cloud = m.max_cloud;
  pr::WorldMapView& v = wm->v;
  memset(&v, 0, sizeof v);
  v.xyz = buffers->xyz; v.inten = buffers->inten; v.src = buffers->src; v.row = buffers->row; v.count = buffers->count; v.state = buffers->state;
  v.m_xyz = m.xyz; v.m_inten = m.inten; v.m_offs = m.offs; v.m_poses = m.poses; v.m_state = m.state;
  v.kcap = m.kcap; v.pcap = m.pcap; v.ocap = out_capacity;
  v.log2T = pr::worldmap_log2T(m.pcap);
  v.nblk = (int)((m.pcap + 255) / 256);
  const size_t T = (size_t)1 << v.log2T;
  void* b = wm->scratch;
  v.slots = at<unsigned long long>(b, l.slots);
  v.cnt = at<int>(b, l.cnt);
  v.ctl = v.cnt + T;                                      // behind the counts: one memset clears both
  v.slot_of = at<int>(b, l.slot_of); v.blk = at<int>(b, l.blk);
  wm->stage_poses = at<double>(b, l.poses); wm->stage_n = at<int32_t>(b, l.n); wm->stage_info = at<int64_t>(b, l.info);
  pr::Transfer t(ctx);
  t.fill(v.state, 0, 4 * sizeof(int32_t));
  t.fill(b, 0, l.total);
  return pr::commit(wm, t, "pr_worldmap_create", out);
}

// the six buffers are the caller's, the map is the caller's
void pr_worldmap_destroy(pr_worldmap* wm) { pr::destroy(wm); }

int pr_worldmap_count(pr_worldmap* wm, int64_t* rows, int32_t* flags) {
  if (!wm) return fail(nullptr, PR_EINVAL, "pr_worldmap_count: world map is NULL");
  if (!rows || !flags) return fail(wm->ctx, PR_EINVAL, "pr_worldmap_count: a required pointer is NULL");
  int32_t s[4];
  if (int rc = pr::read_state(wm->ctx, "pr_worldmap_count", wm->v.state, s)) return rc;
  *rows = s[0];
  *flags = s[1];
  return PR_OK;
}

int pr_worldmap_fuse_dev(pr_worldmap* wm, const double* d_poses, const int32_t* d_n, double cell, int32_t min_count, int32_t keep,
                         int64_t* d_info) {
  // (the checks that need no handle come first: with wm == NULL their text goes to pr_last_error(NULL))
  const int rc = check_fuse(wm, "pr_worldmap_fuse_dev", cell, min_count, keep);
  if (rc != PR_OK) return rc;
  pr_ctx* ctx = wm->ctx;
  if (!d_info) return fail(ctx, PR_EINVAL, "pr_worldmap_fuse_dev: d_info is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  PR_CHECK_HIP(ctx, pr::launch_worldmap_fuse(pr::ctx_stream(ctx), wm->v, d_poses ? d_poses : wm->v.m_poses, d_n ? d_n : wm->v.m_state, cell,
                                             min_count, keep, d_info));
  return PR_OK;
}

int pr_worldmap_fuse(pr_worldmap* wm, const double* poses, const int32_t* n, double cell, int32_t min_count, int32_t keep, double* xyz,
                     float* inten, int64_t* src, int32_t* row, int32_t* count, int64_t* info) {
  int rc = check_fuse(wm, "pr_worldmap_fuse", cell, min_count, keep);
  if (rc != PR_OK) return rc;
  pr_ctx* ctx = wm->ctx;
  if (!xyz || !inten || !src || !row || !count || !info)
    return fail(ctx, PR_EINVAL, "pr_worldmap_fuse: a required pointer is NULL (xyz, inten, src, row, count, info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  const pr::WorldMapView& v = wm->v;
  pr::Transfer t(ctx);
  t.up_opt(wm->stage_poses, poses, 96 * (size_t)v.kcap);
  t.up_opt(wm->stage_n, n, sizeof(int32_t));
  t.run([&] {
    return pr_worldmap_fuse_dev(wm, poses ? wm->stage_poses : nullptr, n ? wm->stage_n : nullptr, cell, min_count, keep, wm->stage_info);
  });
  t.down(info, wm->stage_info, 4 * sizeof(int64_t));
  rc = t.finish(ctx, "pr_worldmap_fuse");                 // info[0] says how many rows were written
  if (rc != PR_OK) return rc;
  const size_t rows = (size_t)std::min<int64_t>(std::max<int64_t>(info[0], 0), v.ocap);
  if (!rows) return PR_OK;
  t.down(xyz, v.xyz, rows * 24);
  t.down(inten, v.inten, rows * 4);
  t.down(src, v.src, rows * 8);
  t.down(row, v.row, rows * 4);
  t.down(count, v.count, rows * 4);
  return t.finish(ctx, "pr_worldmap_fuse");
}

}  // extern "C"
