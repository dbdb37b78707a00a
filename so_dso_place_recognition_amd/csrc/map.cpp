// map.cpp — host side of the resident keyframe map (map.hip): the opaque pr_map over the caller's seven buffers with its
// plan scratch, the argument checks, the stream-ordered entry points, the host form of an append and pr_map_verify_dev = pr_verify_pairs_dev
// over the map's arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"

static_assert(pr::MAP_OVERFLOW == PR_MAP_OVERFLOW && pr::MAP_DROPPED == PR_MAP_DROPPED, "flag bits");

struct pr_map {
  pr_ctx* ctx = nullptr;
  pr::MapView v;
};

namespace {

using pr::at;
using pr::fail;

// offs, frames and state to zero on the stream: what create and reset leave (the invariants of DESIGN.md 4.15)
int clear(pr_map* m) {
  const pr::MapView& v = m->v;
  hipStream_t st = pr::ctx_stream(m->ctx);
  PR_CHECK_HIP(m->ctx, hipMemsetAsync(v.offs, 0, ((size_t)v.kcap + 1) * sizeof(int64_t), st));
  PR_CHECK_HIP(m->ctx, hipMemsetAsync(v.frames, 0, (size_t)v.kcap * 16 * sizeof(double), st));
  PR_CHECK_HIP(m->ctx, hipMemsetAsync(v.state, 0, 4 * sizeof(int32_t), st));
  return PR_OK;
}

// device memory of the host form (pr_map_append), released when it leaves
struct Staging {
  void* p = nullptr;
  ~Staging() { if (p) (void)hipFree(p); }
};

}  // namespace

extern "C" {

int pr_map_create(pr_ctx* ctx, const pr_map_buffers* buffers, int32_t keyframe_capacity, int64_t point_capacity, int32_t max_cloud_points,
                  int32_t max_append, pr_map** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_map_create: out is NULL");
  *out = nullptr;
  if (!buffers) return fail(ctx, PR_EINVAL, "pr_map_create: buffers is NULL");
  if (!buffers->xyz || !buffers->inten || !buffers->offs || !buffers->frames || !buffers->poses || !buffers->ids || !buffers->state)
    return fail(ctx, PR_EINVAL, "pr_map_create: a buffer is NULL (xyz, inten, offs, frames, poses, ids, state)");
  if (keyframe_capacity <= 0 || point_capacity <= 0 || max_cloud_points <= 0 || max_append <= 0)
    return fail(ctx, PR_EINVAL, "pr_map_create: capacities must be positive (keyframe_capacity=%d, point_capacity=%lld, max_cloud_points=%d, "
                "max_append=%d)", keyframe_capacity, (long long)point_capacity, max_cloud_points, max_append);
  if (max_cloud_points > point_capacity)
    return fail(ctx, PR_EINVAL, "pr_map_create: max_cloud_points=%d exceeds point_capacity=%lld", max_cloud_points, (long long)point_capacity);
  if ((int64_t)max_cloud_points * max_append >= ((int64_t)1 << 38))
    return fail(ctx, PR_EINVAL, "pr_map_create: max_cloud_points x max_append = %lld must be below 2^38 (one lane per point of an append)",
                (long long)max_cloud_points * max_append);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_map_create: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_map* m = new (std::nothrow) pr_map;
  if (!m) return fail(ctx, PR_ENOMEM, "out of host memory");
  m->ctx = ctx;
  pr::MapView& v = m->v;
  memset(&v, 0, sizeof v);
  v.xyz = buffers->xyz; v.inten = buffers->inten; v.offs = buffers->offs; v.frames = buffers->frames; v.poses = buffers->poses;
  v.ids = buffers->ids; v.state = buffers->state;
  v.kcap = keyframe_capacity; v.pcap = point_capacity; v.max_cloud = max_cloud_points; v.max_append = max_append;
  void* plan = nullptr;
  hipError_t e = hipMalloc(&plan, pr::map_plan_words(max_append) * sizeof(int64_t));
  if (e != hipSuccess) {
    delete m;
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_map_create: plan scratch: %s", hipGetErrorString(e));
  }
  v.plan = static_cast<int64_t*>(plan);
  int rc = clear(m);
  if (rc == PR_OK && hipStreamSynchronize(pr::ctx_stream(ctx)) != hipSuccess) rc = fail(ctx, PR_EHIP, "pr_map_create: synchronise failed");
  if (rc != PR_OK) { (void)hipFree(plan); delete m; return rc; }
  *out = m;
  return PR_OK;
}

void pr_map_destroy(pr_map* m) {
  if (!m) return;
  (void)hipSetDevice(pr::ctx_device(m->ctx));
  (void)hipStreamSynchronize(pr::ctx_stream(m->ctx));
  (void)hipFree(m->v.plan);             // the seven buffers are the caller's
  delete m;
}

int pr_map_reset(pr_map* m) {
  if (!m) return fail(nullptr, PR_EINVAL, "pr_map_reset: map is NULL");
  PR_CHECK_HIP(m->ctx, hipSetDevice(pr::ctx_device(m->ctx)));
  return clear(m);
}

int pr_map_count(pr_map* m, int32_t* keyframes, int64_t* points, int32_t* flags) {
  if (!m) return fail(nullptr, PR_EINVAL, "pr_map_count: map is NULL");
  if (!keyframes || !points || !flags) return fail(m->ctx, PR_EINVAL, "pr_map_count: a required pointer is NULL");
  int32_t s[4];
  if (int rc = pr::read_state(m->ctx, "pr_map_count", m->v.state, s)) return rc;
  const int32_t k = std::min(std::max(s[0], 0), m->v.kcap);
  pr::Transfer t(m->ctx);
  t.down(points, m->v.offs + k, sizeof(int64_t));
  if (int rc = t.finish(m->ctx, "pr_map_count")) return rc;
  *keyframes = s[0];
  *flags = s[1];
  return PR_OK;
}

int pr_map_append_dev(pr_map* m, const double* d_xyz, const float* d_inten, const int64_t* d_offs, const double* d_frames, const double* d_poses,
                      const int32_t* d_ids, const int32_t* d_emitted, int32_t N, int64_t max_points, int32_t* d_info) {
  // (the checks that need no handle come first: with m == NULL their text goes to pr_last_error(NULL))
  if (N < 0) return fail(m ? m->ctx : nullptr, PR_EINVAL, "pr_map_append_dev: N=%d is negative", N);
  if (max_points < 0) return fail(m ? m->ctx : nullptr, PR_EINVAL, "pr_map_append_dev: max_points=%lld is negative", (long long)max_points);
  if (!m) return fail(nullptr, PR_EINVAL, "pr_map_append_dev: map is NULL");
  if (N > m->v.max_append) return fail(m->ctx, PR_EINVAL, "pr_map_append_dev: N=%d outside 0 .. max_append=%d", N, m->v.max_append);
  if (!d_info || (N > 0 && (!d_offs || !d_frames)) || (N > 0 && max_points > 0 && (!d_xyz || !d_inten)))
    return fail(m->ctx, PR_EINVAL, "pr_map_append_dev: a required pointer is NULL");
  max_points = std::min<int64_t>(max_points, (int64_t)m->v.max_cloud * N);
  PR_CHECK_HIP(m->ctx, hipSetDevice(pr::ctx_device(m->ctx)));
  pr::launch_map_append(pr::ctx_stream(m->ctx), m->v, d_xyz, d_inten, d_offs, d_frames, d_poses, d_ids, d_emitted, N, max_points, d_info);
  PR_CHECK_HIP(m->ctx, hipGetLastError());
  return PR_OK;
}

int pr_map_append(pr_map* m, const double* xyz, const float* inten, const int64_t* offs, const double* frames, const double* poses,
                  const int32_t* ids, const int32_t* emitted, int32_t N, int32_t* info) {
  if (N < 0) return fail(m ? m->ctx : nullptr, PR_EINVAL, "pr_map_append: N=%d is negative", N);
  if (!m) return fail(nullptr, PR_EINVAL, "pr_map_append: map is NULL");
  pr_ctx* ctx = m->ctx;
  if (N > m->v.max_append) return fail(ctx, PR_EINVAL, "pr_map_append: N=%d outside 0 .. max_append=%d", N, m->v.max_append);
  if (!info || (N > 0 && (!offs || !frames))) return fail(ctx, PR_EINVAL, "pr_map_append: a required pointer is NULL");
  int64_t lo = 0, hi = 0;                          // the points any of the N clouds names
  for (int32_t i = 0; i <= N && N > 0; i++) {
    if (offs[i] < 0) return fail(ctx, PR_EINVAL, "pr_map_append: offs[%d]=%lld is negative", i, (long long)offs[i]);
    lo = i ? std::min(lo, offs[i]) : offs[i];
    hi = i ? std::max(hi, offs[i]) : offs[i];
  }
  const int64_t npts = hi - lo;
  if (npts > 0 && (!xyz || !inten)) return fail(ctx, PR_EINVAL, "pr_map_append: a required pointer is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  const size_t n = (size_t)N, np = (size_t)npts;
  pr::Arena a;
  const size_t o_xyz = a.take(np * 24), o_int = a.take(np * 4), o_offs = a.take((n + 1) * 8), o_fr = a.take(n * 128), o_pose = a.take(n * 96),
               o_ids = a.take(n * 4), o_emit = a.take(16), o_info = a.take(16);
  std::unique_ptr<int64_t[]> rel;                  // the offsets counted from the first uploaded point
  if (N > 0) {
    rel.reset(new (std::nothrow) int64_t[n + 1]);
    if (!rel) return fail(ctx, PR_ENOMEM, "out of host memory");
    for (size_t i = 0; i <= n; i++) rel[i] = offs[i] - lo;
  }
  Staging s;                                       // (rel and the staging outlive the synchronise of finish)
  PR_CHECK_HIP(ctx, hipMalloc(&s.p, a.total));
  void* b = s.p;
  pr::Transfer t(ctx);
  if (np) {
    t.up(at<double>(b, o_xyz), xyz + 3 * lo, np * 24);
    t.up(at<float>(b, o_int), inten + lo, np * 4);
  }
  if (N > 0) {
    t.up(at<int64_t>(b, o_offs), rel.get(), (n + 1) * 8);
    t.up(at<double>(b, o_fr), frames, n * 128);
    t.up_opt(at<double>(b, o_pose), poses, n * 96);
    t.up_opt(at<int32_t>(b, o_ids), ids, n * 4);
  }
  t.up_opt(at<int32_t>(b, o_emit), emitted, 4);
  t.run([&] {
    return pr_map_append_dev(m, at<double>(b, o_xyz), at<float>(b, o_int), at<int64_t>(b, o_offs), at<double>(b, o_fr),
                             poses ? at<double>(b, o_pose) : nullptr, ids ? at<int32_t>(b, o_ids) : nullptr,
                             emitted ? at<int32_t>(b, o_emit) : nullptr, N, npts, at<int32_t>(b, o_info));
  });
  t.down(info, at<int32_t>(b, o_info), 16);
  return t.finish(ctx, "pr_map_append");
}

int pr_map_verify_dev(pr_map* m, int type, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_frames_q, int32_t mq,
                      int32_t k, const int32_t* d_idx, const int32_t* d_variant, int32_t variant_stride, int32_t H, int32_t max_src_pts,
                      int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness, int32_t min_inliers, double min_fitness,
                      double max_rmse, double* d_T, pr_icp_stats* d_stats, uint8_t* d_accepted, int32_t* d_hyp) {
  if (!m) return fail(nullptr, PR_EINVAL, "pr_map_verify_dev: map is NULL");
  const pr::MapView& v = m->v;
  return pr_verify_pairs_dev(m->ctx, type, d_xyz_q, d_offs_q, Nq, v.xyz, v.offs, v.kcap, d_frames_q, v.frames, mq, v.kcap, 0, k, d_idx, d_variant,
                             variant_stride, H, max_src_pts, v.max_cloud, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers, min_fitness,
                             max_rmse, d_T, d_stats, d_accepted, d_hyp);
}

}  // extern "C"
