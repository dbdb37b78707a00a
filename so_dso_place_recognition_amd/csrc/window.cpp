// window.cpp — host side of the resident point window (window.hip): the opaque pr_window with every buffer a push needs,
// the argument checks, the stream-ordered entry points and the host form of a push.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/place_recognition.h"
#include "hash_order.hpp"
#include "handle_core.hpp"
#include "kernels.hpp"

static_assert(pr::WIN_OVERFLOW == PR_WINDOW_OVERFLOW && pr::WIN_ORDER_GLOBAL == PR_WINDOW_ORDER_GLOBAL, "flag bits");

struct pr_window {
  pr_ctx* ctx = nullptr;
  pr::WinView v;
  std::vector<void*> owned;       // every device allocation
  // staging of the host form (pr_window_push)
  double *h_pose = nullptr, *h_xyz = nullptr, *h_oxyz = nullptr, *h_frame = nullptr;
  float *h_int = nullptr, *h_oint = nullptr;
  int* h_n = nullptr;
  int* h_info = nullptr;
  int64_t* h_offs = nullptr;
};

namespace {

using pr::fail;

template <class T>
int dev_alloc(pr_window* w, T*& p, size_t n) {
  void* q = nullptr;
  PR_CHECK_HIP(w->ctx, hipMalloc(&q, (n ? n : 1) * sizeof(T)));
  w->owned.push_back(q);
  p = static_cast<T*>(q);
  return PR_OK;
}

void release(pr_window* w) {
  if (!w) return;
  (void)hipSetDevice(pr::ctx_device(w->ctx));
  (void)hipStreamSynchronize(pr::ctx_stream(w->ctx));
  for (void* p : w->owned) (void)hipFree(p);
  delete w;
}

int build(pr_window* w, double range, int polar, int32_t cap, int32_t max_new, int32_t max_out) {
  pr::WinView& v = w->v;
  memset(&v, 0, sizeof v);
  pr::window_fill_grid(v, range, polar);
  v.cap = cap; v.max_new = max_new; v.max_out = max_out;
  v.C = pr::prestage_cells(range, polar);
  // K <= min(points, cells): the schedule up to there, and the largest bucket count it reaches
  const int kmax = (int)std::min<int64_t>(cap, v.C);
  std::vector<int> scnt, snb;
  pr::probe_bucket_schedule(kmax, scnt, snb);
  if (scnt.empty()) { scnt.push_back(0); snb.push_back(1); }
  v.nsched = (int)scnt.size();
  const size_t nblk = ((size_t)cap + 255) / 256, c = (size_t)cap;
  int *d_scnt = nullptr, *d_snb = nullptr;
#define WN_ALLOC(p, n) { if (int rc = dev_alloc(w, p, n)) return rc; }
  WN_ALLOC(v.st, pr::WIN_STATE_WORDS);
  for (int b = 0; b < 2; b++) { WN_ALLOC(v.xyz[b], 3 * c); WN_ALLOC(v.inten[b], c); }
  WN_ALLOC(v.bcnt, nblk); WN_ALLOC(v.boff, nblk); WN_ALLOC(v.kcnt, nblk); WN_ALLOC(v.koff, nblk);
  WN_ALLOC(v.cell, c); WN_ALLOC(v.val, c);
  WN_ALLOC(v.tval, (size_t)v.C); WN_ALLOC(v.tfirst, (size_t)v.C); WN_ALLOC(v.tbest, (size_t)v.C);
  WN_ALLOC(v.keys, c); WN_ALLOC(v.win, c); WN_ALLOC(v.next, c + 1); WN_ALLOC(v.order, c);
  WN_ALLOC(v.bkt, (size_t)snb.back());
  WN_ALLOC(d_scnt, scnt.size()); WN_ALLOC(d_snb, snb.size());
  WN_ALLOC(w->h_pose, 12); WN_ALLOC(w->h_xyz, 3 * (size_t)max_new); WN_ALLOC(w->h_int, (size_t)max_new); WN_ALLOC(w->h_n, 1);
  WN_ALLOC(w->h_oxyz, 3 * (size_t)max_out); WN_ALLOC(w->h_oint, (size_t)max_out); WN_ALLOC(w->h_offs, 2); WN_ALLOC(w->h_frame, 16);
  WN_ALLOC(w->h_info, 4);
#undef WN_ALLOC
  v.sched_cnt = d_scnt; v.sched_nb = d_snb;
  pr::Transfer t(w->ctx);
  t.up(d_scnt, scnt.data(), scnt.size() * sizeof(int));
  t.up(d_snb, snb.data(), snb.size() * sizeof(int));
  t.fill(v.st, 0, pr::WIN_STATE_WORDS * sizeof(int));
  t.fill(v.tval, 0xFF, (size_t)v.C * 8);                   // "empty"; every push leaves the table so (win_clear_kernel)
  t.fill(v.tfirst, 0xFF, (size_t)v.C * 4);
  t.fill(v.tbest, 0xFF, (size_t)v.C * 4);
  return t.finish(w->ctx, "pr_window_create");             // scnt / snb are this function's locals
}

}  // namespace

extern "C" {

int pr_window_create(pr_ctx* ctx, double lidarRange, int polar, int32_t point_capacity, int32_t max_new_points, int32_t max_out_points,
                     pr_window** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_window_create: out is NULL");
  *out = nullptr;
  if (!(lidarRange > 0.0) || !std::isfinite(lidarRange))
    return fail(ctx, PR_EINVAL, "pr_window_create: lidarRange=%g must be positive and finite", lidarRange);
  if (polar != 0 && polar != 1) return fail(ctx, PR_EINVAL, "pr_window_create: polar=%d is neither 0 nor 1", polar);
  if (point_capacity <= 0 || max_new_points <= 0 || max_out_points <= 0)
    return fail(ctx, PR_EINVAL, "pr_window_create: capacities must be positive (point_capacity=%d, max_new_points=%d, max_out_points=%d)",
                point_capacity, max_new_points, max_out_points);
  if (point_capacity >= (1 << 30)) return fail(ctx, PR_EINVAL, "pr_window_create: point_capacity=%d must be below 2^30", point_capacity);
  if (max_new_points > point_capacity)
    return fail(ctx, PR_EINVAL, "pr_window_create: max_new_points=%d exceeds point_capacity=%d", max_new_points, point_capacity);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_window_create: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_window* w = new (std::nothrow) pr_window;
  if (!w) return fail(ctx, PR_ENOMEM, "out of host memory");
  w->ctx = ctx;
  if (int rc = build(w, lidarRange, polar, point_capacity, max_new_points, max_out_points)) { release(w); return rc; }
  *out = w;
  return PR_OK;
}

void pr_window_destroy(pr_window* w) { release(w); }

int pr_window_reset(pr_window* w) {
  if (!w) return fail(nullptr, PR_EINVAL, "pr_window_reset: window is NULL");
  PR_CHECK_HIP(w->ctx, hipSetDevice(pr::ctx_device(w->ctx)));
  pr::launch_window_reset(pr::ctx_stream(w->ctx), w->v);
  PR_CHECK_HIP(w->ctx, hipGetLastError());
  return PR_OK;
}

int pr_window_count(pr_window* w, int32_t* n_alive) {
  if (!w) return fail(nullptr, PR_EINVAL, "pr_window_count: window is NULL");
  if (!n_alive) return fail(w->ctx, PR_EINVAL, "pr_window_count: n_alive is NULL");
  PR_CHECK_HIP(w->ctx, hipSetDevice(pr::ctx_device(w->ctx)));
  hipStream_t st = pr::ctx_stream(w->ctx);
  PR_CHECK_HIP(w->ctx, hipMemcpyAsync(n_alive, w->v.st, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PR_CHECK_HIP(w->ctx, hipStreamSynchronize(st));
  return PR_OK;
}

int pr_window_push_dev(pr_window* w, const double* pose12, const double* xyz_new, const float* inten_new, const int32_t* n_new_dev,
                       int32_t max_new, double* out_xyz, float* out_inten, int64_t* out_offs, double* out_frame, int32_t* info) {
  if (!w) return fail(nullptr, PR_EINVAL, "pr_window_push_dev: window is NULL");
  if (!pose12 || !xyz_new || !inten_new || !n_new_dev || !out_xyz || !out_inten || !out_offs || !out_frame || !info)
    return fail(w->ctx, PR_EINVAL, "pr_window_push_dev: a required pointer is NULL");
  if (max_new <= 0 || max_new > w->v.max_new)
    return fail(w->ctx, PR_EINVAL, "pr_window_push_dev: max_new=%d outside 1 .. max_new_points=%d", max_new, w->v.max_new);
  PR_CHECK_HIP(w->ctx, hipSetDevice(pr::ctx_device(w->ctx)));
  pr::launch_window_push(pr::ctx_stream(w->ctx), w->v, pose12, xyz_new, inten_new, n_new_dev, max_new, out_xyz, out_inten, out_offs, out_frame,
                         info);
  PR_CHECK_HIP(w->ctx, hipGetLastError());
  return PR_OK;
}

int pr_window_push(pr_window* w, const double* pose12, const double* xyz_new, const float* inten_new, int32_t n_new, double* out_xyz,
                   float* out_inten, int32_t* n_out, double* out_frame, int32_t* info) {
  if (!w) return fail(nullptr, PR_EINVAL, "pr_window_push: window is NULL");
  pr_ctx* ctx = w->ctx;
  if (!pose12 || !out_xyz || !out_inten || !n_out || !out_frame || !info || (n_new > 0 && (!xyz_new || !inten_new)))
    return fail(ctx, PR_EINVAL, "pr_window_push: a required pointer is NULL");
  if (n_new < 0 || n_new > w->v.max_new)
    return fail(ctx, PR_EINVAL, "pr_window_push: n_new=%d outside 0 .. max_new_points=%d", n_new, w->v.max_new);
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::Transfer t(ctx);
  t.up(w->h_pose, pose12, 12 * sizeof(double));
  if (n_new > 0) {
    t.up(w->h_xyz, xyz_new, (size_t)n_new * 24);
    t.up(w->h_int, inten_new, (size_t)n_new * 4);
  }
  t.up(w->h_n, &n_new, sizeof(int));
  t.run([&] {
    return pr_window_push_dev(w, w->h_pose, w->h_xyz, w->h_int, w->h_n, w->v.max_new, w->h_oxyz, w->h_oint, w->h_offs, w->h_frame, w->h_info);
  });
  t.down(info, w->h_info, 4 * sizeof(int));
  t.down(out_frame, w->h_frame, 16 * sizeof(double));
  if (int rc = t.finish(ctx, "pr_window_push")) return rc;
  *n_out = info[1];
  if (*n_out <= 0) return PR_OK;
  t.down(out_xyz, w->h_oxyz, (size_t)*n_out * 24);
  t.down(out_inten, w->h_oint, (size_t)*n_out * 4);
  return t.finish(ctx, "pr_window_push");
}

}  // extern "C"
