// session.cpp — host side of the drive sessions (session.hip): the opaque pr_session over the caller's two buffers, its ONE
// scratch allocation, the argument checks, the stream-ordered entry points and their host forms, and the relaxation across breaks, which
// fills the break array and hands it to the pose graph's own relaxation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/place_recognition.h"
#include "host_common.hpp"
#include "kernels.hpp"
#include "posegraph.hpp"
#include "session.hpp"

static_assert(pr::SESSION_OVERFLOW == PR_SESSION_OVERFLOW && pr::SESSION_REUSED == PR_SESSION_REUSED &&
              pr::SESSION_LOG_OVERFLOW == PR_SESSION_LOG_OVERFLOW, "flag bits");
static_assert(pr::SESSION_POSEGRAPH_OVERFLOW == PR_POSEGRAPH_OVERFLOW, "the log's flag bit");
static_assert(pr::SESSION_ALIGNED == PR_SESSION_ALIGNED && pr::SESSION_NO_TARGET == PR_SESSION_NO_TARGET &&
              pr::SESSION_NO_CANDIDATE == PR_SESSION_NO_CANDIDATE && pr::SESSION_WEAK == PR_SESSION_WEAK &&
              pr::SESSION_NONFINITE == PR_SESSION_NONFINITE, "status values");
static_assert(sizeof(pr_session_align_params) == 24, "two int32 and two doubles, no padding");

struct pr_session {
  pr_ctx* ctx = nullptr;
  pr::SessionView v;
  void* scratch = nullptr;            // one allocation: everything SessionView names and the staging of the host forms
  double* stage_G = nullptr;          // [12]
  double* stage_hyp = nullptr;        // [edge_capacity][12]
  int32_t* stage_support = nullptr;   // [edge_capacity]
  uint8_t* stage_inlier = nullptr;    // [edge_capacity]
  int32_t* stage_info = nullptr;      // [8]
  int32_t* stage_begin = nullptr;     // [4]
};

namespace {

using pr::fail;

constexpr int32_t MAX_NODES = 1 << 20, MAX_EDGES = 65536, MAX_SESSIONS = pr::SESSION_MAX;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout {
  size_t sid, brk, cand, q, hyp, c, p, sup, inl, gd, ctl, s_G, s_hyp, s_support, s_inlier, s_info, s_begin, total;
};

Layout layout_of(int32_t node_capacity, int32_t edge_capacity) {
  const size_t NC = (size_t)node_capacity, EC = (size_t)edge_capacity;
  Layout l;
  l.total = 0;
  auto take = [&l](size_t bytes) { const size_t o = l.total; l.total += (bytes + 15) & ~(size_t)15; return o; };
  l.sid = take(4 * NC); l.brk = take(4 * NC); l.cand = take(4 * EC); l.q = take(4 * EC); l.hyp = take(96 * EC); l.c = take(24 * EC);
  l.p = take(24 * EC); l.sup = take(4 * EC); l.inl = take(4 * EC); l.gd = take(192); l.ctl = take(48);
  l.s_G = take(96); l.s_hyp = take(96 * EC); l.s_support = take(4 * EC); l.s_inlier = take(EC); l.s_info = take(32); l.s_begin = take(16);
  return l;
}

bool sizes_ok(int32_t node_capacity, int32_t edge_capacity, int32_t session_capacity) {
  return node_capacity >= 1 && node_capacity <= MAX_NODES && edge_capacity >= 1 && edge_capacity <= MAX_EDGES && session_capacity >= 1 &&
         session_capacity <= MAX_SESSIONS;
}

bool bound_ok(double b) { return !std::isnan(b) && b >= 0.0; }      // +Inf is allowed: it switches that test off

// the checks of an align that need no device; `who` names the entry point
int align_check(const char* who, pr_session* s, const pr_posegraph_buffers* log, int32_t log_edge_capacity, const double* d_poses_in,
                const int32_t* d_n, const pr_session_align_params* params, double* d_poses_out, const void* G, const void* info) {
  pr_ctx* ctx = s ? s->ctx : nullptr;
  if (!params) return fail(ctx, PR_EINVAL, "%s: params is NULL", who);
  if (params->session < -1) return fail(ctx, PR_EINVAL, "%s: session=%d is below -1", who, params->session);
  if (params->min_inliers < 1) return fail(ctx, PR_EINVAL, "%s: min_inliers=%d is below 1", who, params->min_inliers);
  if (!bound_ok(params->rot_c_max)) return fail(ctx, PR_EINVAL, "%s: rot_c_max is NaN or negative", who);
  if (!bound_ok(params->trans2_max)) return fail(ctx, PR_EINVAL, "%s: trans2_max is NaN or negative", who);
  if (!log) return fail(ctx, PR_EINVAL, "%s: the log's buffer record is NULL", who);
  if (!log->edge_ij || !log->edge_Z || !log->edge_w || !log->state)
    return fail(ctx, PR_EINVAL, "%s: a buffer of the log is NULL (edge_ij, edge_Z, edge_w, state)", who);
  if (!s) return fail(nullptr, PR_EINVAL, "%s: session table is NULL", who);
  if (log_edge_capacity < 1 || log_edge_capacity > s->v.edge_capacity)
    return fail(ctx, PR_EINVAL, "%s: log_edge_capacity=%d outside 1 .. edge_capacity=%d", who, log_edge_capacity, s->v.edge_capacity);
  if (!d_poses_in || !d_n || !d_poses_out || !G || !info)
    return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (d_poses_in, d_n, d_poses_out, G, info)", who);
  return PR_OK;
}

}  // namespace

extern "C" {

size_t pr_session_scratch_bytes(int32_t node_capacity, int32_t edge_capacity, int32_t session_capacity) {
  if (!sizes_ok(node_capacity, edge_capacity, session_capacity)) return 0;
  return layout_of(node_capacity, edge_capacity).total;
}

int pr_session_create(pr_ctx* ctx, const pr_session_buffers* buffers, int32_t node_capacity, int32_t edge_capacity, int32_t session_capacity,
                      pr_session** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_session_create: out is NULL");
  *out = nullptr;
  if (!buffers) return fail(ctx, PR_EINVAL, "pr_session_create: buffers is NULL");
  if (!buffers->start || !buffers->state) return fail(ctx, PR_EINVAL, "pr_session_create: a buffer is NULL (start, state)");
  if (node_capacity < 1 || node_capacity > MAX_NODES)
    return fail(ctx, PR_EINVAL, "pr_session_create: node_capacity=%d outside 1 .. %d", node_capacity, MAX_NODES);
  if (edge_capacity < 1 || edge_capacity > MAX_EDGES)
    return fail(ctx, PR_EINVAL, "pr_session_create: edge_capacity=%d outside 1 .. %d", edge_capacity, MAX_EDGES);
  if (session_capacity < 1 || session_capacity > MAX_SESSIONS)
    return fail(ctx, PR_EINVAL, "pr_session_create: session_capacity=%d outside 1 .. %d", session_capacity, MAX_SESSIONS);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_session_create: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_session* s = new (std::nothrow) pr_session;
  if (!s) return fail(ctx, PR_ENOMEM, "out of host memory");
  s->ctx = ctx;
  pr::SessionView& v = s->v;
  memset(&v, 0, sizeof v);
  v.start = buffers->start; v.state = buffers->state;
  v.node_capacity = node_capacity; v.edge_capacity = edge_capacity; v.session_capacity = session_capacity;
  const Layout l = layout_of(node_capacity, edge_capacity);
  hipError_t e = hipMalloc(&s->scratch, l.total);
  if (e != hipSuccess) {
    delete s;
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_session_create: scratch of %zu bytes: %s", l.total, hipGetErrorString(e));
  }
  char* b = static_cast<char*>(s->scratch);
  auto ip = [b](size_t o) { return reinterpret_cast<int*>(b + o); };
  auto dp = [b](size_t o) { return reinterpret_cast<double*>(b + o); };
  v.sid = ip(l.sid); v.brk = ip(l.brk); v.cand = ip(l.cand); v.q = ip(l.q); v.hyp = dp(l.hyp); v.c = dp(l.c); v.p = dp(l.p);
  v.sup = ip(l.sup); v.inl = ip(l.inl); v.gd = dp(l.gd); v.ctl = ip(l.ctl);
  s->stage_G = dp(l.s_G); s->stage_hyp = dp(l.s_hyp); s->stage_support = ip(l.s_support);
  s->stage_inlier = reinterpret_cast<uint8_t*>(b + l.s_inlier); s->stage_info = ip(l.s_info); s->stage_begin = ip(l.s_begin);
  hipStream_t st = pr::ctx_stream(ctx);
  e = hipMemsetAsync(s->scratch, 0, l.total, st);
  if (e == hipSuccess) {
    pr::launch_session_reset(st, v);                             // S = 1, start[0] = 0
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    (void)hipFree(s->scratch);
    delete s;
    return fail(ctx, PR_EHIP, "pr_session_create: clearing the scratch and the table failed: %s", hipGetErrorString(e));
  }
  *out = s;
  return PR_OK;
}

void pr_session_destroy(pr_session* s) {
  if (!s) return;
  (void)hipSetDevice(pr::ctx_device(s->ctx));
  (void)hipStreamSynchronize(pr::ctx_stream(s->ctx));
  (void)hipFree(s->scratch);          // the two buffers are the caller's
  delete s;
}

int pr_session_reset(pr_session* s) {
  if (!s) return fail(nullptr, PR_EINVAL, "pr_session_reset: session table is NULL");
  PR_CHECK_HIP(s->ctx, hipSetDevice(pr::ctx_device(s->ctx)));
  pr::launch_session_reset(pr::ctx_stream(s->ctx), s->v);
  PR_CHECK_HIP(s->ctx, hipGetLastError());
  return PR_OK;
}

int pr_session_count(pr_session* s, int32_t* sessions, int32_t* flags) {
  if (!s) return fail(nullptr, PR_EINVAL, "pr_session_count: session table is NULL");
  if (!sessions || !flags) return fail(s->ctx, PR_EINVAL, "pr_session_count: a required pointer is NULL");
  PR_CHECK_HIP(s->ctx, hipSetDevice(pr::ctx_device(s->ctx)));
  hipStream_t st = pr::ctx_stream(s->ctx);
  int32_t w[4];
  PR_CHECK_HIP(s->ctx, hipMemcpyAsync(w, s->v.state, sizeof w, hipMemcpyDeviceToHost, st));
  PR_CHECK_HIP(s->ctx, hipStreamSynchronize(st));
  *sessions = w[0];
  *flags = w[1];
  return PR_OK;
}

int pr_session_begin_dev(pr_session* s, const int32_t* d_n, int32_t* d_info) {
  if (!s) return fail(nullptr, PR_EINVAL, "pr_session_begin_dev: session table is NULL");
  pr_ctx* ctx = s->ctx;
  if (!d_n || !d_info) return fail(ctx, PR_EINVAL, "pr_session_begin_dev: a required pointer is NULL (d_n, d_info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_session_begin(pr::ctx_stream(ctx), s->v, d_n, d_info);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_session_begin(pr_session* s, const int32_t* d_n, int32_t* info) {
  if (!s) return fail(nullptr, PR_EINVAL, "pr_session_begin: session table is NULL");
  pr_ctx* ctx = s->ctx;
  if (!d_n || !info) return fail(ctx, PR_EINVAL, "pr_session_begin: a required pointer is NULL (d_n, info)");
  if (int rc = pr_session_begin_dev(s, d_n, s->stage_begin)) return rc;
  hipStream_t st = pr::ctx_stream(ctx);
  hipError_t e = hipMemcpyAsync(info, s->stage_begin, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);                // the host array is in flight until here
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(ctx, pr::hip_code(e), "pr_session_begin: %s", hipGetErrorString(e));
  return PR_OK;
}

int pr_session_align_dev(pr_session* s, const pr_posegraph_buffers* log, int32_t log_edge_capacity, const double* d_poses_in, const int32_t* d_n,
                         const pr_session_align_params* params, double* d_poses_out, double* d_G, double* d_hyp, int32_t* d_support,
                         uint8_t* d_inlier, int32_t* d_info) {
  if (int rc = align_check("pr_session_align_dev", s, log, log_edge_capacity, d_poses_in, d_n, params, d_poses_out, d_G, d_info)) return rc;
  pr_ctx* ctx = s->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  const pr::SessionAlign a = {log->edge_ij, log->edge_Z, log->edge_w, log->state, log_edge_capacity, params->session, params->min_inliers,
                              params->rot_c_max, params->trans2_max};
  pr::launch_session_align(pr::ctx_stream(ctx), s->v, a, d_poses_in, d_n, d_poses_out, d_G, d_hyp, d_support, d_inlier, d_info);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_session_align(pr_session* s, const pr_posegraph_buffers* log, int32_t log_edge_capacity, const double* d_poses_in, const int32_t* d_n,
                     const pr_session_align_params* params, double* d_poses_out, double* G, double* hyp, int32_t* support, uint8_t* inlier,
                     int32_t* info) {
  if (int rc = align_check("pr_session_align", s, log, log_edge_capacity, d_poses_in, d_n, params, d_poses_out, G, info)) return rc;
  pr_ctx* ctx = s->ctx;
  if (int rc = pr_session_align_dev(s, log, log_edge_capacity, d_poses_in, d_n, params, d_poses_out, s->stage_G, hyp ? s->stage_hyp : nullptr,
                                    support ? s->stage_support : nullptr, inlier ? s->stage_inlier : nullptr, s->stage_info))
    return rc;
  hipStream_t st = pr::ctx_stream(ctx);
  const size_t EC = (size_t)s->v.edge_capacity;
  hipError_t e = hipMemcpyAsync(info, s->stage_info, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G, s->stage_G, 12 * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && hyp) e = hipMemcpyAsync(hyp, s->stage_hyp, 96 * EC, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && support) e = hipMemcpyAsync(support, s->stage_support, 4 * EC, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && inlier) e = hipMemcpyAsync(inlier, s->stage_inlier, EC, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);                // the host arrays are in flight until here
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(ctx, pr::hip_code(e), "pr_session_align: %s", hipGetErrorString(e));
  return PR_OK;
}

int pr_session_relax_dev(pr_session* s, pr_posegraph* g, const double* d_poses_in, const int32_t* d_n, const pr_posegraph_params* params,
                         double* d_poses_out, double* d_report) {
  if (int rc = pr::posegraph_relax_check("pr_session_relax_dev", g, d_poses_in, d_n, params, d_poses_out, d_report)) return rc;
  if (!s) return fail(nullptr, PR_EINVAL, "pr_session_relax_dev: session table is NULL");
  pr_ctx* ctx = s->ctx;
  if (pr::posegraph_ctx(g) != ctx) return fail(ctx, PR_EINVAL, "pr_session_relax_dev: the session table and the graph live on two contexts");
  if (pr::posegraph_node_capacity(g) != s->v.node_capacity)
    return fail(ctx, PR_EINVAL, "pr_session_relax_dev: the graph's node_capacity=%d is not the session table's %d", pr::posegraph_node_capacity(g),
                s->v.node_capacity);
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_session_rows(pr::ctx_stream(ctx), s->v);            // the break array, from the table as it stands on the stream
  PR_CHECK_HIP(ctx, hipGetLastError());
  return pr::posegraph_relax_launch(g, d_poses_in, d_n, params, d_poses_out, d_report, s->v.brk);
}

}  // extern "C"
