// session.cpp — host side of the drive sessions (session.hip): the opaque pr_session over the caller's two buffers, its ONE
// scratch allocation, the argument checks, the stream-ordered entry points and their host forms, and the relaxation across breaks, which
// fills the break array and hands it to the pose graph's own relaxation.  Layout, create tail, destroy and copy chains: handle_core.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
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

struct pr_session : pr::Handle {     // scratch: everything SessionView names and the staging of the host forms
  pr::SessionView v;
  double* stage_G = nullptr;          // [12]
  double* stage_hyp = nullptr;        // [edge_capacity][12]
  int32_t* stage_support = nullptr;   // [edge_capacity]
  uint8_t* stage_inlier = nullptr;    // [edge_capacity]
  int32_t* stage_info = nullptr;      // [8]
  int32_t* stage_begin = nullptr;     // [4]
};

namespace {

using pr::at;
using pr::fail;

constexpr int32_t MAX_NODES = 1 << 20, MAX_EDGES = 65536, MAX_SESSIONS = pr::SESSION_MAX;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena {
  size_t sid, brk, cand, q, hyp, c, p, sup, inl, gd, ctl, s_G, s_hyp, s_support, s_inlier, s_info, s_begin;
};

Layout layout_of(int32_t node_capacity, int32_t edge_capacity) {
  const size_t NC = (size_t)node_capacity, EC = (size_t)edge_capacity;
  Layout l;
  l.sid = l.take(4 * NC); l.brk = l.take(4 * NC); l.cand = l.take(4 * EC); l.q = l.take(4 * EC); l.hyp = l.take(96 * EC); l.c = l.take(24 * EC);
  l.p = l.take(24 * EC); l.sup = l.take(4 * EC); l.inl = l.take(4 * EC); l.gd = l.take(192); l.ctl = l.take(48);
  l.s_G = l.take(96); l.s_hyp = l.take(96 * EC); l.s_support = l.take(4 * EC); l.s_inlier = l.take(EC); l.s_info = l.take(32); l.s_begin = l.take(16);
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
  const Layout l = layout_of(node_capacity, edge_capacity);
  pr::Owned<pr_session> s;
  if (int rc = pr::make(ctx, "pr_session_create", l.total, s)) return rc;
  pr::SessionView& v = s->v;
  memset(&v, 0, sizeof v);
  v.start = buffers->start; v.state = buffers->state;
  v.node_capacity = node_capacity; v.edge_capacity = edge_capacity; v.session_capacity = session_capacity;
  void* b = s->scratch;
  v.sid = at<int>(b, l.sid); v.brk = at<int>(b, l.brk); v.cand = at<int>(b, l.cand); v.q = at<int>(b, l.q); v.hyp = at<double>(b, l.hyp);
  v.c = at<double>(b, l.c); v.p = at<double>(b, l.p); v.sup = at<int>(b, l.sup); v.inl = at<int>(b, l.inl); v.gd = at<double>(b, l.gd);
  v.ctl = at<int>(b, l.ctl);
  s->stage_G = at<double>(b, l.s_G); s->stage_hyp = at<double>(b, l.s_hyp); s->stage_support = at<int32_t>(b, l.s_support);
  s->stage_inlier = at<uint8_t>(b, l.s_inlier); s->stage_info = at<int32_t>(b, l.s_info); s->stage_begin = at<int32_t>(b, l.s_begin);
  pr::Transfer t(ctx);
  t.fill(b, 0, l.total);
  if (t.ok()) {
    pr::launch_session_reset(t.st, v);                           // S = 1, start[0] = 0
    t.note(hipGetLastError());
  }
  return pr::commit(s, t, "pr_session_create", out);
}

void pr_session_destroy(pr_session* s) { pr::destroy(s); }      // the two buffers are the caller's

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
  int32_t w[4];
  if (int rc = pr::read_state(s->ctx, "pr_session_count", s->v.state, w)) return rc;
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
  pr::Transfer t(ctx);
  t.run([&] { return pr_session_begin_dev(s, d_n, s->stage_begin); });
  t.down(info, s->stage_begin, 4 * sizeof(int32_t));
  return t.finish(ctx, "pr_session_begin");
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
  const size_t EC = (size_t)s->v.edge_capacity;
  pr::Transfer t(ctx);
  t.run([&] {
    return pr_session_align_dev(s, log, log_edge_capacity, d_poses_in, d_n, params, d_poses_out, s->stage_G, hyp ? s->stage_hyp : nullptr,
                                support ? s->stage_support : nullptr, inlier ? s->stage_inlier : nullptr, s->stage_info);
  });
  t.down(info, s->stage_info, 8 * sizeof(int32_t));
  t.down(G, s->stage_G, 12 * sizeof(double));
  t.down(hyp, s->stage_hyp, 96 * EC);
  t.down(support, s->stage_support, 4 * EC);
  t.down(inlier, s->stage_inlier, EC);
  return t.finish(ctx, "pr_session_align");
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
