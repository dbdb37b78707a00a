// posegraph.cpp — host side of the loop-closure log and the pose-graph relaxation (posegraph.hip): the opaque pr_posegraph
// over the caller's four buffers with its scratch, the argument checks, the stream-ordered entry points and the host form of an add.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/place_recognition.h"
#include "host_common.hpp"
#include "kernels.hpp"
#include "posegraph.hpp"

static_assert(pr::POSEGRAPH_OVERFLOW == PR_POSEGRAPH_OVERFLOW, "flag bit");
static_assert(sizeof(pr_posegraph_params) == 32, "two int32 and three doubles, no padding");

struct pr_posegraph {
  pr_ctx* ctx = nullptr;
  pr::PoseGraphView v;
  void* scratch = nullptr;            // one allocation: everything PoseGraphView names and the staging of the host form
  int32_t* stage_idx = nullptr;       // [128]
  double* stage_T = nullptr;          // [128][12]
  uint8_t* stage_acc = nullptr;       // [128]
  int32_t* stage_row = nullptr;       // [4]
  int32_t* stage_info = nullptr;      // [4]
  double* stage_w = nullptr;          // [128][2]
};

namespace {

using pr::fail;

constexpr int32_t MAX_NODES = 1 << 20, MAX_EDGES = 1 << 20, MAX_OUTER = 64, MAX_INNER = 1 << 16;
constexpr int32_t MAX_BATCH = 65535;          // most slots of one batch add: pr_icp_pairs_dev's slot limit

bool weight_ok(double w) { return std::isfinite(w) && w >= 0.0; }

}  // namespace

extern "C" {

int pr_posegraph_create(pr_ctx* ctx, const pr_posegraph_buffers* buffers, int32_t node_capacity, int32_t edge_capacity, int32_t max_outer,
                        int32_t max_inner, pr_posegraph** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_posegraph_create: out is NULL");
  *out = nullptr;
  if (!buffers) return fail(ctx, PR_EINVAL, "pr_posegraph_create: buffers is NULL");
  if (!buffers->edge_ij || !buffers->edge_Z || !buffers->edge_w || !buffers->state)
    return fail(ctx, PR_EINVAL, "pr_posegraph_create: a buffer is NULL (edge_ij, edge_Z, edge_w, state)");
  if (node_capacity < 1 || node_capacity > MAX_NODES)
    return fail(ctx, PR_EINVAL, "pr_posegraph_create: node_capacity=%d outside 1 .. %d", node_capacity, MAX_NODES);
  if (edge_capacity < 1 || edge_capacity > MAX_EDGES)
    return fail(ctx, PR_EINVAL, "pr_posegraph_create: edge_capacity=%d outside 1 .. %d", edge_capacity, MAX_EDGES);
  if (max_outer < 1 || max_outer > MAX_OUTER) return fail(ctx, PR_EINVAL, "pr_posegraph_create: max_outer=%d outside 1 .. %d", max_outer, MAX_OUTER);
  if (max_inner < 1 || max_inner > MAX_INNER) return fail(ctx, PR_EINVAL, "pr_posegraph_create: max_inner=%d outside 1 .. %d", max_inner, MAX_INNER);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_posegraph_create: ctx is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_posegraph* g = new (std::nothrow) pr_posegraph;
  if (!g) return fail(ctx, PR_ENOMEM, "out of host memory");
  g->ctx = ctx;
  pr::PoseGraphView& v = g->v;
  memset(&v, 0, sizeof v);
  v.edge_ij = buffers->edge_ij; v.edge_Z = buffers->edge_Z; v.edge_w = buffers->edge_w; v.state = buffers->state;
  v.node_capacity = node_capacity; v.edge_capacity = edge_capacity; v.max_outer = max_outer; v.max_inner = max_inner;
  v.S = node_capacity - 1 + edge_capacity;
  const size_t NC = (size_t)node_capacity, EC = (size_t)edge_capacity, S = (size_t)v.S;
  size_t total = 0;
  auto take = [&total](size_t bytes) { const size_t o = total; total += (bytes + 15) & ~(size_t)15; return o; };
  const size_t o_X = take(NC * 12 * 8), o_zodo = take(NC * 12 * 8), o_jac = take(S * pr::PG_BLOCKS * 8), o_res = take(S * 6 * 8),
               o_wgt = take(S * 2 * 8), o_cost = take(S * 8), o_u = take(S * 6 * 8), o_g = take(NC * 6 * 8), o_x = take(NC * 6 * 8),
               o_r = take(NC * 6 * 8), o_z = take(NC * 6 * 8), o_p = take(NC * 6 * 8), o_q = take(NC * 6 * 8), o_dinv = take(NC * 36 * 8),
               o_valid = take(S * 4), o_fin = take(NC * 4), o_deg = take(NC * 4), o_cur = take(NC * 4), o_off = take((NC + 1) * 4),
               o_raw = take(2 * EC * 4), o_inc = take(2 * EC * 4), o_ctl = take(16), o_sidx = take(pr::POSEGRAPH_MAX_K * 4), o_sT = take(pr::POSEGRAPH_MAX_K * 12 * 8),
               o_sacc = take(pr::POSEGRAPH_MAX_K), o_srow = take(16), o_sinfo = take(16), o_sw = take(pr::POSEGRAPH_MAX_K * 2 * 8);
  hipError_t e = hipMalloc(&g->scratch, total);
  if (e != hipSuccess) {
    delete g;
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_posegraph_create: scratch: %s", hipGetErrorString(e));
  }
  char* b = static_cast<char*>(g->scratch);
  auto dp = [b](size_t o) { return reinterpret_cast<double*>(b + o); };
  auto ip = [b](size_t o) { return reinterpret_cast<int*>(b + o); };
  v.X = dp(o_X); v.zodo = dp(o_zodo); v.jac = dp(o_jac); v.res = dp(o_res); v.wgt = dp(o_wgt); v.cost = dp(o_cost); v.u = dp(o_u);
  v.g = dp(o_g); v.x = dp(o_x); v.r = dp(o_r); v.z = dp(o_z); v.p = dp(o_p); v.q = dp(o_q); v.dinv = dp(o_dinv);
  v.valid = ip(o_valid); v.finite = ip(o_fin); v.deg = ip(o_deg); v.cursor = ip(o_cur); v.inc_off = ip(o_off); v.inc_raw = ip(o_raw); v.inc = ip(o_inc); v.ctl = ip(o_ctl);
  g->stage_idx = ip(o_sidx); g->stage_T = dp(o_sT); g->stage_acc = reinterpret_cast<uint8_t*>(b + o_sacc); g->stage_row = ip(o_srow);
  g->stage_info = ip(o_sinfo); g->stage_w = dp(o_sw);
  hipStream_t st = pr::ctx_stream(ctx);
  e = hipMemsetAsync(v.state, 0, 4 * sizeof(int32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(g->scratch, 0, total, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(g->scratch);
    delete g;
    return fail(ctx, PR_EHIP, "pr_posegraph_create: clearing the state failed: %s", hipGetErrorString(e));
  }
  *out = g;
  return PR_OK;
}

void pr_posegraph_destroy(pr_posegraph* g) {
  if (!g) return;
  (void)hipSetDevice(pr::ctx_device(g->ctx));
  (void)hipStreamSynchronize(pr::ctx_stream(g->ctx));
  (void)hipFree(g->scratch);          // the four buffers are the caller's
  delete g;
}

int pr_posegraph_reset(pr_posegraph* g) {
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraph_reset: graph is NULL");
  PR_CHECK_HIP(g->ctx, hipSetDevice(pr::ctx_device(g->ctx)));
  PR_CHECK_HIP(g->ctx, hipMemsetAsync(g->v.state, 0, 4 * sizeof(int32_t), pr::ctx_stream(g->ctx)));
  return PR_OK;
}

int pr_posegraph_count(pr_posegraph* g, int32_t* edges, int32_t* flags) {
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraph_count: graph is NULL");
  if (!edges || !flags) return fail(g->ctx, PR_EINVAL, "pr_posegraph_count: a required pointer is NULL");
  PR_CHECK_HIP(g->ctx, hipSetDevice(pr::ctx_device(g->ctx)));
  hipStream_t st = pr::ctx_stream(g->ctx);
  int32_t s[4];
  PR_CHECK_HIP(g->ctx, hipMemcpyAsync(s, g->v.state, sizeof s, hipMemcpyDeviceToHost, st));
  PR_CHECK_HIP(g->ctx, hipStreamSynchronize(st));
  *edges = s[0];
  *flags = s[1];
  return PR_OK;
}

int pr_posegraph_add_dev(pr_posegraph* g, const int32_t* d_idx, const double* d_T, const uint8_t* d_accepted, const int32_t* d_query_row, int32_t k,
                         double w_rot, double w_trans, int32_t* d_info) {
  // (the checks that need no handle come first: with g == NULL their text goes to pr_last_error(NULL))
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (k < 1 || k > pr::POSEGRAPH_MAX_K) return fail(ctx, PR_EINVAL, "pr_posegraph_add_dev: k=%d outside 1 .. %d", k, pr::POSEGRAPH_MAX_K);
  if (!weight_ok(w_rot)) return fail(ctx, PR_EINVAL, "pr_posegraph_add_dev: w_rot is negative or not finite");
  if (!weight_ok(w_trans)) return fail(ctx, PR_EINVAL, "pr_posegraph_add_dev: w_trans is negative or not finite");
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraph_add_dev: graph is NULL");
  if (!d_idx || !d_T || !d_accepted || !d_query_row || !d_info)
    return fail(ctx, PR_EINVAL, "pr_posegraph_add_dev: a required pointer is NULL (d_idx, d_T, d_accepted, d_query_row, d_info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_posegraph_add(pr::ctx_stream(ctx), g->v, d_idx, d_T, d_accepted, d_query_row, k, w_rot, w_trans, d_info);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_posegraph_add(pr_posegraph* g, const int32_t* idx, const double* T, const uint8_t* accepted, int32_t query_row, int32_t k, double w_rot,
                     double w_trans, int32_t* info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (k < 1 || k > pr::POSEGRAPH_MAX_K) return fail(ctx, PR_EINVAL, "pr_posegraph_add: k=%d outside 1 .. %d", k, pr::POSEGRAPH_MAX_K);
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraph_add: graph is NULL");
  if (!idx || !T || !accepted || !info) return fail(ctx, PR_EINVAL, "pr_posegraph_add: a required pointer is NULL (idx, T, accepted, info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const int32_t row[4] = {query_row, 0, 0, 0};
  hipError_t e = hipMemcpyAsync(g->stage_idx, idx, (size_t)k * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->stage_T, T, (size_t)k * 12 * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->stage_acc, accepted, (size_t)k, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->stage_row, row, sizeof row, hipMemcpyHostToDevice, st);
  int rc = PR_OK;
  if (e == hipSuccess) rc = pr_posegraph_add_dev(g, g->stage_idx, g->stage_T, g->stage_acc, g->stage_row, k, w_rot, w_trans, g->stage_info);
  if (e == hipSuccess && rc == PR_OK) e = hipMemcpyAsync(info, g->stage_info, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);     // the host arrays are in flight until here
  if (rc != PR_OK) return rc;
  PR_CHECK_HIP(ctx, e);
  PR_CHECK_HIP(ctx, e2);
  return PR_OK;
}

int pr_posegraphw_add_dev(pr_posegraph* g, const int32_t* d_idx, const double* d_T, const uint8_t* d_accepted, const int32_t* d_query_row,
                                  int32_t k, const double* d_w, int32_t* d_info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (k < 1 || k > pr::POSEGRAPH_MAX_K) return fail(ctx, PR_EINVAL, "pr_posegraphw_add_dev: k=%d outside 1 .. %d", k, pr::POSEGRAPH_MAX_K);
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraphw_add_dev: graph is NULL");
  if (!d_idx || !d_T || !d_accepted || !d_query_row || !d_w || !d_info)
    return fail(ctx, PR_EINVAL, "pr_posegraphw_add_dev: a required pointer is NULL (d_idx, d_T, d_accepted, d_query_row, d_w, d_info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_posegraph_add_weighted(pr::ctx_stream(ctx), g->v, d_idx, d_T, d_accepted, d_query_row, k, d_w, d_info);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_posegraphw_add(pr_posegraph* g, const int32_t* idx, const double* T, const uint8_t* accepted, int32_t query_row, int32_t k,
                              const double* w, int32_t* info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (k < 1 || k > pr::POSEGRAPH_MAX_K) return fail(ctx, PR_EINVAL, "pr_posegraphw_add: k=%d outside 1 .. %d", k, pr::POSEGRAPH_MAX_K);
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraphw_add: graph is NULL");
  if (!idx || !T || !accepted || !w || !info)
    return fail(ctx, PR_EINVAL, "pr_posegraphw_add: a required pointer is NULL (idx, T, accepted, w, info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const int32_t row[4] = {query_row, 0, 0, 0};
  hipError_t e = hipMemcpyAsync(g->stage_idx, idx, (size_t)k * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->stage_T, T, (size_t)k * 12 * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->stage_acc, accepted, (size_t)k, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->stage_row, row, sizeof row, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->stage_w, w, (size_t)k * 2 * 8, hipMemcpyHostToDevice, st);
  int rc = PR_OK;
  if (e == hipSuccess) rc = pr_posegraphw_add_dev(g, g->stage_idx, g->stage_T, g->stage_acc, g->stage_row, k, g->stage_w, g->stage_info);
  if (e == hipSuccess && rc == PR_OK) e = hipMemcpyAsync(info, g->stage_info, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);     // the host arrays are in flight until here
  if (rc != PR_OK) return rc;
  PR_CHECK_HIP(ctx, e);
  PR_CHECK_HIP(ctx, e2);
  return PR_OK;
}

int pr_posegraphb_add_dev(pr_posegraph* g, const int32_t* d_i, const int32_t* d_j, const double* d_T, const uint8_t* d_accepted, const double* d_w,
                          double w_rot, double w_trans, int32_t c, int32_t* d_info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (c < 1 || c > MAX_BATCH) return fail(ctx, PR_EINVAL, "pr_posegraphb_add_dev: c=%d outside 1 .. %d", c, MAX_BATCH);
  if (!weight_ok(w_rot)) return fail(ctx, PR_EINVAL, "pr_posegraphb_add_dev: w_rot is negative or not finite");
  if (!weight_ok(w_trans)) return fail(ctx, PR_EINVAL, "pr_posegraphb_add_dev: w_trans is negative or not finite");
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraphb_add_dev: graph is NULL");
  if (!d_i || !d_j || !d_T || !d_accepted || !d_info)
    return fail(ctx, PR_EINVAL, "pr_posegraphb_add_dev: a required pointer is NULL (d_i, d_j, d_T, d_accepted, d_info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_posegraph_add_batch(pr::ctx_stream(ctx), g->v, d_i, d_j, d_T, d_accepted, d_w, w_rot, w_trans, c, d_info);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

// the host form stages c slots, more than the create-time staging of the single adds holds: it allocates for the call and frees behind
// its synchronise (the device form allocates nothing)
int pr_posegraphb_add(pr_posegraph* g, const int32_t* i, const int32_t* j, const double* T, const uint8_t* accepted, const double* w, double w_rot,
                      double w_trans, int32_t c, int32_t* info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (c < 1 || c > MAX_BATCH) return fail(ctx, PR_EINVAL, "pr_posegraphb_add: c=%d outside 1 .. %d", c, MAX_BATCH);
  if (!weight_ok(w_rot)) return fail(ctx, PR_EINVAL, "pr_posegraphb_add: w_rot is negative or not finite");
  if (!weight_ok(w_trans)) return fail(ctx, PR_EINVAL, "pr_posegraphb_add: w_trans is negative or not finite");
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraphb_add: graph is NULL");
  if (!i || !j || !T || !accepted || !info) return fail(ctx, PR_EINVAL, "pr_posegraphb_add: a required pointer is NULL (i, j, T, accepted, info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const size_t C = (size_t)c, o_T = 0, o_w = o_T + C * 96, o_i = o_w + C * 16, o_j = o_i + C * 4, o_info = o_j + C * 4, o_acc = o_info + 16;
  char* b = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&b), o_acc + C);
  if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_posegraphb_add: staging: %s", hipGetErrorString(e));
  e = hipMemcpyAsync(b + o_T, T, C * 96, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && w) e = hipMemcpyAsync(b + o_w, w, C * 16, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(b + o_i, i, C * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(b + o_j, j, C * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(b + o_acc, accepted, C, hipMemcpyHostToDevice, st);
  int rc = PR_OK;
  if (e == hipSuccess)
    rc = pr_posegraphb_add_dev(g, reinterpret_cast<int32_t*>(b + o_i), reinterpret_cast<int32_t*>(b + o_j), reinterpret_cast<double*>(b + o_T),
                               reinterpret_cast<uint8_t*>(b + o_acc), w ? reinterpret_cast<double*>(b + o_w) : nullptr, w_rot, w_trans, c,
                               reinterpret_cast<int32_t*>(b + o_info));
  if (e == hipSuccess && rc == PR_OK) e = hipMemcpyAsync(info, b + o_info, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);     // the host arrays are in flight until here
  (void)hipFree(b);
  if (rc != PR_OK) return rc;
  PR_CHECK_HIP(ctx, e);
  PR_CHECK_HIP(ctx, e2);
  return PR_OK;
}

int pr_posegraph_relax_dev(pr_posegraph* g, const double* d_poses_in, const int32_t* d_n, const pr_posegraph_params* params, double* d_poses_out,
                           double* d_report) {
  if (int rc = pr::posegraph_relax_check("pr_posegraph_relax_dev", g, d_poses_in, d_n, params, d_poses_out, d_report)) return rc;
  return pr::posegraph_relax_launch(g, d_poses_in, d_n, params, d_poses_out, d_report, nullptr);
}

}  // extern "C"

namespace pr {

int posegraph_relax_check(const char* who, pr_posegraph* g, const double* d_poses_in, const int32_t* d_n, const pr_posegraph_params* params,
                          double* d_poses_out, double* d_report) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (!params) return fail(ctx, PR_EINVAL, "%s: params is NULL", who);
  if (params->outer < 1) return fail(ctx, PR_EINVAL, "%s: outer=%d is below 1", who, params->outer);
  if (params->inner < 1) return fail(ctx, PR_EINVAL, "%s: inner=%d is below 1", who, params->inner);
  if (!weight_ok(params->lambda)) return fail(ctx, PR_EINVAL, "%s: lambda is negative or not finite", who);
  if (!weight_ok(params->w_odo_rot)) return fail(ctx, PR_EINVAL, "%s: w_odo_rot is negative or not finite", who);
  if (!weight_ok(params->w_odo_trans)) return fail(ctx, PR_EINVAL, "%s: w_odo_trans is negative or not finite", who);
  if (!g) return fail(nullptr, PR_EINVAL, "%s: graph is NULL", who);
  if (params->outer > g->v.max_outer) return fail(ctx, PR_EINVAL, "%s: outer=%d outside 1 .. max_outer=%d", who, params->outer, g->v.max_outer);
  if (params->inner > g->v.max_inner) return fail(ctx, PR_EINVAL, "%s: inner=%d outside 1 .. max_inner=%d", who, params->inner, g->v.max_inner);
  if (!d_poses_in || !d_n || !d_poses_out || !d_report)
    return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (d_poses_in, d_n, d_poses_out, d_report)", who);
  return PR_OK;
}

int posegraph_relax_launch(pr_posegraph* g, const double* d_poses_in, const int32_t* d_n, const pr_posegraph_params* params,
                           double* d_poses_out, double* d_report, const int* d_brk) {
  pr_ctx* ctx = g->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  const pr::PoseGraphParams prm = {params->outer, params->inner, params->lambda, params->w_odo_rot, params->w_odo_trans};
  pr::launch_posegraph_relax(pr::ctx_stream(ctx), g->v, d_poses_in, d_n, prm, d_poses_out, d_report, d_brk);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

pr_ctx* posegraph_ctx(pr_posegraph* g) { return g->ctx; }
int posegraph_node_capacity(pr_posegraph* g) { return g->v.node_capacity; }

}  // namespace pr
