// posegraph.cpp — host side of the loop-closure log and the pose-graph relaxation (posegraph.hip): the opaque pr_posegraph
// over the caller's four buffers with its scratch, the argument checks, the stream-ordered entry points and the host forms of an add, on
// the shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"
#include "posegraph.hpp"

static_assert(pr::POSEGRAPH_OVERFLOW == PR_POSEGRAPH_OVERFLOW, "flag bit");
static_assert(sizeof(pr_posegraph_params) == 32, "two int32 and three doubles, no padding");

struct pr_posegraph : pr::Handle {   // scratch: everything PoseGraphView names and the staging of the host form
  pr::PoseGraphView v;
  int32_t* stage_idx = nullptr;       // [128]
  double* stage_T = nullptr;          // [128][12]
  uint8_t* stage_acc = nullptr;       // [128]
  int32_t* stage_row = nullptr;       // [4]
  int32_t* stage_info = nullptr;      // [4]
  double* stage_w = nullptr;          // [128][2]
};

namespace {

using pr::at;
using pr::fail;

constexpr int32_t MAX_NODES = 1 << 20, MAX_EDGES = 1 << 20, MAX_OUTER = 64, MAX_INNER = 1 << 16;
constexpr int32_t MAX_BATCH = 65535;          // most slots of one batch add: pr_icp_pairs_dev's slot limit

bool weight_ok(double w) { return std::isfinite(w) && w >= 0.0; }

// the uploads the two single adds share: k slots and the four-word query row (the caller's, alive until its finish) into the create-time staging
void stage_slots(pr::Transfer& t, pr_posegraph* g, const int32_t* idx, const double* T, const uint8_t* accepted, const int32_t* row, int32_t k) {
  t.up(g->stage_idx, idx, (size_t)k * 4);
  t.up(g->stage_T, T, (size_t)k * 12 * 8);
  t.up(g->stage_acc, accepted, (size_t)k);
  t.up(g->stage_row, row, 4 * sizeof(int32_t));
}

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
  const size_t NC = (size_t)node_capacity, EC = (size_t)edge_capacity, S = NC - 1 + EC;
  pr::Arena a;
  const size_t o_X = a.take(NC * 12 * 8), o_zodo = a.take(NC * 12 * 8), o_jac = a.take(S * pr::PG_BLOCKS * 8), o_res = a.take(S * 6 * 8),
               o_wgt = a.take(S * 2 * 8), o_cost = a.take(S * 8), o_u = a.take(S * 6 * 8), o_g = a.take(NC * 6 * 8), o_x = a.take(NC * 6 * 8),
               o_r = a.take(NC * 6 * 8), o_z = a.take(NC * 6 * 8), o_p = a.take(NC * 6 * 8), o_q = a.take(NC * 6 * 8), o_dinv = a.take(NC * 36 * 8),
               o_valid = a.take(S * 4), o_fin = a.take(NC * 4), o_deg = a.take(NC * 4), o_cur = a.take(NC * 4), o_off = a.take((NC + 1) * 4),
               o_raw = a.take(2 * EC * 4), o_inc = a.take(2 * EC * 4), o_ctl = a.take(16), o_sidx = a.take(pr::POSEGRAPH_MAX_K * 4),
               o_sT = a.take(pr::POSEGRAPH_MAX_K * 12 * 8), o_sacc = a.take(pr::POSEGRAPH_MAX_K), o_srow = a.take(16), o_sinfo = a.take(16),
               o_sw = a.take(pr::POSEGRAPH_MAX_K * 2 * 8);
  pr::Owned<pr_posegraph> g;
  if (int rc = pr::make(ctx, "pr_posegraph_create", a.total, g)) return rc;
  pr::PoseGraphView& v = g->v;
  memset(&v, 0, sizeof v);
  v.edge_ij = buffers->edge_ij; v.edge_Z = buffers->edge_Z; v.edge_w = buffers->edge_w; v.state = buffers->state;
  v.node_capacity = node_capacity; v.edge_capacity = edge_capacity; v.max_outer = max_outer; v.max_inner = max_inner;
  v.S = node_capacity - 1 + edge_capacity;
  void* b = g->scratch;
  v.X = at<double>(b, o_X); v.zodo = at<double>(b, o_zodo); v.jac = at<double>(b, o_jac); v.res = at<double>(b, o_res);
  v.wgt = at<double>(b, o_wgt); v.cost = at<double>(b, o_cost); v.u = at<double>(b, o_u); v.g = at<double>(b, o_g); v.x = at<double>(b, o_x);
  v.r = at<double>(b, o_r); v.z = at<double>(b, o_z); v.p = at<double>(b, o_p); v.q = at<double>(b, o_q); v.dinv = at<double>(b, o_dinv);
  v.valid = at<int>(b, o_valid); v.finite = at<int>(b, o_fin); v.deg = at<int>(b, o_deg); v.cursor = at<int>(b, o_cur);
  v.inc_off = at<int>(b, o_off); v.inc_raw = at<int>(b, o_raw); v.inc = at<int>(b, o_inc); v.ctl = at<int>(b, o_ctl);
  g->stage_idx = at<int32_t>(b, o_sidx); g->stage_T = at<double>(b, o_sT); g->stage_acc = at<uint8_t>(b, o_sacc);
  g->stage_row = at<int32_t>(b, o_srow); g->stage_info = at<int32_t>(b, o_sinfo); g->stage_w = at<double>(b, o_sw);
  pr::Transfer t(ctx);
  t.fill(v.state, 0, 4 * sizeof(int32_t));
  t.fill(b, 0, a.total);
  return pr::commit(g, t, "pr_posegraph_create", out);
}

void pr_posegraph_destroy(pr_posegraph* g) { pr::destroy(g); }  // the four buffers are the caller's

int pr_posegraph_reset(pr_posegraph* g) {
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraph_reset: graph is NULL");
  return pr::clear_state(g->ctx, g->v.state);
}

int pr_posegraph_count(pr_posegraph* g, int32_t* edges, int32_t* flags) {
  if (!g) return fail(nullptr, PR_EINVAL, "pr_posegraph_count: graph is NULL");
  if (!edges || !flags) return fail(g->ctx, PR_EINVAL, "pr_posegraph_count: a required pointer is NULL");
  int32_t s[4];
  if (int rc = pr::read_state(g->ctx, "pr_posegraph_count", g->v.state, s)) return rc;
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
  const int32_t row[4] = {query_row, 0, 0, 0};
  pr::Transfer t(ctx);
  stage_slots(t, g, idx, T, accepted, row, k);
  t.run([&] { return pr_posegraph_add_dev(g, g->stage_idx, g->stage_T, g->stage_acc, g->stage_row, k, w_rot, w_trans, g->stage_info); });
  t.down(info, g->stage_info, 4 * sizeof(int32_t));
  return t.finish(ctx, "pr_posegraph_add");
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
  const int32_t row[4] = {query_row, 0, 0, 0};
  pr::Transfer t(ctx);
  stage_slots(t, g, idx, T, accepted, row, k);
  t.up(g->stage_w, w, (size_t)k * 2 * 8);
  t.run([&] { return pr_posegraphw_add_dev(g, g->stage_idx, g->stage_T, g->stage_acc, g->stage_row, k, g->stage_w, g->stage_info); });
  t.down(info, g->stage_info, 4 * sizeof(int32_t));
  return t.finish(ctx, "pr_posegraphw_add");
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
  const size_t C = (size_t)c, o_T = 0, o_w = o_T + C * 96, o_i = o_w + C * 16, o_j = o_i + C * 4, o_info = o_j + C * 4, o_acc = o_info + 16;
  void* b = nullptr;
  const hipError_t e = hipMalloc(&b, o_acc + C);
  if (e != hipSuccess) return fail(ctx, pr::hip_code(e), "pr_posegraphb_add: staging of %zu bytes: %s", o_acc + C, hipGetErrorString(e));
  pr::Transfer t(ctx);
  t.up(at<double>(b, o_T), T, C * 96);
  t.up_opt(at<double>(b, o_w), w, C * 16);
  t.up(at<int32_t>(b, o_i), i, C * 4);
  t.up(at<int32_t>(b, o_j), j, C * 4);
  t.up(at<uint8_t>(b, o_acc), accepted, C);
  t.run([&] {
    return pr_posegraphb_add_dev(g, at<int32_t>(b, o_i), at<int32_t>(b, o_j), at<double>(b, o_T), at<uint8_t>(b, o_acc),
                                 w ? at<double>(b, o_w) : nullptr, w_rot, w_trans, c, at<int32_t>(b, o_info));
  });
  t.down(info, at<int32_t>(b, o_info), 4 * sizeof(int32_t));
  const int rc = t.finish(ctx, "pr_posegraphb_add");
  (void)hipFree(b);                                   // behind the synchronise
  return rc;
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
