// proximity.cpp — host side of the pose-proximity candidate search (proximity.hip): the opaque pr_proximity, its ONE
// scratch allocation, the argument checks, the stream-ordered search and its host form, on the shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"
#include "proximity.hpp"

static_assert(pr::PROX_QRANGE_CLAMPED == PR_PROXIMITY_QRANGE_CLAMPED, "flag bit");
static_assert(sizeof(pr_proximity_params) == 48, "four doubles and four int32, no padding");

struct pr_proximity : pr::Handle {   // scratch: everything ProxView names and the staging of the host form
  pr::ProxView v;
  pr::ProxOut stage;                  // the staging of the host form, [query_capacity k_max] slots
};

namespace {

using pr::at;
using pr::fail;

constexpr int32_t MAX_NODES = 1 << 20, MAX_SLOTS = 65535, MAX_LOG_EDGES = 1 << 20;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena {
  size_t cen, axis, s, valid, part_d2, part_idx, s_idx, s_d2, s_T0, s_src, s_dst, s_known, s_info;
};

Layout layout_of(int32_t node_capacity, int32_t query_capacity, int32_t k_max) {
  const size_t NC = (size_t)node_capacity, QK = (size_t)query_capacity * (size_t)k_max;
  const size_t P = QK * (size_t)pr::prox_runs(node_capacity, query_capacity);
  Layout l;
  l.cen = l.take(24 * NC); l.axis = l.take(24 * NC); l.s = l.take(8 * NC); l.valid = l.take(4 * NC);
  l.part_d2 = l.take(8 * P); l.part_idx = l.take(4 * P);
  l.s_idx = l.take(4 * QK); l.s_d2 = l.take(8 * QK); l.s_T0 = l.take(96 * QK); l.s_src = l.take(4 * QK); l.s_dst = l.take(4 * QK); l.s_known = l.take(QK);
  l.s_info = l.take(16);
  return l;
}

bool sizes_ok(int32_t node_capacity, int32_t query_capacity, int32_t k_max) {
  return node_capacity >= 1 && node_capacity <= MAX_NODES && k_max >= 1 && k_max <= pr::PROX_MAX_K && query_capacity >= 1 &&
         (int64_t)query_capacity * k_max <= MAX_SLOTS;
}

// the value checks of a search, before any device is touched; 0 when acceptable
int check_search(pr_ctx* ctx, const pr_proximity* g, const pr_proximity_params* p, const pr_posegraph_buffers* log, int32_t log_edge_capacity,
                 const void* known, const char* who) {
  if (!p) return fail(ctx, PR_EINVAL, "%s: params is NULL", who);
  if (!std::isfinite(p->radius) || !(p->radius > 0.0)) return fail(ctx, PR_EINVAL, "%s: radius is not finite and positive", who);
  if (!std::isfinite(p->growth) || p->growth < 0.0) return fail(ctx, PR_EINVAL, "%s: growth is negative or not finite", who);
  if (!std::isfinite(p->radius_max) || p->radius_max < p->radius) return fail(ctx, PR_EINVAL, "%s: radius_max is not finite or below radius", who);
  if (!(p->cos_min >= -1.0 && p->cos_min <= 1.0)) return fail(ctx, PR_EINVAL, "%s: cos_min outside -1 .. 1", who);
  if (p->min_gap < 1) return fail(ctx, PR_EINVAL, "%s: min_gap=%d is below 1", who, p->min_gap);
  if (p->stride < 1) return fail(ctx, PR_EINVAL, "%s: stride=%d is below 1", who, p->stride);
  if (p->known_window < 0) return fail(ctx, PR_EINVAL, "%s: known_window=%d is negative", who, p->known_window);
  if (log_edge_capacity < 0 || log_edge_capacity > MAX_LOG_EDGES)
    return fail(ctx, PR_EINVAL, "%s: log_edge_capacity=%d outside 0 .. %d", who, log_edge_capacity, MAX_LOG_EDGES);
  if (log && (!log->edge_ij || !log->state)) return fail(ctx, PR_EINVAL, "%s: a buffer of the closure log is NULL (edge_ij, state)", who);
  if (log && !known) return fail(ctx, PR_EINVAL, "%s: known is NULL with a closure log", who);
  if (g && (p->k < 1 || p->k > g->v.k_max)) return fail(ctx, PR_EINVAL, "%s: k=%d outside 1 .. k_max=%d", who, p->k, g->v.k_max);
  return PR_OK;
}

}  // namespace

extern "C" {

int64_t pr_proximity_scratch_bytes(int32_t node_capacity, int32_t query_capacity, int32_t k_max) {
  if (!sizes_ok(node_capacity, query_capacity, k_max)) return 0;
  return (int64_t)layout_of(node_capacity, query_capacity, k_max).total;
}

void pr_proximity_tile(int32_t* rows, int32_t* cols) {
  if (rows) *rows = pr::PROX_ROWS;
  if (cols) *cols = pr::PROX_COLS;
}

int pr_proximity_create(pr_ctx* ctx, int32_t node_capacity, int32_t query_capacity, int32_t k_max, pr_proximity** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_proximity_create: out is NULL");
  *out = nullptr;
  if (node_capacity < 1 || node_capacity > MAX_NODES)
    return fail(ctx, PR_EINVAL, "pr_proximity_create: node_capacity=%d outside 1 .. %d", node_capacity, MAX_NODES);
  if (k_max < 1 || k_max > pr::PROX_MAX_K) return fail(ctx, PR_EINVAL, "pr_proximity_create: k_max=%d outside 1 .. %d", k_max, pr::PROX_MAX_K);
  if (query_capacity < 1 || (int64_t)query_capacity * k_max > MAX_SLOTS)
    return fail(ctx, PR_EINVAL, "pr_proximity_create: query_capacity=%d is below 1 or query_capacity x k_max exceeds %d", query_capacity, MAX_SLOTS);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_proximity_create: ctx is NULL");
  const Layout l = layout_of(node_capacity, query_capacity, k_max);
  pr::Owned<pr_proximity> g;
  if (int rc = pr::make(ctx, "pr_proximity_create", l.total, g)) return rc;
  pr::ProxView& v = g->v;
  memset(&v, 0, sizeof v);
  memset(&g->stage, 0, sizeof g->stage);
  v.node_capacity = node_capacity; v.query_capacity = query_capacity; v.k_max = k_max; v.runs = pr::prox_runs(node_capacity, query_capacity);
  void* b = g->scratch;
  v.cen = at<double>(b, l.cen); v.axis = at<double>(b, l.axis); v.s = at<double>(b, l.s); v.valid = at<int>(b, l.valid);
  v.part_d2 = at<double>(b, l.part_d2); v.part_idx = at<int>(b, l.part_idx);
  pr::ProxOut& s = g->stage;
  s.idx = at<int>(b, l.s_idx); s.d2 = at<double>(b, l.s_d2); s.T0 = at<double>(b, l.s_T0); s.pair_src = at<int>(b, l.s_src);
  s.pair_dst = at<int>(b, l.s_dst); s.known = at<unsigned char>(b, l.s_known); s.info = at<int>(b, l.s_info);
  pr::Transfer t(ctx);
  t.fill(b, 0, l.total);
  return pr::commit(g, t, "pr_proximity_create", out);
}

void pr_proximity_destroy(pr_proximity* g) { pr::destroy(g); }

int pr_proximity_search_dev(pr_proximity* g, const double* d_poses, const int32_t* d_n, const int32_t* d_qrange, const pr_proximity_params* params,
                            const pr_posegraph_buffers* log, int32_t log_edge_capacity, int32_t* d_idx, double* d_d2, double* d_T0,
                            int32_t* d_pair_src, int32_t* d_pair_dst, uint8_t* d_known, int32_t* d_info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (int rc = check_search(ctx, g, params, log, log_edge_capacity, d_known, "pr_proximity_search_dev")) return rc;
  if (!g) return fail(nullptr, PR_EINVAL, "pr_proximity_search_dev: handle is NULL");
  if (!d_poses || !d_n || !d_qrange || !d_idx || !d_d2 || !d_T0 || !d_pair_src || !d_pair_dst || !d_info)
    return fail(ctx, PR_EINVAL, "pr_proximity_search_dev: a required pointer is NULL (d_poses, d_n, d_qrange, d_idx, d_d2, d_T0, d_pair_src, "
                "d_pair_dst, d_info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::ProxIn in;
  in.poses = d_poses; in.n = d_n; in.qrange = d_qrange;
  in.e_ij = log ? log->edge_ij : nullptr; in.e_state = log ? log->state : nullptr; in.log_edge_capacity = log ? log_edge_capacity : 0;
  pr::ProxParams prm;
  prm.radius = params->radius; prm.growth = params->growth; prm.radius_max = params->radius_max; prm.cos_min = params->cos_min;
  prm.min_gap = params->min_gap; prm.stride = params->stride; prm.k = params->k; prm.known_window = params->known_window;
  pr::ProxOut o;
  o.idx = d_idx; o.d2 = d_d2; o.T0 = d_T0; o.pair_src = d_pair_src; o.pair_dst = d_pair_dst; o.known = d_known; o.info = d_info;
  pr::launch_proximity(pr::ctx_stream(ctx), g->v, in, prm, o);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_proximity_search(pr_proximity* g, const double* d_poses, const int32_t* d_n, const int32_t* d_qrange, const pr_proximity_params* params,
                        const pr_posegraph_buffers* log, int32_t log_edge_capacity, int32_t* idx, double* d2, double* T0, int32_t* pair_src,
                        int32_t* pair_dst, uint8_t* known, int32_t* info) {
  pr_ctx* ctx = g ? g->ctx : nullptr;
  if (int rc = check_search(ctx, g, params, log, log_edge_capacity, known, "pr_proximity_search")) return rc;
  if (!g) return fail(nullptr, PR_EINVAL, "pr_proximity_search: handle is NULL");
  if (!d_poses || !d_n || !d_qrange || !idx || !d2 || !T0 || !pair_src || !pair_dst || !info)
    return fail(ctx, PR_EINVAL, "pr_proximity_search: a required pointer is NULL (d_poses, d_n, d_qrange, idx, d2, T0, pair_src, pair_dst, info)");
  const pr::ProxOut& s = g->stage;
  const size_t QK = (size_t)g->v.query_capacity * (size_t)params->k;
  pr::Transfer t(ctx);
  t.run([&] {
    return pr_proximity_search_dev(g, d_poses, d_n, d_qrange, params, log, log_edge_capacity, s.idx, s.d2, s.T0, s.pair_src, s.pair_dst, s.known,
                                   s.info);
  });
  t.down(idx, s.idx, 4 * QK); t.down(d2, s.d2, 8 * QK); t.down(T0, s.T0, 96 * QK); t.down(pair_src, s.pair_src, 4 * QK);
  t.down(pair_dst, s.pair_dst, 4 * QK); t.down(known, s.known, QK); t.down(info, s.info, 16);
  return t.finish(ctx, "pr_proximity_search");
}

}  // extern "C"
