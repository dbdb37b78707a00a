// gate.cpp — host side of the closure consistency gate (gate.hip): the opaque pr_gate over the buffer records of two
// loop-closure logs, its ONE scratch allocation with the two tables, the argument checks, the stream-ordered run and its host form, on the
// shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "gate.hpp"
#include "handle_core.hpp"
#include "kernels.hpp"

static_assert(pr::GATE_SRC_OVERFLOW == PR_GATE_SRC_OVERFLOW && pr::GATE_UNSETTLED == PR_GATE_UNSETTLED, "flag bits");
static_assert(pr::GATE_LOG_OVERFLOW == PR_POSEGRAPH_OVERFLOW, "the source log's flag bit");
static_assert(sizeof(pr_gate_params) == 12, "three int32, no padding");

struct pr_gate : pr::Handle {        // scratch: everything GateView names and the staging of the host form
  pr::GateView v;
  uint8_t* stage_keep = nullptr;      // [edge_capacity]
  int32_t* stage_support = nullptr;   // [edge_capacity]
  int32_t* stage_map = nullptr;       // [edge_capacity]
  int32_t* stage_info = nullptr;      // [4]
};

namespace {

using pr::at;
using pr::fail;

constexpr int32_t MAX_NODES = 1 << 20, MAX_EDGES = 65536, MAX_GAP = 65535, MAX_ROUNDS = 64;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena {
  size_t lmn, eij, valid, keep0, keep1, sup, map, rot, trans, ctl, s_keep, s_support, s_map, s_info;
};

Layout layout_of(int32_t edge_capacity, int32_t max_gap) {
  const size_t EC = (size_t)edge_capacity, G = (size_t)max_gap + 1;
  Layout l;
  l.lmn = l.take(8 * pr::GATE_LMN * EC); l.eij = l.take(8 * EC); l.valid = l.take(4 * EC); l.keep0 = l.take(4 * EC); l.keep1 = l.take(4 * EC);
  l.sup = l.take(4 * EC); l.map = l.take(4 * EC); l.rot = l.take(8 * G); l.trans = l.take(8 * G); l.ctl = l.take(16);
  l.s_keep = l.take(EC); l.s_support = l.take(4 * EC); l.s_map = l.take(4 * EC); l.s_info = l.take(16);
  return l;
}

bool sizes_ok(int32_t node_capacity, int32_t edge_capacity, int32_t max_gap) {
  return node_capacity >= 1 && node_capacity <= MAX_NODES && edge_capacity >= 1 && edge_capacity <= MAX_EDGES && max_gap >= 0 && max_gap <= MAX_GAP;
}

}  // namespace

extern "C" {

size_t pr_gate_scratch_bytes(int32_t node_capacity, int32_t edge_capacity, int32_t max_gap) {
  if (!sizes_ok(node_capacity, edge_capacity, max_gap)) return 0;
  return layout_of(edge_capacity, max_gap).total;
}

int pr_gate_create(pr_ctx* ctx, const pr_posegraph_buffers* src, const pr_posegraph_buffers* dst, int32_t node_capacity, int32_t edge_capacity,
                   int32_t dst_edge_capacity, const pr_gate_params* params, const double* rot_tab, const double* trans2_tab, pr_gate** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_gate_create: out is NULL");
  *out = nullptr;
  if (!src || !dst) return fail(ctx, PR_EINVAL, "pr_gate_create: a buffer record is NULL (src, dst)");
  if (!params || !rot_tab || !trans2_tab) return fail(ctx, PR_EINVAL, "pr_gate_create: a required pointer is NULL (params, rot_tab, trans2_tab)");
  const void* sb[4] = {src->edge_ij, src->edge_Z, src->edge_w, src->state};
  const void* db[4] = {dst->edge_ij, dst->edge_Z, dst->edge_w, dst->state};
  for (int a = 0; a < 4; a++)
    if (!sb[a] || !db[a]) return fail(ctx, PR_EINVAL, "pr_gate_create: a buffer is NULL (edge_ij, edge_Z, edge_w, state of src and dst)");
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++)
      if (sb[a] == db[b]) return fail(ctx, PR_EINVAL, "pr_gate_create: src and dst share a buffer");
  if (node_capacity < 1 || node_capacity > MAX_NODES)
    return fail(ctx, PR_EINVAL, "pr_gate_create: node_capacity=%d outside 1 .. %d", node_capacity, MAX_NODES);
  if (edge_capacity < 1 || edge_capacity > MAX_EDGES)
    return fail(ctx, PR_EINVAL, "pr_gate_create: edge_capacity=%d outside 1 .. %d", edge_capacity, MAX_EDGES);
  if (dst_edge_capacity < edge_capacity)
    return fail(ctx, PR_EINVAL, "pr_gate_create: dst_edge_capacity=%d is below edge_capacity=%d", dst_edge_capacity, edge_capacity);
  if (params->max_gap < 0 || params->max_gap > MAX_GAP) return fail(ctx, PR_EINVAL, "pr_gate_create: max_gap=%d outside 0 .. %d", params->max_gap, MAX_GAP);
  if (params->min_support < 0) return fail(ctx, PR_EINVAL, "pr_gate_create: min_support=%d is negative", params->min_support);
  if (params->rounds < 1 || params->rounds > MAX_ROUNDS) return fail(ctx, PR_EINVAL, "pr_gate_create: rounds=%d outside 1 .. %d", params->rounds, MAX_ROUNDS);
  for (int32_t g = 0; g <= params->max_gap; g++) {               // +Inf is allowed: it switches that test off
    if (std::isnan(rot_tab[g]) || rot_tab[g] < 0.0) return fail(ctx, PR_EINVAL, "pr_gate_create: rot_tab[%d] is NaN or negative", g);
    if (std::isnan(trans2_tab[g]) || trans2_tab[g] < 0.0) return fail(ctx, PR_EINVAL, "pr_gate_create: trans2_tab[%d] is NaN or negative", g);
  }
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_gate_create: ctx is NULL");
  const Layout l = layout_of(edge_capacity, params->max_gap);
  pr::Owned<pr_gate> g;
  if (int rc = pr::make(ctx, "pr_gate_create", l.total, g)) return rc;
  pr::GateView& v = g->v;
  memset(&v, 0, sizeof v);
  v.s_ij = src->edge_ij; v.s_Z = src->edge_Z; v.s_w = src->edge_w; v.s_state = src->state;
  v.d_ij = dst->edge_ij; v.d_Z = dst->edge_Z; v.d_w = dst->edge_w; v.d_state = dst->state;
  v.node_capacity = node_capacity; v.edge_capacity = edge_capacity;
  v.max_gap = params->max_gap; v.min_support = params->min_support; v.rounds = params->rounds;
  void* b = g->scratch;
  double* rot = at<double>(b, l.rot);
  double* trans = at<double>(b, l.trans);
  v.lmn = at<double>(b, l.lmn); v.eij = at<int>(b, l.eij); v.valid = at<int>(b, l.valid);
  v.keep[0] = at<int>(b, l.keep0); v.keep[1] = at<int>(b, l.keep1); v.sup = at<int>(b, l.sup); v.map = at<int>(b, l.map);
  v.rot_tab = rot; v.trans2_tab = trans; v.ctl = at<int>(b, l.ctl);
  g->stage_keep = at<uint8_t>(b, l.s_keep); g->stage_support = at<int32_t>(b, l.s_support);
  g->stage_map = at<int32_t>(b, l.s_map); g->stage_info = at<int32_t>(b, l.s_info);
  const size_t G = (size_t)params->max_gap + 1;
  pr::Transfer t(ctx);
  t.fill(b, 0, l.total);
  t.up(rot, rot_tab, 8 * G);
  t.up(trans, trans2_tab, 8 * G);
  return pr::commit(g, t, "pr_gate_create", out);
}

void pr_gate_destroy(pr_gate* g) { pr::destroy(g); }            // the buffers of both logs are the caller's

int pr_gate_run_dev(pr_gate* g, const double* d_poses, const int32_t* d_n, uint8_t* d_keep, int32_t* d_support, int32_t* d_map, int32_t* d_info) {
  if (!g) return fail(nullptr, PR_EINVAL, "pr_gate_run_dev: gate is NULL");
  pr_ctx* ctx = g->ctx;
  if (!d_poses || !d_n || !d_info) return fail(ctx, PR_EINVAL, "pr_gate_run_dev: a required pointer is NULL (d_poses, d_n, d_info)");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_gate(pr::ctx_stream(ctx), g->v, d_poses, d_n, d_keep, d_support, d_map, d_info);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_gate_run(pr_gate* g, const double* d_poses, const int32_t* d_n, uint8_t* keep, int32_t* support, int32_t* map, int32_t* info) {
  if (!g) return fail(nullptr, PR_EINVAL, "pr_gate_run: gate is NULL");
  pr_ctx* ctx = g->ctx;
  if (!d_poses || !d_n || !info) return fail(ctx, PR_EINVAL, "pr_gate_run: a required pointer is NULL (d_poses, d_n, info)");
  const size_t EC = (size_t)g->v.edge_capacity;
  pr::Transfer t(ctx);
  t.run([&] {
    return pr_gate_run_dev(g, d_poses, d_n, keep ? g->stage_keep : nullptr, support ? g->stage_support : nullptr, map ? g->stage_map : nullptr,
                           g->stage_info);
  });
  t.down(info, g->stage_info, 4 * sizeof(int32_t));
  t.down(keep, g->stage_keep, EC);
  t.down(support, g->stage_support, 4 * EC);
  t.down(map, g->stage_map, 4 * EC);
  return t.finish(ctx, "pr_gate_run");
}

}  // extern "C"
