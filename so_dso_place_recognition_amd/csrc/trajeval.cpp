// trajeval.cpp — host side of the trajectory evaluation (trajeval.hip): the opaque pr_trajeval, its ONE scratch allocation
// with the two tables, the argument checks, the stream-ordered run and its host form, on the shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"
#include "trajeval.hpp"

static_assert(pr::TRAJ_ALIGN_NONE == PR_TRAJ_ALIGN_NONE && pr::TRAJ_ALIGN_FIRST == PR_TRAJ_ALIGN_FIRST && pr::TRAJ_ALIGN_SE3 == PR_TRAJ_ALIGN_SE3 &&
              pr::TRAJ_ALIGN_SIM3 == PR_TRAJ_ALIGN_SIM3, "alignment modes");
static_assert(pr::TRAJ_GT_W2C == PR_TRAJ_GT_W2C && pr::TRAJ_GT_C2W == PR_TRAJ_GT_C2W && pr::TRAJ_GT_POSITIONS == PR_TRAJ_GT_POSITIONS, "gt kinds");
static_assert(pr::TRAJ_FEW == PR_TRAJ_FEW && pr::TRAJ_DEGENERATE == PR_TRAJ_DEGENERATE && pr::TRAJ_NO_SCALE == PR_TRAJ_NO_SCALE, "flag bits");
static_assert(pr::TRAJ_ATE == PR_TRAJ_ATE_STATS && pr::TRAJ_RPE == PR_TRAJ_RPE_STATS && pr::TRAJ_SEG == PR_TRAJ_SEG_STATS &&
              pr::TRAJ_CLO == PR_TRAJ_CLO_STATS, "statistics rows");
static_assert(sizeof(pr_trajeval_params) == 48, "eight int32 and two doubles, no padding");
static_assert(sizeof(pr_trajeval_out) == 9 * sizeof(void*), "nine pointers");

struct pr_trajeval : pr::Handle {    // scratch: everything TrajView names and the staging of the host form
  pr::TrajView v;
  pr::TrajOut stage;                  // the staging of the host form
};

namespace {

using pr::at;
using pr::fail;

constexpr int32_t MAX_NODES = 1 << 20, MAX_EDGES = 65536;

// where the parts of the one scratch allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena {
  size_t used, gtok, cen, prefix, S, segsum, deltas, lengths, s_ate, s_rpe, s_seg, s_clo, s_err, s_end, s_edge;
};

Layout layout_of(const pr_trajeval_params& p) {
  const size_t cap = (size_t)p.node_capacity, B = (size_t)p.batch, K = (size_t)p.n_deltas, L = (size_t)p.n_lengths, EC = (size_t)p.edge_capacity;
  const size_t slots = (size_t)pr::traj_slots(p.node_capacity, p.step);
  Layout l;
  l.used = l.take(4 * B * cap); l.gtok = l.take(4 * cap); l.cen = l.take(24 * (B + 1) * cap); l.prefix = l.take(16 * B * cap); l.S = l.take(128 * B);
  l.segsum = l.take(32 * B * L);
  l.deltas = l.take(32); l.lengths = l.take(64);
  l.s_ate = l.take(8 * pr::TRAJ_ATE * B); l.s_rpe = l.take(8 * pr::TRAJ_RPE * B * K); l.s_seg = l.take(8 * pr::TRAJ_SEG * B * (L + 1));
  l.s_clo = l.take(8 * pr::TRAJ_CLO); l.s_err = l.take(8 * B * cap); l.s_end = l.take(4 * B * slots * L); l.s_edge = l.take(16 * EC);
  return l;
}

// the value checks of create, sizes first (what the scratch formula needs), then the tables; 0 when acceptable
int check_sizes(pr_ctx* ctx, const pr_trajeval_params* p) {
  if (!p) return fail(ctx, PR_EINVAL, "pr_trajeval_create: params is NULL");
  if (p->node_capacity < 1 || p->node_capacity > MAX_NODES)
    return fail(ctx, PR_EINVAL, "pr_trajeval_create: node_capacity=%d outside 1 .. %d", p->node_capacity, MAX_NODES);
  if (p->batch < 1 || p->batch > pr::TRAJ_MAX_B) return fail(ctx, PR_EINVAL, "pr_trajeval_create: batch=%d outside 1 .. %d", p->batch, pr::TRAJ_MAX_B);
  if (p->align < PR_TRAJ_ALIGN_NONE || p->align > PR_TRAJ_ALIGN_SIM3) return fail(ctx, PR_EINVAL, "pr_trajeval_create: align=%d is no mode", p->align);
  if (p->gt_kind < PR_TRAJ_GT_W2C || p->gt_kind > PR_TRAJ_GT_POSITIONS) return fail(ctx, PR_EINVAL, "pr_trajeval_create: gt_kind=%d is no kind", p->gt_kind);
  if (p->n_deltas < 0 || p->n_deltas > pr::TRAJ_MAX_K) return fail(ctx, PR_EINVAL, "pr_trajeval_create: n_deltas=%d outside 0 .. %d", p->n_deltas, pr::TRAJ_MAX_K);
  if (p->n_lengths < 0 || p->n_lengths > pr::TRAJ_MAX_L)
    return fail(ctx, PR_EINVAL, "pr_trajeval_create: n_lengths=%d outside 0 .. %d", p->n_lengths, pr::TRAJ_MAX_L);
  if (p->step < 1) return fail(ctx, PR_EINVAL, "pr_trajeval_create: step=%d is below 1", p->step);
  if (p->edge_capacity < 0 || p->edge_capacity > MAX_EDGES)
    return fail(ctx, PR_EINVAL, "pr_trajeval_create: edge_capacity=%d outside 0 .. %d", p->edge_capacity, MAX_EDGES);
  if (p->gt_kind == PR_TRAJ_GT_POSITIONS && (p->n_deltas > 0 || p->n_lengths > 0 || p->edge_capacity > 0 || p->align == PR_TRAJ_ALIGN_FIRST))
    return fail(ctx, PR_EINVAL, "pr_trajeval_create: ground-truth positions carry no rotations: only ATE under NONE, SE3 or SIM3 is defined "
                "(n_deltas, n_lengths and edge_capacity must be 0)");
  if (std::isnan(p->rot_thr) || p->rot_thr < 0.0 || std::isnan(p->trans_thr) || p->trans_thr < 0.0)
    return fail(ctx, PR_EINVAL, "pr_trajeval_create: rot_thr or trans_thr is NaN or negative");
  return PR_OK;
}

int check_tables(pr_ctx* ctx, const pr_trajeval_params* p, const int32_t* deltas, const double* lengths) {
  if ((p->n_deltas > 0 && !deltas) || (p->n_lengths > 0 && !lengths)) return fail(ctx, PR_EINVAL, "pr_trajeval_create: a table is NULL (deltas, lengths)");
  for (int32_t k = 0; k < p->n_deltas; k++)
    if (deltas[k] < 1) return fail(ctx, PR_EINVAL, "pr_trajeval_create: deltas[%d]=%d is below 1", k, deltas[k]);
  for (int32_t l = 0; l < p->n_lengths; l++)
    if (!std::isfinite(lengths[l]) || !(lengths[l] > 0.0)) return fail(ctx, PR_EINVAL, "pr_trajeval_create: lengths[%d] is not finite and positive", l);
  return PR_OK;
}

// the required outputs of a run
int check_out(pr_ctx* ctx, const pr::TrajView& v, const pr_trajeval_out* o, bool log, const char* who) {
  if (!o) return fail(ctx, PR_EINVAL, "%s: out is NULL", who);
  if (!o->ate) return fail(ctx, PR_EINVAL, "%s: out.ate is NULL", who);
  if (v.K > 0 && !o->rpe) return fail(ctx, PR_EINVAL, "%s: out.rpe is NULL with n_deltas > 0", who);
  if (v.L > 0 && !o->seg) return fail(ctx, PR_EINVAL, "%s: out.seg is NULL with n_lengths > 0", who);
  if (log && !o->clo) return fail(ctx, PR_EINVAL, "%s: out.clo is NULL with a closure log", who);
  return PR_OK;
}

}  // namespace

extern "C" {

size_t pr_trajeval_scratch_bytes(const pr_trajeval_params* params) {
  if (!params || check_sizes(nullptr, params) != PR_OK) return 0;
  return layout_of(*params).total;
}

int pr_trajeval_create(pr_ctx* ctx, const pr_trajeval_params* params, const int32_t* deltas, const double* lengths, pr_trajeval** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_trajeval_create: out is NULL");
  *out = nullptr;
  if (int rc = check_sizes(ctx, params)) return rc;
  if (int rc = check_tables(ctx, params, deltas, lengths)) return rc;
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_trajeval_create: ctx is NULL");
  const Layout l = layout_of(*params);
  pr::Owned<pr_trajeval> g;
  if (int rc = pr::make(ctx, "pr_trajeval_create", l.total, g)) return rc;
  pr::TrajView& v = g->v;
  memset(&v, 0, sizeof v);
  memset(&g->stage, 0, sizeof g->stage);
  v.cap = params->node_capacity; v.B = params->batch; v.align = params->align; v.gt_kind = params->gt_kind;
  v.K = params->n_deltas; v.L = params->n_lengths; v.step = params->step; v.slots = pr::traj_slots(v.cap, v.step);
  v.edge_capacity = params->edge_capacity; v.rot_thr = params->rot_thr; v.trans_thr = params->trans_thr;
  void* b = g->scratch;
  v.used = at<int>(b, l.used); v.gtok = at<int>(b, l.gtok); v.cen = at<double>(b, l.cen); v.prefix = at<double>(b, l.prefix);
  v.S = at<double>(b, l.S); v.segsum = at<double>(b, l.segsum); v.deltas = at<int>(b, l.deltas); v.lengths = at<double>(b, l.lengths);
  pr::TrajOut& s = g->stage;
  s.ate = at<double>(b, l.s_ate); s.rpe = at<double>(b, l.s_rpe); s.seg = at<double>(b, l.s_seg); s.clo = at<double>(b, l.s_clo);
  s.err = at<double>(b, l.s_err); s.seg_end = at<int>(b, l.s_end); s.edge_err = at<double>(b, l.s_edge);
  pr::Transfer t(ctx);
  t.fill(b, 0, l.total);
  t.up(at<int>(b, l.deltas), deltas, 4 * (size_t)v.K);           // (a table of no entries may be NULL)
  t.up(at<double>(b, l.lengths), lengths, 8 * (size_t)v.L);
  return pr::commit(g, t, "pr_trajeval_create", out);
}

void pr_trajeval_destroy(pr_trajeval* g) { pr::destroy(g); }

int pr_trajeval_run_dev(pr_trajeval* g, const double* d_est, const int32_t* d_n, const void* d_gt, const uint8_t* d_valid,
                        const pr_posegraph_buffers* log, const pr_trajeval_out* out) {
  if (!g) return fail(nullptr, PR_EINVAL, "pr_trajeval_run_dev: handle is NULL");
  pr_ctx* ctx = g->ctx;
  if (!d_est || !d_n || !d_gt) return fail(ctx, PR_EINVAL, "pr_trajeval_run_dev: a required pointer is NULL (d_est, d_n, d_gt)");
  if (log && g->v.edge_capacity == 0) return fail(ctx, PR_EINVAL, "pr_trajeval_run_dev: a closure log was given but edge_capacity is 0");
  if (log && (!log->edge_ij || !log->edge_Z || !log->state))
    return fail(ctx, PR_EINVAL, "pr_trajeval_run_dev: a buffer of the closure log is NULL (edge_ij, edge_Z, state)");
  if (int rc = check_out(ctx, g->v, out, log != nullptr, "pr_trajeval_run_dev")) return rc;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::TrajIn in;
  in.est = d_est; in.n = d_n; in.gt = static_cast<const double*>(d_gt); in.valid = d_valid;
  in.e_ij = log ? log->edge_ij : nullptr; in.e_Z = log ? log->edge_Z : nullptr; in.e_state = log ? log->state : nullptr;
  pr::TrajOut o;
  o.ate = out->ate; o.rpe = out->rpe; o.seg = out->seg; o.clo = out->clo; o.err = out->err; o.seg_end = out->seg_end; o.edge_err = out->edge_err;
  o.centres = out->centres; o.prefix = out->prefix;
  pr::launch_trajeval(pr::ctx_stream(ctx), g->v, in, o);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_trajeval_run(pr_trajeval* g, const double* d_est, const int32_t* d_n, const void* d_gt, const uint8_t* d_valid,
                    const pr_posegraph_buffers* log, const pr_trajeval_out* out) {
  if (!g) return fail(nullptr, PR_EINVAL, "pr_trajeval_run: handle is NULL");
  pr_ctx* ctx = g->ctx;
  const pr::TrajView& v = g->v;
  if (int rc = check_out(ctx, v, out, log != nullptr, "pr_trajeval_run")) return rc;
  pr_trajeval_out d;
  memset(&d, 0, sizeof d);
  d.ate = g->stage.ate; d.rpe = v.K > 0 ? g->stage.rpe : nullptr; d.seg = v.L > 0 ? g->stage.seg : nullptr; d.clo = log ? g->stage.clo : nullptr;
  d.err = out->err ? g->stage.err : nullptr; d.seg_end = out->seg_end && v.L > 0 ? g->stage.seg_end : nullptr;
  d.edge_err = out->edge_err && log ? g->stage.edge_err : nullptr;      // the centres and the prefixes are read from the scratch itself
  const size_t cap = (size_t)v.cap, B = (size_t)v.B, K = (size_t)v.K, L = (size_t)v.L;
  pr::Transfer t(ctx);
  t.run([&] { return pr_trajeval_run_dev(g, d_est, d_n, d_gt, d_valid, log, &d); });
  t.down(out->ate, d.ate, 8 * pr::TRAJ_ATE * B);
  t.down(out->rpe, d.rpe, 8 * pr::TRAJ_RPE * B * K);
  t.down(out->seg, d.seg, 8 * pr::TRAJ_SEG * B * (L + 1));
  t.down(out->clo, d.clo, 8 * pr::TRAJ_CLO);
  t.down(out->err, d.err, 8 * B * cap);
  t.down(out->seg_end, d.seg_end, 4 * B * (size_t)v.slots * L);
  t.down(out->edge_err, d.edge_err, 16 * (size_t)v.edge_capacity);
  t.down(out->centres, v.cen, 24 * (B + 1) * cap);
  t.down(out->prefix, v.prefix, 16 * B * cap);
  return t.finish(ctx, "pr_trajeval_run");
}

}  // extern "C"
