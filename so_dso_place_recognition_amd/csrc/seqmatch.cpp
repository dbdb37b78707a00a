// seqmatch.cpp — host side of the sequence matcher (seqmatch.hip): the tile constants, the argument checks and the
// stream-ordered launch of the batch form.  The host-buffer form (pr_match_topk_seq_f64) lives with the shared top-k pipeline in pr_api.cpp.
// The online form (pr_seqmatch, its ONE scratch allocation, push and read) stands on the shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"
#include "seqmatch.hpp"

static_assert(pr::SEQ_REACH == PR_SEQ_MAX_STEP && pr::SEQ_MAX_L == PR_SEQ_MAX_L && pr::SEQ_MAX_V == PR_SEQ_MAX_V && pr::SEQ_MAX_K == PR_SEQ_MAX_K,
              "the header's limits");
static_assert(pr::SEQ_ONLINE_MAX_K == PR_SEQMATCH_MAX_K, "the header's limit of the online form");

using pr::at;
using pr::fail;

extern "C" {

void pr_seq_tile(int32_t* rows, int32_t* cols) {
  if (rows) *rows = pr::SEQ_R;
  if (cols) *cols = pr::SEQ_W;
}

int pr_seq_select_dev(pr_ctx* ctx, const float* d_p, const float* d_i, int32_t m, int32_t n, const double* mom, const int32_t* d_steps,
                      int32_t V, int32_t L, int32_t q_row0, int32_t db_row0, int32_t mask_width, double p_weight, int32_t k, int32_t* idx,
                      double* score, int32_t* vel, double* d_S) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!d_p || !d_steps || !idx || !score || !vel)
    return fail(ctx, PR_EINVAL, "pr_seq_select_dev: a required pointer is NULL (d_p, d_steps, idx, score, vel)");
  if (d_i && !mom) return fail(ctx, PR_EINVAL, "pr_seq_select_dev: mom is NULL with d_i given");
  if (m < 0 || n < 1) return fail(ctx, PR_EINVAL, "pr_seq_select_dev: m=%d, n=%d (m >= 0, n >= 1)", m, n);
  if (V < 1 || V > pr::SEQ_MAX_V) return fail(ctx, PR_EINVAL, "pr_seq_select_dev: V=%d outside 1 .. %d", V, pr::SEQ_MAX_V);
  if (L < 1 || L > pr::SEQ_MAX_L) return fail(ctx, PR_EINVAL, "pr_seq_select_dev: L=%d outside 1 .. %d", L, pr::SEQ_MAX_L);
  if (k < 1 || k > pr::SEQ_MAX_K) return fail(ctx, PR_EINVAL, "pr_seq_select_dev: k=%d outside 1 .. %d", k, pr::SEQ_MAX_K);
  if (mask_width < 0) return fail(ctx, PR_EINVAL, "pr_seq_select_dev: mask_width=%d is negative", mask_width);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_seq_select_dev: ctx is NULL");
  if (m == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_seq_select(pr::ctx_stream(ctx), d_p, d_i, m, n, mom, d_steps, V, L, q_row0, db_row0, mask_width, p_weight, k, idx, score, vel, d_S,
                        pr::ctx_seq_scratch(ctx));
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------ the online form
struct pr_seqmatch : pr::Handle {    // scratch: everything SeqView names, then the staging of the host form
  pr::SeqView v;
  size_t state_bytes = 0;             // ring | ids | count: what reset clears
  double* stage_rows = nullptr;       // [channels][capacity]
  int32_t* stage_count = nullptr;     // [4]
  double* stage_score = nullptr;      // [max_k]
  int32_t* stage_idx = nullptr;       // [max_k]
  int32_t* stage_vel = nullptr;       // [max_k]
  int32_t* stage_info = nullptr;      // [4]
};

namespace {

constexpr int32_t SEQ_MAX_CAPACITY = 1 << 24;

struct Layout : pr::Arena {
  size_t ring, ids, count, stats, ctl, steps, lscore, lj, lv, s_rows, s_count, s_score, s_idx, s_vel, s_info;
};

// where the parts of the one allocation lie (each on a 16-byte boundary); the formula of the header
Layout layout_of(int32_t capacity, int32_t channels, int32_t V, int32_t L, int32_t max_k) {
  const size_t cap = (size_t)capacity, B = (cap + pr::SEQ_PUSH_COLS - 1) / pr::SEQ_PUSH_COLS, K = (size_t)max_k;
  Layout l;
  l.ring = l.take(8 * cap * L); l.ids = l.take(4 * (size_t)L); l.count = l.take(16);
  l.stats = l.take(64); l.ctl = l.take(16); l.steps = l.take(4 * (size_t)V * L);
  l.lscore = l.take(8 * B * K); l.lj = l.take(4 * B * K); l.lv = l.take(4 * B * K);
  l.s_rows = l.take(8 * cap * channels); l.s_count = l.take(16); l.s_score = l.take(8 * K); l.s_idx = l.take(4 * K); l.s_vel = l.take(4 * K);
  l.s_info = l.take(16);
  return l;
}

bool sizes_ok(int32_t capacity, int32_t channels, int32_t V, int32_t L, int32_t max_k) {
  return capacity >= 1 && capacity <= SEQ_MAX_CAPACITY && (channels == 1 || channels == 2 || channels == 4) && V >= 1 && V <= pr::SEQ_MAX_V &&
         L >= 1 && L <= pr::SEQ_MAX_L && max_k >= 1 && max_k <= pr::SEQ_ONLINE_MAX_K;
}

}  // namespace

extern "C" {

size_t pr_seqmatch_scratch_bytes(int32_t capacity, int32_t channels, int32_t V, int32_t L, int32_t max_k) {
  if (!sizes_ok(capacity, channels, V, L, max_k)) return 0;
  return layout_of(capacity, channels, V, L, max_k).total;
}

int pr_seqmatch_create(pr_ctx* ctx, int32_t capacity, int32_t channels, const int32_t* steps, int32_t V, int32_t L, int32_t max_k,
                       pr_seqmatch** out) {
  if (!out) return fail(ctx, PR_EINVAL, "pr_seqmatch_create: out is NULL");
  *out = nullptr;
  if (!steps) return fail(ctx, PR_EINVAL, "pr_seqmatch_create: steps is NULL");
  if (capacity < 1 || capacity > SEQ_MAX_CAPACITY)
    return fail(ctx, PR_EINVAL, "pr_seqmatch_create: capacity=%d outside 1 .. %d", capacity, SEQ_MAX_CAPACITY);
  if (channels != 1 && channels != 2 && channels != 4) return fail(ctx, PR_EINVAL, "pr_seqmatch_create: channels=%d is not 1, 2 or 4", channels);
  if (int bad = pr::seq_steps_bad(steps, V, L))
    return fail(ctx, PR_EINVAL, "pr_seqmatch_create: bad step table (V=%d, L=%d): %s", V, L,
                bad == 1 ? "V outside 1 .. 16 or L outside 1 .. 32" : bad == 2 ? "steps[v][0] != 0" : "|steps[v][l]| > 64");
  if (max_k < 1 || max_k > pr::SEQ_ONLINE_MAX_K)
    return fail(ctx, PR_EINVAL, "pr_seqmatch_create: max_k=%d outside 1 .. %d", max_k, pr::SEQ_ONLINE_MAX_K);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_seqmatch_create: ctx is NULL");
  const Layout l = layout_of(capacity, channels, V, L, max_k);
  pr::Owned<pr_seqmatch> s;
  if (int rc = pr::make(ctx, "pr_seqmatch_create", l.total, s)) return rc;
  void* b = s->scratch;
  pr::SeqView& v = s->v;
  v.capacity = capacity; v.channels = channels; v.V = V; v.L = L; v.max_k = max_k;
  v.blocks = (capacity + pr::SEQ_PUSH_COLS - 1) / pr::SEQ_PUSH_COLS;
  v.ring = at<double>(b, l.ring); v.ids = at<int>(b, l.ids); v.count = at<int>(b, l.count); v.stats = at<double>(b, l.stats);
  v.ctl = at<int>(b, l.ctl); v.steps = at<int>(b, l.steps); v.lscore = at<double>(b, l.lscore); v.lj = at<int>(b, l.lj); v.lv = at<int>(b, l.lv);
  s->state_bytes = l.stats;                                       // ring | ids | count lie first
  s->stage_rows = at<double>(b, l.s_rows); s->stage_count = at<int32_t>(b, l.s_count); s->stage_score = at<double>(b, l.s_score);
  s->stage_idx = at<int32_t>(b, l.s_idx); s->stage_vel = at<int32_t>(b, l.s_vel); s->stage_info = at<int32_t>(b, l.s_info);
  pr::Transfer t(ctx);
  t.fill(b, 0, l.total);
  t.up(at<int>(b, l.steps), steps, 4 * (size_t)V * L);
  return pr::commit(s, t, "pr_seqmatch_create", out);
}

void pr_seqmatch_destroy(pr_seqmatch* s) { pr::destroy(s); }

int pr_seqmatch_reset(pr_seqmatch* s) {
  if (!s) return fail(nullptr, PR_EINVAL, "pr_seqmatch_reset: handle is NULL");
  PR_CHECK_HIP(s->ctx, hipSetDevice(pr::ctx_device(s->ctx)));
  PR_CHECK_HIP(s->ctx, hipMemsetAsync(s->scratch, 0, s->state_bytes, pr::ctx_stream(s->ctx)));   // stream-ordered: ring, row ids, counter
  return PR_OK;
}

static int push_checks(pr_seqmatch* s, const char* who, const void* rows, const void* count, const double* weights, int32_t normalize,
                       int32_t mask_width, int32_t k, const void* idx, const void* score, const void* vel, const void* info) {
  if (!s) return fail(nullptr, PR_EINVAL, "%s: handle is NULL", who);
  pr_ctx* ctx = s->ctx;
  if (k < 1 || k > s->v.max_k) return fail(ctx, PR_EINVAL, "%s: k=%d outside 1 .. max_k=%d", who, k, s->v.max_k);
  if (!rows || !count || !weights || !idx || !score || !vel || !info)
    return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (rows, count, weights, idx, score, vel, info)", who);
  if (mask_width < 0) return fail(ctx, PR_EINVAL, "%s: mask_width=%d is negative", who, mask_width);
  if (normalize != 0 && normalize != 1) return fail(ctx, PR_EINVAL, "%s: normalize=%d is not 0 or 1", who, normalize);
  if (!normalize && s->v.channels != 1) return fail(ctx, PR_EINVAL, "%s: normalize=0 needs channels == 1 (have %d)", who, s->v.channels);
  for (int c = 0; c < s->v.channels; c++)
    if (!std::isfinite(weights[c])) return fail(ctx, PR_EINVAL, "%s: weights[%d] is not finite", who, c);
  return PR_OK;
}

int pr_seqmatch_push_dev(pr_seqmatch* s, const double* d_rows, const int32_t* d_count, const int32_t* d_emitted, const double* weights,
                         int32_t normalize, int32_t mask_width, int32_t k, int32_t* d_idx, double* d_score, int32_t* d_vel, int32_t* d_info) {
  if (int rc = push_checks(s, "pr_seqmatch_push_dev", d_rows, d_count, weights, normalize, mask_width, k, d_idx, d_score, d_vel, d_info)) return rc;
  pr_ctx* ctx = s->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::SeqWeights w = {{0.0, 0.0, 0.0, 0.0}};
  for (int c = 0; c < s->v.channels; c++) w.w[c] = weights[c];
  pr::launch_seq_push(pr::ctx_stream(ctx), s->v, d_rows, d_count, d_emitted, w, normalize, mask_width, k, d_idx, d_score, d_vel, d_info);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_seqmatch_push(pr_seqmatch* s, const double* rows, int32_t count, const double* weights, int32_t normalize, int32_t mask_width, int32_t k,
                     int32_t* idx, double* score, int32_t* vel, int32_t* info) {
  if (int rc = push_checks(s, "pr_seqmatch_push", rows, &count, weights, normalize, mask_width, k, idx, score, vel, info)) return rc;
  pr_ctx* ctx = s->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::Transfer t(ctx);
  t.up(s->stage_rows, rows, 8 * (size_t)s->v.capacity * s->v.channels);
  t.up(s->stage_count, &count, 4);
  t.run([&] {
    return pr_seqmatch_push_dev(s, s->stage_rows, s->stage_count, nullptr, weights, normalize, mask_width, k, s->stage_idx, s->stage_score,
                                s->stage_vel, s->stage_info);
  });
  t.down(idx, s->stage_idx, 4 * (size_t)k);
  t.down(score, s->stage_score, 8 * (size_t)k);
  t.down(vel, s->stage_vel, 4 * (size_t)k);
  t.down(info, s->stage_info, 16);
  return t.finish(ctx, "pr_seqmatch_push");
}

int pr_seqmatch_read(pr_seqmatch* s, double* ring, int32_t* ids, int32_t* pushes) {
  if (!s) return fail(nullptr, PR_EINVAL, "pr_seqmatch_read: handle is NULL");
  pr_ctx* ctx = s->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::Transfer t(ctx);
  t.down(ring, s->v.ring, 8 * (size_t)s->v.capacity * s->v.L);
  t.down(ids, s->v.ids, 4 * (size_t)s->v.L);
  t.down(pushes, s->v.count, 4);
  return t.finish(ctx, "pr_seqmatch_read");
}

}  // extern "C"
