// online.cpp — host side of the online engine (online.hip): ONE core - the view over the caller's buffers, its scratch, match, append and
// the host form of an append - behind two C families, pr_online (SC, M2DP) and pr_onlineset (FUSED, DELIGHT), whose entry points do their own argument checks.
// Layout, create tail, destroy, the state word and the copy chain come from the shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"
#include "online.hpp"

static_assert(pr::ONLINE_OVERFLOW == PR_ONLINE_OVERFLOW, "flag bit");
static_assert(PR_TYPE_SC == pr::ONLINE_SC && PR_TYPE_M2DP == pr::ONLINE_M2DP, "pr_online_create passes its type on as the kind");
static_assert(PR_ONLINESET_FUSED == 0 && PR_ONLINESET_DELIGHT == 1 && pr::ONLINE_DELIGHT == pr::ONLINE_FUSED + 1, "pr_onlineset_create adds ONLINE_FUSED");

struct OnlineCore : pr::Handle {     // scratch: rows, partial, stats and the staging of the host form
  pr::OnlineView v;
  double* stage_sig = nullptr;        // [len[0] + len[1]]: the parts, one behind the other
  int32_t* stage_info = nullptr;      // [4]
};
struct pr_online : OnlineCore {};
struct pr_onlineset : OnlineCore {};

namespace {

using pr::at;
using pr::fail;

// Below, fn is the entry point's name and noun what it calls its handle ("database" / "set").  create: what is left once the entry point has
// checked its own arguments - the checks both families share, the handle, the view over (p0, p1, state) and the scratch, from (kind, capacity) alone.
template <class T>
int create(pr_ctx* ctx, const char* fn, int kind, double* p0, double* p1, int32_t* state, int32_t capacity, int32_t max_k, T** out) {
  if (capacity < 1 || capacity > PR_MAX_SIGS) return fail(ctx, PR_EINVAL, "%s: capacity=%d outside 1 .. PR_MAX_SIGS=%d", fn, capacity, PR_MAX_SIGS);
  if (max_k < 1 || max_k > pr::ONLINE_MAX_K) return fail(ctx, PR_EINVAL, "%s: max_k=%d outside 1 .. %d", fn, max_k, pr::ONLINE_MAX_K);
  if (!ctx) return fail(nullptr, PR_EINVAL, "%s: ctx is NULL", fn);
  const int len0 = kind == pr::ONLINE_M2DP ? pr::ONLINE_M2DP_LEN : (kind == pr::ONLINE_DELIGHT ? pr::ONLINE_DELIGHT_LEN : pr::ONLINE_SC_LEN);
  const int len1 = kind == pr::ONLINE_FUSED ? pr::ONLINE_M2DP_LEN : 0, NB = pr::online_blocks(kind, capacity);
  const size_t C = (size_t)pr::online_channels(kind);
  pr::Arena a;
  const size_t o_rows = a.take(C * capacity * 8), o_part = a.take((size_t)NB * 2 * C * 8), o_stats = a.take(2 * C * 8),
               o_sig = a.take((size_t)(len0 + len1) * 8), o_info = a.take(16);
  pr::Owned<T> o;
  if (int rc = pr::make(ctx, fn, a.total, o)) return rc;
  pr::OnlineView& v = o->v;
  memset(&v, 0, sizeof v);
  v.part[0] = p0; v.part[1] = p1; v.state = state;
  v.len[0] = len0; v.len[1] = len1;
  v.kind = kind; v.capacity = capacity; v.max_k = max_k; v.NB = NB;
  void* b = o->scratch;
  v.rows = at<double>(b, o_rows); v.partial = at<double>(b, o_part); v.stats = at<double>(b, o_stats);
  o->stage_sig = at<double>(b, o_sig); o->stage_info = at<int32_t>(b, o_info);
  pr::Transfer t(ctx);
  t.fill(v.state, 0, 4 * sizeof(int32_t));
  t.fill(b, 0, a.total);
  return pr::commit(o, t, fn, out);
}

int no_handle(const char* fn, const char* noun) { return fail(nullptr, PR_EINVAL, "%s: %s is NULL", fn, noun); }

int reset(OnlineCore* o, const char* fn, const char* noun) {
  if (!o) return no_handle(fn, noun);
  return pr::clear_state(o->ctx, o->v.state);
}

int read_count(OnlineCore* o, const char* fn, const char* noun, int32_t* count, int32_t* flags) {
  if (!o) return no_handle(fn, noun);
  if (!count || !flags) return fail(o->ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  int32_t s[4];
  if (int rc = pr::read_state(o->ctx, fn, o->v.state, s)) return rc;
  *count = s[0]; *flags = s[1];
  return PR_OK;
}

// The checks of a match that come before its pointers.  Those that need no handle come first: with o == NULL their text goes to pr_last_error(NULL).
int check_match(const OnlineCore* o, const char* fn, const char* noun, int32_t mask_width, double p_weight, int32_t k) {
  pr_ctx* ctx = o ? o->ctx : nullptr;
  if (mask_width < 0) return fail(ctx, PR_EINVAL, "%s: mask_width=%d is negative", fn, mask_width);
  if (!std::isfinite(p_weight)) return fail(ctx, PR_EINVAL, "%s: p_weight is not finite", fn);
  if (k < 1 || k > pr::ONLINE_MAX_K) return fail(ctx, PR_EINVAL, "%s: k=%d outside 1 .. %d", fn, k, pr::ONLINE_MAX_K);
  if (!o) return no_handle(fn, noun);
  if (k > o->v.max_k) return fail(ctx, PR_EINVAL, "%s: k=%d outside 1 .. max_k=%d", fn, k, o->v.max_k);
  return 0;
}

int match(OnlineCore* o, const pr::OnlineParts& q, const int32_t* d_emitted, int32_t mask_width, double p_weight, int32_t k, int32_t* d_idx,
          double* d_score, double* d_rows) {
  PR_CHECK_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  pr::launch_online_match(pr::ctx_stream(o->ctx), o->v, q, d_emitted, mask_width, p_weight, k, d_idx, d_score, d_rows ? d_rows : o->v.rows);
  PR_CHECK_HIP(o->ctx, hipGetLastError());
  return PR_OK;
}

int append_dev(OnlineCore* o, const pr::OnlineParts& src, const int32_t* d_emitted, int32_t* d_info) {
  PR_CHECK_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  pr::launch_online_append(pr::ctx_stream(o->ctx), o->v, src, d_emitted, d_info);
  PR_CHECK_HIP(o->ctx, hipGetLastError());
  return PR_OK;
}

// The host form: the parts through stage_sig, the device path, info back; synchronises.
int append_host(OnlineCore* o, const char* fn, const pr::OnlineParts& src, int32_t* info) {
  PR_CHECK_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  double* const stage[2] = {o->stage_sig, o->v.len[1] ? o->stage_sig + o->v.len[0] : nullptr};
  pr::Transfer t(o->ctx);
  for (int p = 0; p < 2; p++) t.up(stage[p], src.p[p], (size_t)o->v.len[p] * sizeof(double));
  t.run([&] { return append_dev(o, {{stage[0], stage[1]}}, nullptr, o->stage_info); });
  t.down(info, o->stage_info, 4 * sizeof(int32_t));
  return t.finish(o->ctx, fn);
}

// The parts a pr_onlineset call of this kind takes: FUSED needs sc and m2dp and no delight, DELIGHT the reverse.  0, or PR_EINVAL with the text set.
int check_parts(pr_ctx* ctx, const char* fn, int kind, const void* sc, const void* m2dp, const void* delight, const char* prefix) {
  if (kind == pr::ONLINE_FUSED) {
    if (delight) return fail(ctx, PR_EINVAL, "%s: %sdelight must be NULL for a PR_ONLINESET_FUSED set", fn, prefix);
    if (!sc || !m2dp) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (%ssc, %sm2dp)", fn, prefix, prefix);
  } else {
    if (sc || m2dp) return fail(ctx, PR_EINVAL, "%s: %ssc and %sm2dp must be NULL for a PR_ONLINESET_DELIGHT set", fn, prefix, prefix);
    if (!delight) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (%sdelight)", fn, prefix);
  }
  return 0;
}
// (after check_parts) the set's parts in the view's order
pr::OnlineParts set_parts(const double* sc, const double* m2dp, const double* delight) { return {{sc ? sc : delight, m2dp}}; }

}  // namespace

extern "C" {

// In both creates the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL).
int pr_online_create(pr_ctx* ctx, int type, const pr_online_buffers* buffers, int32_t capacity, int32_t max_k, pr_online** out) {
  if (!out) return fail(ctx, PR_EINVAL, "pr_online_create: out is NULL");
  *out = nullptr;
  if (!buffers) return fail(ctx, PR_EINVAL, "pr_online_create: buffers is NULL");
  if (!buffers->sig || !buffers->state) return fail(ctx, PR_EINVAL, "pr_online_create: a buffer is NULL (sig, state)");
  if (type != PR_TYPE_SC && type != PR_TYPE_M2DP) return fail(ctx, PR_EINVAL, "pr_online_create: type=%d is neither PR_TYPE_SC nor PR_TYPE_M2DP", type);
  return create(ctx, "pr_online_create", type, buffers->sig, nullptr, buffers->state, capacity, max_k, out);
}

int pr_onlineset_create(pr_ctx* ctx, int kind, const pr_onlineset_buffers* buffers, int32_t capacity, int32_t max_k, pr_onlineset** out) {
  if (!out) return fail(ctx, PR_EINVAL, "pr_onlineset_create: out is NULL");
  *out = nullptr;
  if (!buffers) return fail(ctx, PR_EINVAL, "pr_onlineset_create: buffers is NULL");
  if (kind != PR_ONLINESET_FUSED && kind != PR_ONLINESET_DELIGHT)
    return fail(ctx, PR_EINVAL, "pr_onlineset_create: kind=%d is neither PR_ONLINESET_FUSED nor PR_ONLINESET_DELIGHT", kind);
  if (!buffers->state) return fail(ctx, PR_EINVAL, "pr_onlineset_create: a buffer is NULL (state)");
  if (kind == PR_ONLINESET_FUSED) {
    if (buffers->delight) return fail(ctx, PR_EINVAL, "pr_onlineset_create: buffer delight must be NULL for a PR_ONLINESET_FUSED set");
    if (!buffers->sc || !buffers->m2dp) return fail(ctx, PR_EINVAL, "pr_onlineset_create: a buffer is NULL (sc, m2dp)");
  } else {
    if (buffers->sc || buffers->m2dp) return fail(ctx, PR_EINVAL, "pr_onlineset_create: buffers sc and m2dp must be NULL for a PR_ONLINESET_DELIGHT set");
    if (!buffers->delight) return fail(ctx, PR_EINVAL, "pr_onlineset_create: a buffer is NULL (delight)");
  }
  return create(ctx, "pr_onlineset_create", pr::ONLINE_FUSED + kind, kind == PR_ONLINESET_FUSED ? buffers->sc : buffers->delight, buffers->m2dp,
                buffers->state, capacity, max_k, out);
}

void pr_online_destroy(pr_online* o) { pr::destroy(o); }         // the buffers are the caller's
void pr_onlineset_destroy(pr_onlineset* o) { pr::destroy(o); }

int pr_online_reset(pr_online* o) { return reset(o, "pr_online_reset", "database"); }
int pr_onlineset_reset(pr_onlineset* o) { return reset(o, "pr_onlineset_reset", "set"); }

int pr_online_count(pr_online* o, int32_t* count, int32_t* flags) { return read_count(o, "pr_online_count", "database", count, flags); }
int pr_onlineset_count(pr_onlineset* o, int32_t* count, int32_t* flags) { return read_count(o, "pr_onlineset_count", "set", count, flags); }

int pr_online_match_dev(pr_online* o, const double* d_sig, const int32_t* d_emitted, int32_t mask_width, double p_weight, int32_t k,
                        int32_t* d_idx, double* d_score, double* d_rows) {
  if (int rc = check_match(o, "pr_online_match_dev", "database", mask_width, p_weight, k)) return rc;
  if (!d_sig || !d_idx || !d_score) return fail(o->ctx, PR_EINVAL, "pr_online_match_dev: a required pointer is NULL (d_sig, d_idx, d_score)");
  return match(o, {{d_sig, nullptr}}, d_emitted, mask_width, p_weight, k, d_idx, d_score, d_rows);
}

int pr_onlineset_match_dev(pr_onlineset* o, const double* d_sc, const double* d_m2dp, const double* d_delight, const int32_t* d_emitted,
                           int32_t mask_width, double p_weight, int32_t k, int32_t* d_idx, double* d_score, double* d_rows) {
  if (int rc = check_match(o, "pr_onlineset_match_dev", "set", mask_width, p_weight, k)) return rc;
  if (int rc = check_parts(o->ctx, "pr_onlineset_match_dev", o->v.kind, d_sc, d_m2dp, d_delight, "d_")) return rc;
  if (!d_idx || !d_score) return fail(o->ctx, PR_EINVAL, "pr_onlineset_match_dev: a required pointer is NULL (d_idx, d_score)");
  return match(o, set_parts(d_sc, d_m2dp, d_delight), d_emitted, mask_width, p_weight, k, d_idx, d_score, d_rows);
}

int pr_online_append_dev(pr_online* o, const double* d_sig, const int32_t* d_emitted, int32_t* d_info) {
  if (!o) return no_handle("pr_online_append_dev", "database");
  if (!d_sig || !d_info) return fail(o->ctx, PR_EINVAL, "pr_online_append_dev: a required pointer is NULL (d_sig, d_info)");
  return append_dev(o, {{d_sig, nullptr}}, d_emitted, d_info);
}

int pr_onlineset_append_dev(pr_onlineset* o, const double* d_sc, const double* d_m2dp, const double* d_delight, const int32_t* d_emitted,
                            int32_t* d_info) {
  if (!o) return no_handle("pr_onlineset_append_dev", "set");
  if (int rc = check_parts(o->ctx, "pr_onlineset_append_dev", o->v.kind, d_sc, d_m2dp, d_delight, "d_")) return rc;
  if (!d_info) return fail(o->ctx, PR_EINVAL, "pr_onlineset_append_dev: a required pointer is NULL (d_info)");
  return append_dev(o, set_parts(d_sc, d_m2dp, d_delight), d_emitted, d_info);
}

int pr_online_append(pr_online* o, const double* sig, int32_t* info) {
  if (!o) return no_handle("pr_online_append", "database");
  if (!sig || !info) return fail(o->ctx, PR_EINVAL, "pr_online_append: a required pointer is NULL (sig, info)");
  return append_host(o, "pr_online_append", {{sig, nullptr}}, info);
}

int pr_onlineset_append(pr_onlineset* o, const double* sc, const double* m2dp, const double* delight, int32_t* info) {
  if (!o) return no_handle("pr_onlineset_append", "set");
  if (int rc = check_parts(o->ctx, "pr_onlineset_append", o->v.kind, sc, m2dp, delight, "")) return rc;
  if (!info) return fail(o->ctx, PR_EINVAL, "pr_onlineset_append: a required pointer is NULL (info)");
  return append_host(o, "pr_onlineset_append", set_parts(sc, m2dp, delight), info);
}

}  // extern "C"
