// onlineset.cpp — host side of the online signature sets (onlineset.hip): the opaque pr_onlineset over the caller's
// buffers with its scratch, the argument checks, the stream-ordered entry points and the host form of an append.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/place_recognition.h"
#include "kernels.hpp"
#include "onlineset.hpp"

static_assert(pr::ONLINESET_OVERFLOW == PR_ONLINE_OVERFLOW, "flag bit");
static_assert(pr::ONLINESET_FUSED == PR_ONLINESET_FUSED && pr::ONLINESET_DELIGHT == PR_ONLINESET_DELIGHT, "onlineset.hip tells the kinds apart by these values");

struct pr_onlineset {
  pr_ctx* ctx = nullptr;
  pr::OnlineSetView v;
  void* scratch = nullptr;            // one allocation: rows, partial, stats and the staging of the host form
  double* stage_sig = nullptr;        // FUSED: [2400 + 1536] (SC, then M2DP); DELIGHT: [4096]
  int32_t* stage_info = nullptr;      // [4]
};

namespace {

int fail(pr_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int fail(pr_ctx* ctx, int code, const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  pr::ctx_set_error(ctx, b);
  return code;
}

#define ONSET_HIP(ctx, call)                                                                                      \
  do {                                                                                                            \
    hipError_t _e = (call);                                                                                       \
    if (_e != hipSuccess)                                                                                         \
      return fail(ctx, _e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
  } while (0)

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// The parts a call of this kind takes: FUSED needs sc and m2dp and no delight, DELIGHT the reverse.  0, or PR_EINVAL with the text set.
int check_parts(pr_ctx* ctx, const char* fn, int kind, const void* sc, const void* m2dp, const void* delight, const char* prefix) {
  if (kind == PR_ONLINESET_FUSED) {
    if (delight) return fail(ctx, PR_EINVAL, "%s: %sdelight must be NULL for a PR_ONLINESET_FUSED set", fn, prefix);
    if (!sc || !m2dp) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (%ssc, %sm2dp)", fn, prefix, prefix);
  } else {
    if (sc || m2dp) return fail(ctx, PR_EINVAL, "%s: %ssc and %sm2dp must be NULL for a PR_ONLINESET_DELIGHT set", fn, prefix, prefix);
    if (!delight) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (%sdelight)", fn, prefix);
  }
  return 0;
}

}  // namespace

extern "C" {

int pr_onlineset_create(pr_ctx* ctx, int kind, const pr_onlineset_buffers* buffers, int32_t capacity, int32_t max_k, pr_onlineset** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
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
  if (capacity < 1 || capacity > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_onlineset_create: capacity=%d outside 1 .. PR_MAX_SIGS=%d", capacity, PR_MAX_SIGS);
  if (max_k < 1 || max_k > pr::ONLINESET_MAX_K) return fail(ctx, PR_EINVAL, "pr_onlineset_create: max_k=%d outside 1 .. %d", max_k, pr::ONLINESET_MAX_K);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_onlineset_create: ctx is NULL");
  ONSET_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_onlineset* o = new (std::nothrow) pr_onlineset;
  if (!o) return fail(ctx, PR_ENOMEM, "out of host memory");
  o->ctx = ctx;
  pr::OnlineSetView& v = o->v;
  memset(&v, 0, sizeof v);
  v.sc = buffers->sc; v.m2dp = buffers->m2dp; v.delight = buffers->delight; v.state = buffers->state;
  v.kind = kind; v.capacity = capacity; v.max_k = max_k; v.NB = pr::onlineset_blocks(kind, capacity);
  const size_t sig_doubles = kind == PR_ONLINESET_FUSED ? (size_t)pr::ONLINESET_SC + pr::ONLINESET_M2DP : (size_t)pr::ONLINESET_DELIGHT_LEN;
  const size_t o_rows = 0, o_part = o_rows + up16((size_t)pr::onlineset_channels(kind) * capacity * 8), o_stats = o_part + up16((size_t)v.NB * 8 * 8),
               o_sig = o_stats + 64, o_info = o_sig + up16(sig_doubles * 8), total = o_info + 16;
  hipError_t e = hipMalloc(&o->scratch, total);
  if (e != hipSuccess) {
    delete o;
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_onlineset_create: scratch: %s", hipGetErrorString(e));
  }
  char* b = static_cast<char*>(o->scratch);
  v.rows = reinterpret_cast<double*>(b + o_rows); v.partial = reinterpret_cast<double*>(b + o_part); v.stats = reinterpret_cast<double*>(b + o_stats);
  o->stage_sig = reinterpret_cast<double*>(b + o_sig); o->stage_info = reinterpret_cast<int32_t*>(b + o_info);
  hipStream_t st = pr::ctx_stream(ctx);
  e = hipMemsetAsync(v.state, 0, 4 * sizeof(int32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(o->scratch, 0, total, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(o->scratch);
    delete o;
    return fail(ctx, PR_EHIP, "pr_onlineset_create: clearing the state failed: %s", hipGetErrorString(e));
  }
  *out = o;
  return PR_OK;
}

void pr_onlineset_destroy(pr_onlineset* o) {
  if (!o) return;
  (void)hipSetDevice(pr::ctx_device(o->ctx));
  (void)hipStreamSynchronize(pr::ctx_stream(o->ctx));
  (void)hipFree(o->scratch);            // the buffers are the caller's
  delete o;
}

int pr_onlineset_reset(pr_onlineset* o) {
  if (!o) return fail(nullptr, PR_EINVAL, "pr_onlineset_reset: set is NULL");
  ONSET_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  ONSET_HIP(o->ctx, hipMemsetAsync(o->v.state, 0, 4 * sizeof(int32_t), pr::ctx_stream(o->ctx)));
  return PR_OK;
}

int pr_onlineset_count(pr_onlineset* o, int32_t* count, int32_t* flags) {
  if (!o) return fail(nullptr, PR_EINVAL, "pr_onlineset_count: set is NULL");
  if (!count || !flags) return fail(o->ctx, PR_EINVAL, "pr_onlineset_count: a required pointer is NULL");
  ONSET_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  hipStream_t st = pr::ctx_stream(o->ctx);
  int32_t s[4];
  ONSET_HIP(o->ctx, hipMemcpyAsync(s, o->v.state, sizeof s, hipMemcpyDeviceToHost, st));
  ONSET_HIP(o->ctx, hipStreamSynchronize(st));
  *count = s[0];
  *flags = s[1];
  return PR_OK;
}

int pr_onlineset_match_dev(pr_onlineset* o, const double* d_sc, const double* d_m2dp, const double* d_delight, const int32_t* d_emitted,
                           int32_t mask_width, double p_weight, int32_t k, int32_t* d_idx, double* d_score, double* d_rows) {
  // (the checks that need no handle come first: with o == NULL their text goes to pr_last_error(NULL))
  pr_ctx* ctx = o ? o->ctx : nullptr;
  if (mask_width < 0) return fail(ctx, PR_EINVAL, "pr_onlineset_match_dev: mask_width=%d is negative", mask_width);
  if (!std::isfinite(p_weight)) return fail(ctx, PR_EINVAL, "pr_onlineset_match_dev: p_weight is not finite");
  if (k < 1 || k > pr::ONLINESET_MAX_K) return fail(ctx, PR_EINVAL, "pr_onlineset_match_dev: k=%d outside 1 .. %d", k, pr::ONLINESET_MAX_K);
  if (!o) return fail(nullptr, PR_EINVAL, "pr_onlineset_match_dev: set is NULL");
  if (k > o->v.max_k) return fail(ctx, PR_EINVAL, "pr_onlineset_match_dev: k=%d outside 1 .. max_k=%d", k, o->v.max_k);
  if (int rc = check_parts(ctx, "pr_onlineset_match_dev", o->v.kind, d_sc, d_m2dp, d_delight, "d_")) return rc;
  if (!d_idx || !d_score) return fail(ctx, PR_EINVAL, "pr_onlineset_match_dev: a required pointer is NULL (d_idx, d_score)");
  ONSET_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_onlineset_match(pr::ctx_stream(ctx), o->v, d_sc, d_m2dp, d_delight, d_emitted, mask_width, p_weight, k, d_idx, d_score,
                             d_rows ? d_rows : o->v.rows);
  ONSET_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_onlineset_append_dev(pr_onlineset* o, const double* d_sc, const double* d_m2dp, const double* d_delight, const int32_t* d_emitted,
                            int32_t* d_info) {
  if (!o) return fail(nullptr, PR_EINVAL, "pr_onlineset_append_dev: set is NULL");
  if (int rc = check_parts(o->ctx, "pr_onlineset_append_dev", o->v.kind, d_sc, d_m2dp, d_delight, "d_")) return rc;
  if (!d_info) return fail(o->ctx, PR_EINVAL, "pr_onlineset_append_dev: a required pointer is NULL (d_info)");
  ONSET_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  pr::launch_onlineset_append(pr::ctx_stream(o->ctx), o->v, d_sc, d_m2dp, d_delight, d_emitted, d_info);
  ONSET_HIP(o->ctx, hipGetLastError());
  return PR_OK;
}

int pr_onlineset_append(pr_onlineset* o, const double* sc, const double* m2dp, const double* delight, int32_t* info) {
  if (!o) return fail(nullptr, PR_EINVAL, "pr_onlineset_append: set is NULL");
  pr_ctx* ctx = o->ctx;
  if (int rc = check_parts(ctx, "pr_onlineset_append", o->v.kind, sc, m2dp, delight, "")) return rc;
  if (!info) return fail(ctx, PR_EINVAL, "pr_onlineset_append: a required pointer is NULL (info)");
  ONSET_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const bool fused = o->v.kind == PR_ONLINESET_FUSED;
  double* s_sc = fused ? o->stage_sig : nullptr;
  double* s_m2 = fused ? o->stage_sig + pr::ONLINESET_SC : nullptr;
  double* s_de = fused ? nullptr : o->stage_sig;
  hipError_t e = hipSuccess;
  if (fused) {
    e = hipMemcpyAsync(s_sc, sc, (size_t)pr::ONLINESET_SC * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s_m2, m2dp, (size_t)pr::ONLINESET_M2DP * sizeof(double), hipMemcpyHostToDevice, st);
  } else {
    e = hipMemcpyAsync(s_de, delight, (size_t)pr::ONLINESET_DELIGHT_LEN * sizeof(double), hipMemcpyHostToDevice, st);
  }
  int rc = PR_OK;
  if (e == hipSuccess) rc = pr_onlineset_append_dev(o, s_sc, s_m2, s_de, nullptr, o->stage_info);
  if (e == hipSuccess && rc == PR_OK) e = hipMemcpyAsync(info, o->stage_info, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);    // the host arrays are in flight until here
  if (rc != PR_OK) return rc;
  ONSET_HIP(ctx, e);
  ONSET_HIP(ctx, e2);
  return PR_OK;
}

}  // extern "C"
