// online.cpp — host side of the online signature database (online.hip): the opaque pr_online over the caller's two buffers
// with its scratch, the argument checks, the stream-ordered entry points and the host form of an append.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/place_recognition.h"
#include "kernels.hpp"
#include "online.hpp"

static_assert(pr::ONLINE_OVERFLOW == PR_ONLINE_OVERFLOW, "flag bit");
static_assert(PR_TYPE_SC == 0 && PR_TYPE_M2DP == 1, "online.hip tells the types apart by these values");

struct pr_online {
  pr_ctx* ctx = nullptr;
  pr::OnlineView v;
  void* scratch = nullptr;            // one allocation: rows, partial, stats and the staging of the host form
  double* stage_sig = nullptr;        // [sig_doubles]
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

#define ON_HIP(ctx, call)                                                                                         \
  do {                                                                                                            \
    hipError_t _e = (call);                                                                                       \
    if (_e != hipSuccess)                                                                                         \
      return fail(ctx, _e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
  } while (0)

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int pr_online_create(pr_ctx* ctx, int type, const pr_online_buffers* buffers, int32_t capacity, int32_t max_k, pr_online** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_online_create: out is NULL");
  *out = nullptr;
  if (!buffers) return fail(ctx, PR_EINVAL, "pr_online_create: buffers is NULL");
  if (!buffers->sig || !buffers->state) return fail(ctx, PR_EINVAL, "pr_online_create: a buffer is NULL (sig, state)");
  if (type != PR_TYPE_SC && type != PR_TYPE_M2DP) return fail(ctx, PR_EINVAL, "pr_online_create: type=%d is neither PR_TYPE_SC nor PR_TYPE_M2DP", type);
  if (capacity < 1 || capacity > PR_MAX_SIGS)
    return fail(ctx, PR_EINVAL, "pr_online_create: capacity=%d outside 1 .. PR_MAX_SIGS=%d", capacity, PR_MAX_SIGS);
  if (max_k < 1 || max_k > pr::ONLINE_MAX_K) return fail(ctx, PR_EINVAL, "pr_online_create: max_k=%d outside 1 .. %d", max_k, pr::ONLINE_MAX_K);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_online_create: ctx is NULL");
  ON_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr_online* o = new (std::nothrow) pr_online;
  if (!o) return fail(ctx, PR_ENOMEM, "out of host memory");
  o->ctx = ctx;
  pr::OnlineView& v = o->v;
  memset(&v, 0, sizeof v);
  v.sig = buffers->sig; v.state = buffers->state;
  v.type = type; v.capacity = capacity; v.max_k = max_k; v.NB = pr::online_blocks(capacity);
  v.sig_doubles = type == PR_TYPE_SC ? 2400 : 4 * 384;
  const size_t o_rows = 0, o_part = o_rows + up16((size_t)2 * capacity * 8), o_stats = o_part + up16((size_t)v.NB * 4 * 8), o_sig = o_stats + 32,
               o_info = o_sig + up16((size_t)v.sig_doubles * 8), total = o_info + 16;
  hipError_t e = hipMalloc(&o->scratch, total);
  if (e != hipSuccess) {
    delete o;
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_online_create: scratch: %s", hipGetErrorString(e));
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
    return fail(ctx, PR_EHIP, "pr_online_create: clearing the state failed: %s", hipGetErrorString(e));
  }
  *out = o;
  return PR_OK;
}

void pr_online_destroy(pr_online* o) {
  if (!o) return;
  (void)hipSetDevice(pr::ctx_device(o->ctx));
  (void)hipStreamSynchronize(pr::ctx_stream(o->ctx));
  (void)hipFree(o->scratch);            // the two buffers are the caller's
  delete o;
}

int pr_online_reset(pr_online* o) {
  if (!o) return fail(nullptr, PR_EINVAL, "pr_online_reset: database is NULL");
  ON_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  ON_HIP(o->ctx, hipMemsetAsync(o->v.state, 0, 4 * sizeof(int32_t), pr::ctx_stream(o->ctx)));
  return PR_OK;
}

int pr_online_count(pr_online* o, int32_t* count, int32_t* flags) {
  if (!o) return fail(nullptr, PR_EINVAL, "pr_online_count: database is NULL");
  if (!count || !flags) return fail(o->ctx, PR_EINVAL, "pr_online_count: a required pointer is NULL");
  ON_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  hipStream_t st = pr::ctx_stream(o->ctx);
  int32_t s[4];
  ON_HIP(o->ctx, hipMemcpyAsync(s, o->v.state, sizeof s, hipMemcpyDeviceToHost, st));
  ON_HIP(o->ctx, hipStreamSynchronize(st));
  *count = s[0];
  *flags = s[1];
  return PR_OK;
}

int pr_online_match_dev(pr_online* o, const double* d_sig, const int32_t* d_emitted, int32_t mask_width, double p_weight, int32_t k,
                        int32_t* d_idx, double* d_score, double* d_rows) {
  // (the checks that need no handle come first: with o == NULL their text goes to pr_last_error(NULL))
  pr_ctx* ctx = o ? o->ctx : nullptr;
  if (mask_width < 0) return fail(ctx, PR_EINVAL, "pr_online_match_dev: mask_width=%d is negative", mask_width);
  if (!std::isfinite(p_weight)) return fail(ctx, PR_EINVAL, "pr_online_match_dev: p_weight is not finite");
  if (k < 1 || k > pr::ONLINE_MAX_K) return fail(ctx, PR_EINVAL, "pr_online_match_dev: k=%d outside 1 .. %d", k, pr::ONLINE_MAX_K);
  if (!o) return fail(nullptr, PR_EINVAL, "pr_online_match_dev: database is NULL");
  if (k > o->v.max_k) return fail(ctx, PR_EINVAL, "pr_online_match_dev: k=%d outside 1 .. max_k=%d", k, o->v.max_k);
  if (!d_sig || !d_idx || !d_score) return fail(ctx, PR_EINVAL, "pr_online_match_dev: a required pointer is NULL (d_sig, d_idx, d_score)");
  ON_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_online_match(pr::ctx_stream(ctx), o->v, d_sig, d_emitted, mask_width, p_weight, k, d_idx, d_score, d_rows ? d_rows : o->v.rows);
  ON_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_online_append_dev(pr_online* o, const double* d_sig, const int32_t* d_emitted, int32_t* d_info) {
  if (!o) return fail(nullptr, PR_EINVAL, "pr_online_append_dev: database is NULL");
  if (!d_sig || !d_info) return fail(o->ctx, PR_EINVAL, "pr_online_append_dev: a required pointer is NULL (d_sig, d_info)");
  ON_HIP(o->ctx, hipSetDevice(pr::ctx_device(o->ctx)));
  pr::launch_online_append(pr::ctx_stream(o->ctx), o->v, d_sig, d_emitted, d_info);
  ON_HIP(o->ctx, hipGetLastError());
  return PR_OK;
}

int pr_online_append(pr_online* o, const double* sig, int32_t* info) {
  if (!o) return fail(nullptr, PR_EINVAL, "pr_online_append: database is NULL");
  pr_ctx* ctx = o->ctx;
  if (!sig || !info) return fail(ctx, PR_EINVAL, "pr_online_append: a required pointer is NULL (sig, info)");
  ON_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  hipError_t e = hipMemcpyAsync(o->stage_sig, sig, (size_t)o->v.sig_doubles * sizeof(double), hipMemcpyHostToDevice, st);
  int rc = PR_OK;
  if (e == hipSuccess) rc = pr_online_append_dev(o, o->stage_sig, nullptr, o->stage_info);
  if (e == hipSuccess && rc == PR_OK) e = hipMemcpyAsync(info, o->stage_info, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);    // sig is in flight until here
  if (rc != PR_OK) return rc;
  ON_HIP(ctx, e);
  ON_HIP(ctx, e2);
  return PR_OK;
}

}  // extern "C"
