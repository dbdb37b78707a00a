// handle_core.hpp — what the host files of the resident handle families share: the arena that lays out a handle's ONE scratch
// allocation (arena.hpp, HIP-free), the two-field base of every opaque handle with its destroy, the tail of a create, the transfer chain of
// a host form and the four-word state.  The rule the chain enforces: a host form never returns between its first enqueue and its synchronise.
#pragma once
#include <memory>
#include <new>

#include "arena.hpp"
#include "host_common.hpp"

namespace pr {

// What every opaque handle starts with: its context and its one device allocation (the buffers a view names besides are the caller's).
struct Handle {
  pr_ctx* ctx = nullptr;
  void* scratch = nullptr;
};

template <class H>
void destroy(H* h) {
  if (!h) return;
  (void)hipSetDevice(ctx_device(h->ctx));
  (void)hipStreamSynchronize(ctx_stream(h->ctx));
  (void)hipFree(h->scratch);
  delete h;
}

// A handle under construction: leaving create on any path but commit() frees the scratch and the handle, once.
struct Drop {
  template <class H>
  void operator()(H* h) const { (void)hipFree(h->scratch); delete h; }
};
template <class H>
using Owned = std::unique_ptr<H, Drop>;

// The tail of a create, first half: the device, the handle with its context, the scratch of `bytes`.  PR_ENOMEM / PR_EHIP with the text set.
template <class H>
int make(pr_ctx* ctx, const char* fn, size_t bytes, Owned<H>& h) {
  PR_CHECK_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  h.reset(new (std::nothrow) H);
  if (!h) return fail(ctx, PR_ENOMEM, "out of host memory");
  h->ctx = ctx;
  const hipError_t e = hipMalloc(&h->scratch, bytes);
  if (e != hipSuccess) {
    h->scratch = nullptr;
    return fail(ctx, hip_code(e), "%s: scratch of %zu bytes: %s", fn, bytes, hipGetErrorString(e));
  }
  return PR_OK;
}

// The copies of a host form (and the clears and uploads of a create) on the context's stream.  After the first failure - of a HIP call or of
// the form's own _dev call - every later step is skipped; finish() synchronises on every path, because the host arrays are in flight until then.
struct Transfer {
  hipStream_t st;
  hipError_t e = hipSuccess;
  int rc = PR_OK;

  explicit Transfer(pr_ctx* ctx) : st(ctx_stream(ctx)) {}
  bool ok() const { return e == hipSuccess && rc == PR_OK; }
  void note(hipError_t x) { if (ok()) e = x; }                       // the status of a launch or of a HIP call of the form's own
  // Zero bytes are skipped everywhere.  up() is for a REQUIRED input: a NULL source with bytes to copy is an error (the value checks of the
  // form should have refused it), never a silent run on stale staging.  up_opt() is for an optional input and down() for outputs, of which
  // every one may be optional: a NULL host array is skipped.
  void up(void* dst_dev, const void* src_host, size_t bytes) {
    if (ok() && bytes) e = src_host ? hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, st) : hipErrorInvalidValue;
  }
  void up_opt(void* dst_dev, const void* src_host, size_t bytes) {
    if (src_host) up(dst_dev, src_host, bytes);
  }
  void down(void* dst_host, const void* src_dev, size_t bytes) {
    if (ok() && dst_host && src_dev && bytes) e = hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st);
  }
  void fill(void* dst_dev, int value, size_t bytes) {
    if (ok() && bytes) e = hipMemsetAsync(dst_dev, value, bytes, st);
  }
  template <class F>
  void run(F&& dev) { if (ok()) rc = dev(); }                        // the form's _dev call: its code, when not PR_OK, is what finish returns
  void sync() {                                                      // keeps the first error; a form that reads what came down goes on if ok()
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
  }
  int finish(pr_ctx* ctx, const char* fn) {
    sync();
    if (rc != PR_OK) return rc;
    if (e != hipSuccess) return fail(ctx, hip_code(e), "%s: %s", fn, hipGetErrorString(e));
    return PR_OK;
  }
};

// The tail of a create, second half: after the family's fills and uploads on `t`, synchronise and hand the handle out.  A failure is PR_EHIP.
template <class H>
int commit(Owned<H>& h, Transfer& t, const char* fn, H** out) {
  t.sync();
  if (t.e != hipSuccess) return fail(h->ctx, PR_EHIP, "%s: clearing and filling the scratch failed: %s", fn, hipGetErrorString(t.e));
  *out = h.release();
  return PR_OK;
}

// The four-int state word of a family (which word means what is the family's): cleared in stream order, read with a synchronise.
inline int clear_state(pr_ctx* ctx, int32_t* d_state) {
  PR_CHECK_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  PR_CHECK_HIP(ctx, hipMemsetAsync(d_state, 0, 4 * sizeof(int32_t), ctx_stream(ctx)));
  return PR_OK;
}

inline int read_state(pr_ctx* ctx, const char* fn, const int32_t* d_state, int32_t out[4]) {
  PR_CHECK_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  Transfer t(ctx);
  t.down(out, d_state, 4 * sizeof(int32_t));
  return t.finish(ctx, fn);
}

}  // namespace pr
