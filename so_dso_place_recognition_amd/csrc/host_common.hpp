// host_common.hpp — what the host files of the library share: an error return that leaves its text in the context, and the check of a
// HIP call.  (pr_api.cpp's PR_HIP / PRE_HIP and pr_group.cpp's G_HIP report in other shapes and stay where they are.)  What the resident
// handle families share on top of this - layout arena, handle base, create tail, transfer chain, state word - is handle_core.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/place_recognition.h"
#include "kernels.hpp"

namespace pr {

inline int fail(pr_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int fail(pr_ctx* ctx, int code, const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  ctx_set_error(ctx, b);
  return code;
}

inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP; }

}  // namespace pr

// returns from the calling function (PR_ENOMEM / PR_EHIP, "<call> failed: <HIP's text>") when `call` does not succeed
#define PR_CHECK_HIP(ctx, call)                                                                     \
  do {                                                                                              \
    hipError_t _e = (call);                                                                         \
    if (_e != hipSuccess) return pr::fail(ctx, pr::hip_code(_e), "%s failed: %s", #call, hipGetErrorString(_e)); \
  } while (0)
