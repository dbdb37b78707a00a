// gist.cpp — host side of the GIST generator (GIST/src/test_gist.cpp:57-96 -> gist.cpp:54-94 -> libgist.cpp:914-951): argument
// checks, the filter tables in the reference's own arithmetic, the per-context cache of those tables and of the scratch, and the
// pr_gist_* entry points.  The kernels are in gist_gen.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/place_recognition.h"
#include "gist_tables.hpp"
#include "host_common.hpp"
#include "kernels.hpp"

namespace {

using pr::gist::GS;
using pr::gist::REF_PI;
static_assert(pr::gist::LD == pr::GIST_LD, "padded row stride");

struct GistState {
  float* circ = nullptr;                      // [GIST_LD][GIST_LD] whitening circulant
  float2* tw = nullptr;                       // [256] W256^m
  std::vector<std::pair<std::vector<int>, float*>> gabor;   // orientations per scale -> [nf][256][256]
  float* scratch = nullptr;
  size_t scratch_floats = 0;
};

using pr::fail;

int check_params(pr_ctx* ctx, const char* fn, int nblocks, int n_scale, const int32_t* orients) {
  if (nblocks < 1 || nblocks > 16) return fail(ctx, PR_EINVAL, "%s: nblocks must be 1..16 (got %d)", fn, nblocks);
  if (n_scale < 1 || n_scale > 8) return fail(ctx, PR_EINVAL, "%s: n_scale must be 1..8 (got %d)", fn, n_scale);
  if (!orients) return fail(ctx, PR_EINVAL, "%s: orients is NULL", fn);
  for (int s = 0; s < n_scale; s++)
    if (orients[s] < 1 || orients[s] > 32)
      return fail(ctx, PR_EINVAL, "%s: orients[%d] must be 1..32 (got %d)", fn, s, orients[s]);
  return PR_OK;
}

int check_args(pr_ctx* ctx, const char* fn, const void* img, int dtype, int32_t N, int32_t height, int32_t width, int nblocks, int n_scale,
               const int32_t* orients, const float* out) {
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  if (int rc = check_params(ctx, fn, nblocks, n_scale, orients)) return rc;
  if (dtype != PR_U8 && dtype != PR_F32) return fail(ctx, PR_EINVAL, "%s: dtype must be PR_U8 or PR_F32 (got %d)", fn, dtype);
  if (N < 0) return fail(ctx, PR_EINVAL, "%s: N = %d", fn, N);
  if (height != GS || width != GS)
    return fail(ctx, PR_EINVAL,
                "%s: images must be 256 x 256 (got %d x %d); GIST::extract (gist.cpp:62-75) first resizes with INTER_LANCZOS4 to the side "
                "whose ratio is smaller and centre-crops the other one: do that before the call (INTEGRATION.md)",
                fn, height, width);
  if (N > 0 && (!img || !out)) return fail(ctx, PR_EINVAL, "%s: img / out is NULL", fn);
  return PR_OK;
}

GistState* state(pr_ctx* ctx) {
  void*& slot = pr::ctx_gist(ctx);
  if (!slot) slot = new GistState;
  return static_cast<GistState*>(slot);
}

// Allocates a device buffer and uploads `bytes` from host memory on stream s, waiting for the copy; on any failure the buffer is freed
// and *d stays NULL, so nothing half-initialised is ever published.
int upload(pr_ctx* ctx, hipStream_t s, const void* h, size_t bytes, void** d) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    if (p) { (void)hipStreamSynchronize(s); (void)hipFree(p); }
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "GIST table upload failed: %s", hipGetErrorString(e));
  }
  *d = p;
  return PR_OK;
}

// tables of this parameter set, uploaded on first use (waits for the upload; a steady-state call does no transfer).  A table is recorded
// in the state only after its upload has completed.
int tables(pr_ctx* ctx, GistState* st, int n_scale, const int32_t* orients, float** gabor) {
  hipStream_t s = pr::ctx_stream(ctx);
  if (!st->circ || !st->tw) {
    const std::vector<float> C = pr::gist::circulant();
    std::vector<float2> tw(GS);
    for (int m = 0; m < GS; m++) tw[m] = make_float2((float)std::cos(2.0 * REF_PI * m / GS), (float)-std::sin(2.0 * REF_PI * m / GS));
    void *dc = nullptr, *dt = nullptr;
    if (int rc = upload(ctx, s, C.data(), C.size() * sizeof(float), &dc)) return rc;
    if (int rc = upload(ctx, s, tw.data(), tw.size() * sizeof(float2), &dt)) { (void)hipFree(dc); return rc; }
    if (st->circ) (void)hipFree(st->circ);
    if (st->tw) (void)hipFree(st->tw);
    st->circ = static_cast<float*>(dc);
    st->tw = static_cast<float2*>(dt);
  }
  const std::vector<int> key(orients, orients + n_scale);
  for (auto& e : st->gabor)
    if (e.first == key) { *gabor = e.second; return PR_OK; }
  const std::vector<float> G = pr::gist::gabor_table(n_scale, orients);
  void* d = nullptr;
  if (int rc = upload(ctx, s, G.data(), G.size() * sizeof(float), &d)) return rc;
  st->gabor.emplace_back(key, static_cast<float*>(d));
  *gabor = static_cast<float*>(d);
  return PR_OK;
}

// images per launch sequence: at most 32, and the row sums of a chunk at most 32 MiB
int chunk_size(int N, int nf, int nb) {
  int c = N < 32 ? N : 32;
  while (c > 1 && (size_t)c * nf * GS * nb > ((size_t)8 << 20)) c /= 2;
  return c;
}

}  // namespace

namespace pr {
void gist_release(void* p) {
  GistState* st = static_cast<GistState*>(p);
  if (!st) return;
  if (st->circ) (void)hipFree(st->circ);
  if (st->tw) (void)hipFree(st->tw);
  for (auto& e : st->gabor) (void)hipFree(e.second);
  if (st->scratch) (void)hipFree(st->scratch);
  delete st;
}
}  // namespace pr

extern "C" {

int pr_gist_signature_size(int32_t nblocks, int32_t n_scale, const int32_t* orients) {
  if (int rc = check_params(nullptr, "pr_gist_signature_size", nblocks, n_scale, orients)) return rc;
  int nf = 0;
  for (int s = 0; s < n_scale; s++) nf += orients[s];
  return nblocks * nblocks * nf;                  // gist.cpp:40-50 (use_color = false)
}

int pr_gist_generate_dev(pr_ctx* ctx, const void* img, int dtype, int32_t N, int32_t height, int32_t width, int32_t nblocks,
                         int32_t n_scale, const int32_t* orients, float* out) {
  if (int rc = check_args(ctx, "pr_gist_generate_dev", img, dtype, N, height, width, nblocks, n_scale, orients, out)) return rc;
  if (N == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  GistState* st = state(ctx);
  float* gabor = nullptr;
  if (int rc = tables(ctx, st, n_scale, orients, &gabor)) return rc;
  int nf = 0;
  for (int s = 0; s < n_scale; s++) nf += orients[s];
  const int chunk = chunk_size(N, nf, nblocks);
  const size_t need = pr::gist_scratch_floats(chunk, nf, nblocks);
  hipStream_t s = pr::ctx_stream(ctx);
  if (need > st->scratch_floats) {               // grow-only: a later call of at most this size allocates nothing
    if (st->scratch) {
      PR_CHECK_HIP(ctx, hipStreamSynchronize(s));
      PR_CHECK_HIP(ctx, hipFree(st->scratch));
      st->scratch = nullptr;
      st->scratch_floats = 0;
    }
    PR_CHECK_HIP(ctx, hipMalloc(&st->scratch, need * sizeof(float)));
    st->scratch_floats = need;
  }
  const size_t px = (size_t)GS * GS * (dtype == PR_U8 ? 1 : 4);
  const size_t D = (size_t)nblocks * nblocks * nf;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int n = N - c0 < chunk ? N - c0 : chunk;
    pr::launch_gist(s, static_cast<const char*>(img) + c0 * px, dtype == PR_U8, n, nblocks, nf, st->circ, gabor, st->tw, st->scratch,
                    out + c0 * D);
  }
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_gist_generate(pr_ctx* ctx, const void* img, int dtype, int32_t N, int32_t height, int32_t width, int32_t nblocks, int32_t n_scale,
                     const int32_t* orients, float* out) {
  if (int rc = check_args(ctx, "pr_gist_generate", img, dtype, N, height, width, nblocks, n_scale, orients, out)) return rc;
  if (N == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t s = pr::ctx_stream(ctx);
  const size_t in_bytes = (size_t)N * GS * GS * (dtype == PR_U8 ? 1 : 4);
  const size_t D = (size_t)pr_gist_signature_size(nblocks, n_scale, orients);
  void* din = nullptr;
  float* dout = nullptr;
  int rc = PR_OK;
  auto release = [&]() {
    (void)hipStreamSynchronize(s);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
  };
  hipError_t e = hipMalloc(&din, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&dout, (size_t)N * D * sizeof(float));
  if (e == hipSuccess) e = hipMemcpyAsync(din, img, in_bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    release();
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_gist_generate: %s", hipGetErrorString(e));
  }
  rc = pr_gist_generate_dev(ctx, din, dtype, N, height, width, nblocks, n_scale, orients, dout);
  if (rc == PR_OK) {
    e = hipMemcpyAsync(out, dout, (size_t)N * D * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(ctx, PR_EHIP, "pr_gist_generate: %s", hipGetErrorString(e));
  }
  release();
  if (rc) return rc;
  for (int32_t i = 0; i < N; i++)                 // bw_gist_scaletab refuses a descriptor with a NaN or Inf (libgist.cpp:936-945)
    for (size_t k = 0; k < D; k++)
      if (!std::isfinite(out[(size_t)i * D + k]))
        return fail(ctx, PR_ENAN, "pr_gist_generate: the descriptor of image %d is not valid (nan or inf); the reference returns NULL for it", i);
  return PR_OK;
}

}  // extern "C"
