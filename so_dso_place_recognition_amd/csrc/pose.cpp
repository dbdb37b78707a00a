// pose.cpp — host side of the pose seed and the stream-ordered verify chain (pose.hip): pr_relative_pose (host form, no
// context), pr_relative_pose_dev, pr_verify_select_dev and pr_verify_pairs_dev = seed -> pr_icp_pairs_dev over the [m][k][H] slots -> select.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "../../include/place_recognition.h"
#include "host_common.hpp"
#include "kernels.hpp"
#include "pose_seed.hpp"

static_assert(pr::POSE_SC == PR_POSE_SC && pr::POSE_M2DP == PR_POSE_M2DP && pr::POSE_DELIGHT == PR_POSE_DELIGHT, "pose types");

namespace {

struct Buf { void* p = nullptr; size_t cap = 0; };

struct PoseState {
  double* angles = nullptr;      // device: cos | sin of k D
  Buf T0, src, dst, Th, sth;     // the [m k H] slots of pr_verify_pairs_dev
};

using pr::fail;

// the angles of pr_sc_relative_pose: (double)k * D through the same cos / sin calls
void sc_angles(double* t) {
  const double D = 2.0 * M_PI / 60.0;
  for (int k = 0; k < pr::POSE_SC_ANGLES; k++) { t[k] = std::cos(k * D); t[pr::POSE_SC_ANGLES + k] = std::sin(k * D); }
}

// the context's state; its tables are uploaded once, by the first call (which therefore cannot be captured)
int state(pr_ctx* ctx, PoseState** out) {
  void*& slot = pr::ctx_pose(ctx);
  if (!slot) {
    PoseState* S = new PoseState;
    double t[2 * pr::POSE_SC_ANGLES];
    sc_angles(t);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&S->angles), sizeof t);
    if (e == hipSuccess) e = hipMemcpy(S->angles, t, sizeof t, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      if (S->angles) (void)hipFree(S->angles);
      delete S;
      return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pose tables: %s", hipGetErrorString(e));
    }
    slot = S;
  }
  *out = static_cast<PoseState*>(slot);
  return PR_OK;
}

// grow-only: a call whose shapes an earlier call covered allocates nothing (and can be captured)
int grow(pr_ctx* ctx, Buf& b, size_t bytes) {
  bytes = std::max<size_t>(bytes, 64);
  if (b.cap >= bytes) return PR_OK;
  if (b.p) {
    PR_CHECK_HIP(ctx, hipStreamSynchronize(pr::ctx_stream(ctx)));
    (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
  }
  PR_CHECK_HIP(ctx, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return PR_OK;
}

int check_type(pr_ctx* ctx, const char* fn, int type) {
  if (type != PR_POSE_SC && type != PR_POSE_M2DP && type != PR_POSE_DELIGHT) return fail(ctx, PR_EINVAL, "%s: type=%d (PR_POSE_SC | _M2DP | _DELIGHT)", fn, type);
  return PR_OK;
}

int check_slots(pr_ctx* ctx, const char* fn, int type, int32_t m, int32_t n_local, int32_t k, int32_t stride, int32_t H, const void* fq,
                const void* fd, const void* idx, const void* variant) {
  if (int rc = check_type(ctx, fn, type)) return rc;
  if (m < 0 || n_local < 0 || k < 0) return fail(ctx, PR_EINVAL, "%s: negative size (m=%d, n_local=%d, k=%d)", fn, m, n_local, k);
  if (H != 1 && H != 2) return fail(ctx, PR_EINVAL, "%s: H=%d (1 | 2)", fn, H);
  if (H == 2 && type == PR_POSE_DELIGHT) return fail(ctx, PR_EINVAL, "%s: H=2 with PR_POSE_DELIGHT: DELIGHT has one variant per pair", fn);
  if (stride < H) return fail(ctx, PR_EINVAL, "%s: variant_stride=%d < H=%d", fn, stride, H);
  if ((long long)m * k * H > 65535) return fail(ctx, PR_EINVAL, "%s: m k H = %lld > 65535", fn, (long long)m * k * H);
  if ((long long)m * k > 0 && (!fq || !idx || !variant || (n_local > 0 && !fd))) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  return PR_OK;
}

}  // namespace

namespace pr {
void pose_release(void* p) {
  if (!p) return;
  PoseState* S = static_cast<PoseState*>(p);
  if (S->angles) (void)hipFree(S->angles);
  for (Buf* b : {&S->T0, &S->src, &S->dst, &S->Th, &S->sth})
    if (b->p) (void)hipFree(b->p);
  delete S;
}
}  // namespace pr

extern "C" {

int pr_relative_pose(int type, const double* frames_q, const double* frames_db, const int32_t* variant, int32_t c, double* T) {
  const char* fn = "pr_relative_pose";
  if (int rc = check_type(nullptr, fn, type)) return rc;
  if (c < 0 || (c > 0 && (!frames_q || !frames_db || !variant || !T))) return fail(nullptr, PR_EINVAL, "%s: bad arguments (c=%d)", fn, c);
  const int nv = pr::pose_variants(type);
  for (int32_t i = 0; i < c; i++) {
    if (variant[i] < 0 || variant[i] >= nv) return fail(nullptr, PR_EINVAL, "%s: variant[%d] = %d is outside [0, %d)", fn, i, variant[i], nv);
    if (!(frames_q[16 * (size_t)i + 13] >= 3) || !(frames_db[16 * (size_t)i + 13] >= 3))
      return fail(nullptr, PR_EINVAL, "%s: frame %d has fewer than 3 points (slot 13)", fn, i);
  }
  double t[2 * pr::POSE_SC_ANGLES];
  sc_angles(t);
  for (int32_t i = 0; i < c; i++)
    pr::pose_seed(type, frames_q + 16 * (size_t)i, frames_db + 16 * (size_t)i, variant[i], t, t + pr::POSE_SC_ANGLES, T + 12 * (size_t)i);
  return PR_OK;
}

int pr_relative_pose_dev(pr_ctx* ctx, int type, const double* d_frames_q, int32_t m, const double* d_frames_db, int32_t n_local, int32_t db_row0,
                         int32_t k, const int32_t* d_idx, const int32_t* d_variant, int32_t variant_stride, int32_t H, double* d_T0,
                         int32_t* d_pair_src, int32_t* d_pair_dst) {
  const char* fn = "pr_relative_pose_dev";
  if (int rc = check_slots(ctx, fn, type, m, n_local, k, variant_stride, H, d_frames_q, d_frames_db, d_idx, d_variant)) return rc;
  if ((long long)m * k > 0 && (!d_T0 || !d_pair_src || !d_pair_dst)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  if ((long long)m * k == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  PoseState* S;
  if (int rc = state(ctx, &S)) return rc;
  pr::launch_pose_seed(pr::ctx_stream(ctx), type, d_frames_q, m, d_frames_db, n_local, db_row0, k, d_idx, d_variant, variant_stride, H, S->angles,
                       d_T0, d_pair_src, d_pair_dst);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_verify_select_dev(pr_ctx* ctx, const double* d_T_h, const pr_icp_stats* d_stats_h, int32_t c, int32_t H, double min_fitness, double max_rmse,
                         double* d_T, pr_icp_stats* d_stats, uint8_t* d_accepted, int32_t* d_hyp) {
  const char* fn = "pr_verify_select_dev";
  if (c < 0 || H < 1) return fail(ctx, PR_EINVAL, "%s: c=%d, H=%d", fn, c, H);
  if (std::isnan(min_fitness) || std::isnan(max_rmse)) return fail(ctx, PR_EINVAL, "%s: min_fitness / max_rmse is NaN", fn);
  if (c > 0 && (!d_T_h || !d_stats_h || !d_T || !d_stats || !d_accepted || !d_hyp)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  if (c == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  pr::launch_verify_select(pr::ctx_stream(ctx), d_T_h, reinterpret_cast<const pr::IcpStats*>(d_stats_h), c, H, min_fitness, max_rmse, d_T,
                           reinterpret_cast<pr::IcpStats*>(d_stats), d_accepted, d_hyp);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int pr_verify_pairs_dev(pr_ctx* ctx, int type, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const double* d_xyz_db,
                        const int64_t* d_offs_db, int32_t Ndb, const double* d_frames_q, const double* d_frames_db, int32_t m, int32_t n_local,
                        int32_t db_row0, int32_t k, const int32_t* d_idx, const int32_t* d_variant, int32_t variant_stride, int32_t H,
                        int32_t max_src_pts, int32_t max_dst_pts, int32_t max_iter, double max_corr, double tol_rmse, double tol_fitness,
                        int32_t min_inliers, double min_fitness, double max_rmse, double* d_T, pr_icp_stats* d_stats, uint8_t* d_accepted,
                        int32_t* d_hyp) {
  const char* fn = "pr_verify_pairs_dev";
  if (int rc = check_slots(ctx, fn, type, m, n_local, k, variant_stride, H, d_frames_q, d_frames_db, d_idx, d_variant)) return rc;
  if (std::isnan(min_fitness) || std::isnan(max_rmse)) return fail(ctx, PR_EINVAL, "%s: min_fitness / max_rmse is NaN", fn);
  const int32_t c = m * k, slots = c * H;
  if (int rc = pr::icp_check_pairs_args(ctx, fn, d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, slots, max_src_pts, max_dst_pts, max_iter, max_corr,
                                        tol_rmse, tol_fitness, min_inliers))
    return rc;
  if (c > 0 && (!d_T || !d_stats || !d_accepted || !d_hyp)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  PoseState* S = nullptr;
  if (c > 0) {
    PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
    if (int rc = state(ctx, &S)) return rc;
    if (int rc = grow(ctx, S->T0, (size_t)slots * 96)) return rc;
    if (int rc = grow(ctx, S->src, (size_t)slots * 4)) return rc;
    if (int rc = grow(ctx, S->dst, (size_t)slots * 4)) return rc;
    if (int rc = grow(ctx, S->Th, (size_t)slots * 96)) return rc;
    if (int rc = grow(ctx, S->sth, (size_t)slots * sizeof(pr_icp_stats))) return rc;
  }
  double* T0 = S ? static_cast<double*>(S->T0.p) : nullptr;
  int32_t* src = S ? static_cast<int32_t*>(S->src.p) : nullptr;
  int32_t* dst = S ? static_cast<int32_t*>(S->dst.p) : nullptr;
  double* Th = S ? static_cast<double*>(S->Th.p) : nullptr;
  pr_icp_stats* sth = S ? static_cast<pr_icp_stats*>(S->sth.p) : nullptr;
  if (int rc = pr_relative_pose_dev(ctx, type, d_frames_q, m, d_frames_db, n_local, db_row0, k, d_idx, d_variant, variant_stride, H, T0, src, dst))
    return rc;
  if (int rc = pr_icp_pairs_dev(ctx, d_xyz_q, d_offs_q, Nq, d_xyz_db, d_offs_db, Ndb, src, dst, slots, T0, max_src_pts, max_dst_pts, max_iter, max_corr,
                                tol_rmse, tol_fitness, min_inliers, Th, sth))
    return rc;
  return pr_verify_select_dev(ctx, Th, sth, c, H, min_fitness, max_rmse, d_T, d_stats, d_accepted, d_hyp);
}

}  // extern "C"
