// reginfo.cpp — host side of the registration information (reginfo.hip): the opaque pr_reginfo, its ONE allocation, the
// argument checks, the two stream-ordered calls and their host forms, on the shared handle core (handle_core.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"
#include "reginfo.hpp"

static_assert(pr::REGINFO_OFF == PR_REGINFO_OFF && pr::REGINFO_NONFINITE == PR_REGINFO_NONFINITE && pr::REGINFO_TOO_FEW == PR_REGINFO_TOO_FEW &&
                  pr::REGINFO_SINGULAR == PR_REGINFO_SINGULAR && pr::REGINFO_WEAK_ROT == PR_REGINFO_WEAK_ROT &&
                  pr::REGINFO_WEAK_TRANS == PR_REGINFO_WEAK_TRANS,
              "flag bits");

namespace {

// where the parts of the one allocation lie (each on a 16-byte boundary); the formula of the header
struct Layout : pr::Arena {
  size_t part, s_xyz, s_offs, s_src, s_T, s_acc, s_ooffs, s_idx, s_d2, s_world, s_normals, s_ninfo, o_H, o_cov, o_spec, o_w, o_stat, o_ok;
};

Layout layout_of(int32_t pcap, int32_t max_src) {
  const size_t pc = (size_t)pcap, ld = (size_t)std::max(max_src, 1), nch = (ld + 255) / 256;
  Layout l;
  l.part = l.take(8 * pc * nch * pr::REGINFO_NS);
  l.s_xyz = l.take(24 * pc * ld); l.s_offs = l.take(8 * (pc + 1)); l.s_src = l.take(4 * pc); l.s_T = l.take(96 * pc); l.s_acc = l.take(pc);
  l.s_ooffs = l.take(8 * (pc + 1)); l.s_idx = l.take(4 * pc * ld); l.s_d2 = l.take(8 * pc * ld);
  l.s_world = l.take(24 * pc * ld); l.s_normals = l.take(24 * pc * ld); l.s_ninfo = l.take(4 * pc * ld);
  l.o_H = l.take(288 * pc); l.o_cov = l.take(288 * pc); l.o_spec = l.take(128 * pc); l.o_w = l.take(16 * pc); l.o_stat = l.take(16 * pc); l.o_ok = l.take(pc);
  return l;
}

bool sizes_ok(int32_t pcap, int32_t max_src) { return pcap >= 1 && pcap <= 65535 && max_src >= 0 && max_src <= (1 << 26); }

}  // namespace

struct pr_reginfo : pr::Handle {     // scratch: the partial sums and the staging of the host forms
  int32_t pair_cap = 0, max_src = 0, ld = 1, nchunks = 1;
  double* part = nullptr;             // [pair_capacity][nchunks][REGINFO_NS]
  Layout l;
};

namespace {

using pr::at;
using pr::fail;

struct Outputs { double* H; double* cov; double* spec; double* w; int32_t* stat; uint8_t* ok; };

// the value checks: no device, no handle needed (with ri == NULL their text goes to pr_last_error(NULL))
int check_values(pr_reginfo* ri, const char* fn, int plane, int32_t Nq, int32_t c, double max_corr, int32_t min_inliers, double min_ratio,
                 double sigma_min, double w_max) {
  pr_ctx* ctx = ri ? ri->ctx : nullptr;
  if (!(max_corr > 0.0) || !std::isfinite(max_corr)) return fail(ctx, PR_EINVAL, "%s: max_corr=%g must be positive and finite", fn, max_corr);
  if (!(sigma_min > 0.0) || !std::isfinite(sigma_min)) return fail(ctx, PR_EINVAL, "%s: sigma_min=%g must be positive and finite", fn, sigma_min);
  if (!(min_ratio >= 0.0) || !(min_ratio <= 1.0)) return fail(ctx, PR_EINVAL, "%s: min_ratio=%g outside [0, 1]", fn, min_ratio);
  if (!(w_max > 0.0)) return fail(ctx, PR_EINVAL, "%s: w_max=%g must be positive (+Inf is allowed)", fn, w_max);
  if (min_inliers < (plane ? 6 : 3)) return fail(ctx, PR_EINVAL, "%s: min_inliers=%d < %d", fn, min_inliers, plane ? 6 : 3);
  if (Nq < 0) return fail(ctx, PR_EINVAL, "%s: Nq=%d < 0", fn, Nq);
  if (!ri) return fail(nullptr, PR_EINVAL, "%s: handle is NULL", fn);
  if (c < 0 || c > ri->pair_cap) return fail(ctx, PR_EINVAL, "%s: c=%d outside 0 .. pair_capacity=%d", fn, c, ri->pair_cap);
  return PR_OK;
}

int check_pointers(pr_reginfo* ri, const char* fn, int plane, const void* xyz_q, const void* offs_q, const void* pair_src, int32_t c, const void* T,
                   const void* out_offs, const void* nn_idx, const void* nn_d2, const void* world, int64_t ocap, const void* normals,
                   const void* ninfo, const Outputs& o) {
  pr_ctx* ctx = ri->ctx;
  if (!offs_q || !out_offs) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (offs_q, out_offs)", fn);
  if (c > 0 && (!pair_src || !T || !o.H || !o.cov || !o.spec || !o.w || !o.stat || !o.ok))
    return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (pair_src, T, H, cov, spec, w, stat, ok)", fn);
  if (c > 0 && ri->max_src > 0 && (!xyz_q || !nn_idx || !nn_d2)) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (xyz_q, nn_idx, nn_d2)", fn);
  if (plane) {
    if (ocap < 1 || ocap > ((int64_t)1 << 29)) return fail(ctx, PR_EINVAL, "%s: out_capacity=%lld outside 1 .. 2^29", fn, (long long)ocap);
    if (!world || !normals || !ninfo) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL (world_xyz, normals, ninfo)", fn);
  }
  return PR_OK;
}

int run_dev(pr_reginfo* ri, int plane, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
            const double* d_T, const uint8_t* d_accepted, const int64_t* d_out_offs, const int32_t* d_nn_idx, const double* d_nn_d2,
            const double* d_world_xyz, int64_t out_capacity, const double* d_normals, const int32_t* d_ninfo, double max_corr,
            int32_t min_inliers, double min_ratio, double sigma_min, double w_max, const Outputs& o) {
  const char* fn = plane ? "pr_reginfo_plane_dev" : "pr_reginfo_point_dev";
  if (int rc = check_values(ri, fn, plane, Nq, c, max_corr, min_inliers, min_ratio, sigma_min, w_max)) return rc;
  if (int rc = check_pointers(ri, fn, plane, d_xyz_q, d_offs_q, d_pair_src, c, d_T, d_out_offs, d_nn_idx, d_nn_d2, d_world_xyz, out_capacity,
                              d_normals, d_ninfo, o))
    return rc;
  if (c == 0) return PR_OK;
  pr_ctx* ctx = ri->ctx;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t st = pr::ctx_stream(ctx);
  const pr::RegInfoIn in{d_xyz_q, d_offs_q, Nq, d_pair_src, c, d_T, d_accepted, d_out_offs, d_nn_idx, d_nn_d2, ri->max_src, ri->nchunks,
                         max_corr * max_corr, d_world_xyz, out_capacity, d_normals, d_ninfo};
  const pr::RegInfoParams prm{min_inliers, min_ratio, sigma_min, w_max};
  const pr::RegInfoOut out{o.H, o.cov, o.spec, o.w, o.stat, o.ok};
  pr::launch_reginfo_sums(st, in, plane, ri->part);
  pr::launch_reginfo_finish(st, in, plane, ri->part, prm, out);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

int run_host(pr_reginfo* ri, int plane, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T,
             const uint8_t* accepted, const int64_t* out_offs, const int32_t* nn_idx, const double* nn_d2, const double* world_xyz,
             int64_t out_capacity, const double* normals, const int32_t* ninfo, double max_corr, int32_t min_inliers, double min_ratio,
             double sigma_min, double w_max, const Outputs& o) {
  const char* fn = plane ? "pr_reginfo_plane" : "pr_reginfo_point";
  if (int rc = check_values(ri, fn, plane, Nq, c, max_corr, min_inliers, min_ratio, sigma_min, w_max)) return rc;
  if (int rc = check_pointers(ri, fn, plane, xyz_q, offs_q, pair_src, c, T, out_offs, nn_idx, nn_d2, world_xyz, out_capacity, normals, ninfo, o))
    return rc;
  pr_ctx* ctx = ri->ctx;
  const int64_t rows = (int64_t)ri->pair_cap * ri->ld;
  if (Nq > ri->pair_cap) return fail(ctx, PR_EINVAL, "%s: Nq=%d exceeds pair_capacity=%d (the staging of the host forms)", fn, Nq, ri->pair_cap);
  if (offs_q[0] < 0) return fail(ctx, PR_EINVAL, "%s: offs_q is not ascending from 0", fn);
  for (int32_t i = 0; i < Nq; i++) if (offs_q[i + 1] < offs_q[i]) return fail(ctx, PR_EINVAL, "%s: offs_q is not ascending", fn);
  if (offs_q[Nq] > rows) return fail(ctx, PR_EINVAL, "%s: %lld source points exceed pair_capacity x max(max_src_pts, 1)", fn, (long long)offs_q[Nq]);
  if (out_offs[0] < 0) return fail(ctx, PR_EINVAL, "%s: out_offs is not ascending from 0", fn);
  for (int32_t i = 0; i < c; i++) if (out_offs[i + 1] < out_offs[i]) return fail(ctx, PR_EINVAL, "%s: out_offs is not ascending", fn);
  if (out_offs[c] > rows) return fail(ctx, PR_EINVAL, "%s: %lld correspondences exceed pair_capacity x max(max_src_pts, 1)", fn, (long long)out_offs[c]);
  if ((offs_q[Nq] > 0 && !xyz_q) || (out_offs[c] > 0 && (!nn_idx || !nn_d2))) return fail(ctx, PR_EINVAL, "%s: a required pointer is NULL", fn);
  if (plane && out_capacity > rows)
    return fail(ctx, PR_EINVAL, "%s: out_capacity=%lld exceeds pair_capacity x max(max_src_pts, 1) (the staging of the host forms)", fn,
                (long long)out_capacity);
  if (c == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  void* b = ri->scratch;
  const Layout& l = ri->l;
  const size_t oc = plane ? (size_t)out_capacity : 0, C = (size_t)c;
  double *s_xyz = at<double>(b, l.s_xyz), *s_T = at<double>(b, l.s_T), *s_d2 = at<double>(b, l.s_d2), *s_world = at<double>(b, l.s_world),
         *s_normals = at<double>(b, l.s_normals);
  int64_t *s_offs = at<int64_t>(b, l.s_offs), *s_ooffs = at<int64_t>(b, l.s_ooffs);
  int32_t *s_src = at<int32_t>(b, l.s_src), *s_idx = at<int32_t>(b, l.s_idx), *s_ninfo = at<int32_t>(b, l.s_ninfo);
  uint8_t* s_acc = at<uint8_t>(b, l.s_acc);
  const Outputs d{at<double>(b, l.o_H), at<double>(b, l.o_cov), at<double>(b, l.o_spec), at<double>(b, l.o_w), at<int32_t>(b, l.o_stat),
                  at<uint8_t>(b, l.o_ok)};
  pr::Transfer t(ctx);
  t.up(s_offs, offs_q, ((size_t)Nq + 1) * 8);
  t.up(s_xyz, xyz_q, (size_t)offs_q[Nq] * 24);
  t.up(s_src, pair_src, C * 4);
  t.up(s_T, T, C * 96);
  t.up_opt(s_acc, accepted, C);
  t.up(s_ooffs, out_offs, (C + 1) * 8);
  t.up(s_idx, nn_idx, (size_t)out_offs[c] * 4);
  t.up(s_d2, nn_d2, (size_t)out_offs[c] * 8);
  t.up(s_world, world_xyz, oc * 24);                                // (the plane form's alone)
  t.up(s_normals, normals, oc * 24);
  t.up(s_ninfo, ninfo, oc * 4);
  t.run([&] {
    return run_dev(ri, plane, s_xyz, s_offs, Nq, s_src, c, s_T, accepted ? s_acc : nullptr, s_ooffs, s_idx, s_d2, s_world, out_capacity, s_normals,
                   s_ninfo, max_corr, min_inliers, min_ratio, sigma_min, w_max, d);
  });
  t.down(o.H, d.H, C * 288);
  t.down(o.cov, d.cov, C * 288);
  t.down(o.spec, d.spec, C * 128);
  t.down(o.w, d.w, C * 16);
  t.down(o.stat, d.stat, C * 16);
  t.down(o.ok, d.ok, C);
  return t.finish(ctx, fn);
}

}  // namespace

extern "C" {

int64_t pr_reginfo_scratch_bytes(int32_t pair_capacity, int32_t max_src_pts) {
  if (!sizes_ok(pair_capacity, max_src_pts)) return 0;
  return (int64_t)layout_of(pair_capacity, max_src_pts).total;
}

int pr_reginfo_create(pr_ctx* ctx, int32_t pair_capacity, int32_t max_src_pts, pr_reginfo** out) {
  if (!out) return fail(ctx, PR_EINVAL, "pr_reginfo_create: out is NULL");
  *out = nullptr;
  if (pair_capacity < 1 || pair_capacity > 65535) return fail(ctx, PR_EINVAL, "pr_reginfo_create: pair_capacity=%d outside 1 .. 65535", pair_capacity);
  if (max_src_pts < 0 || max_src_pts > (1 << 26)) return fail(ctx, PR_EINVAL, "pr_reginfo_create: max_src_pts=%d outside 0 .. 2^26", max_src_pts);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_reginfo_create: ctx is NULL");
  const Layout l = layout_of(pair_capacity, max_src_pts);
  pr::Owned<pr_reginfo> ri;
  if (int rc = pr::make(ctx, "pr_reginfo_create", l.total, ri)) return rc;
  ri->pair_cap = pair_capacity; ri->max_src = max_src_pts;
  ri->ld = std::max(max_src_pts, 1); ri->nchunks = (ri->ld + 255) / 256;
  ri->l = l;
  ri->part = at<double>(ri->scratch, l.part);
  pr::Transfer t(ctx);
  t.fill(ri->scratch, 0, l.total);
  return pr::commit(ri, t, "pr_reginfo_create", out);
}

void pr_reginfo_destroy(pr_reginfo* ri) { pr::destroy(ri); }

int pr_reginfo_point_dev(pr_reginfo* ri, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                         const double* d_T, const uint8_t* d_accepted, const int64_t* d_out_offs, const int32_t* d_nn_idx, const double* d_nn_d2,
                         double max_corr, int32_t min_inliers, double min_ratio, double sigma_min, double w_max, double* d_H, double* d_cov,
                         double* d_spec, double* d_w, int32_t* d_stat, uint8_t* d_ok) {
  return run_dev(ri, 0, d_xyz_q, d_offs_q, Nq, d_pair_src, c, d_T, d_accepted, d_out_offs, d_nn_idx, d_nn_d2, nullptr, 0, nullptr, nullptr, max_corr,
                 min_inliers, min_ratio, sigma_min, w_max, Outputs{d_H, d_cov, d_spec, d_w, d_stat, d_ok});
}

int pr_reginfo_plane_dev(pr_reginfo* ri, const double* d_xyz_q, const int64_t* d_offs_q, int32_t Nq, const int32_t* d_pair_src, int32_t c,
                         const double* d_T, const uint8_t* d_accepted, const int64_t* d_out_offs, const int32_t* d_nn_idx, const double* d_nn_d2,
                         const double* d_world_xyz, int64_t out_capacity, const double* d_normals, const int32_t* d_ninfo, double max_corr,
                         int32_t min_inliers, double min_ratio, double sigma_min, double w_max, double* d_H, double* d_cov, double* d_spec,
                         double* d_w, int32_t* d_stat, uint8_t* d_ok) {
  return run_dev(ri, 1, d_xyz_q, d_offs_q, Nq, d_pair_src, c, d_T, d_accepted, d_out_offs, d_nn_idx, d_nn_d2, d_world_xyz, out_capacity, d_normals,
                 d_ninfo, max_corr, min_inliers, min_ratio, sigma_min, w_max, Outputs{d_H, d_cov, d_spec, d_w, d_stat, d_ok});
}

int pr_reginfo_point(pr_reginfo* ri, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T,
                     const uint8_t* accepted, const int64_t* out_offs, const int32_t* nn_idx, const double* nn_d2, double max_corr,
                     int32_t min_inliers, double min_ratio, double sigma_min, double w_max, double* H, double* cov, double* spec, double* w,
                     int32_t* stat, uint8_t* ok) {
  return run_host(ri, 0, xyz_q, offs_q, Nq, pair_src, c, T, accepted, out_offs, nn_idx, nn_d2, nullptr, 0, nullptr, nullptr, max_corr, min_inliers,
                  min_ratio, sigma_min, w_max, Outputs{H, cov, spec, w, stat, ok});
}

int pr_reginfo_plane(pr_reginfo* ri, const double* xyz_q, const int64_t* offs_q, int32_t Nq, const int32_t* pair_src, int32_t c, const double* T,
                     const uint8_t* accepted, const int64_t* out_offs, const int32_t* nn_idx, const double* nn_d2, const double* world_xyz,
                     int64_t out_capacity, const double* normals, const int32_t* ninfo, double max_corr, int32_t min_inliers, double min_ratio,
                     double sigma_min, double w_max, double* H, double* cov, double* spec, double* w, int32_t* stat, uint8_t* ok) {
  return run_host(ri, 1, xyz_q, offs_q, Nq, pair_src, c, T, accepted, out_offs, nn_idx, nn_d2, world_xyz, out_capacity, normals, ninfo, max_corr,
                  min_inliers, min_ratio, sigma_min, w_max, Outputs{H, cov, spec, w, stat, ok});
}

}  // extern "C"
