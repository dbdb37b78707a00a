// reginfo.hip — the information of a registration at its final pose (no reference counterpart): the 6 x 6 normal matrix
// of the point or the plane metric over the correspondences of a pass the caller has already run, its inverse, the marginal spectra of
// rotation and translation with their weakest directions, a graded weakness test and a per-slot (w_rot, w_trans) for the pose graph.
// Every launch's grid depends on the create sizes and c only; every decision is made on the device.  Compiled with -ffp-contract=off.
//
// The rule (normative: include/place_recognition.h; restated in fp64 in tests/reginfo_np.py).
//   sums    grid (chunks of 256 source points, c): a chunk's sums - 11 for the point metric, 25 for the plane metric - by the fixed
//           tree: a 64-lane shuffle tree per wave, then the four waves in order, to [slot][chunk][REGINFO_NS] in the handle's scratch.
//   finish  one wave per slot, both metrics: lane k adds sum k over the slot's chunks in index order; lane 0: the flags, H, L D L^T,
//           Sigma by six solves, the two 3 x 3 Jacobi decompositions, the weakness test and the weights.  Every output row < c is written.
// A correspondent read from the caller's nn_idx is compared with out_capacity before an address is formed (plane metric; the point metric
// forms no address from it).  No floating-point atomics; no workgroup waits for another; plain C++, vector stores.
#include "icp_common.hpp"
#include "mapplane_normal.hpp"
#include "reginfo.hpp"

namespace pr {
namespace {

using icp_dev::IC_THREADS;
using icp_dev::transform;
using mapplane_dev::jacobi_rotate;
using mapplane_dev::MP_SWEEPS;

struct SlotShape { long long q0, o0; int ns; };

// the slot's first source row, first correspondence row and the points it reads = min(span, cloud, max_src_pts); false: the slot is OFF
__device__ __forceinline__ bool slot_shape(const RegInfoIn& in, int p, SlotShape& s) {
  const int src = in.pair_src[p];
  if (src < 0 || src >= in.Nq) return false;
  if (in.accepted && in.accepted[p] == 0) return false;
  s.o0 = in.out_offs[p];
  const long long span = in.out_offs[p + 1] - s.o0;
  if (span <= 0) return false;                                   // the pass switched the slot off (or its cloud is empty)
  s.q0 = in.offs_q[src];
  const long long cloud = in.offs_q[src + 1] - s.q0;
  long long n = span < cloud ? span : cloud;
  n = n < in.max_src ? n : in.max_src;
  s.ns = (int)(n < 0 ? 0 : n);
  return true;
}

template <int PLANE>
__global__ __launch_bounds__(IC_THREADS) void reginfo_sums_kernel(RegInfoIn in, double* __restrict__ part) {
  constexpr int NS = PLANE ? REGINFO_PLANE_SUMS : REGINFO_POINT_SUMS;
  __shared__ double red[IC_THREADS / 64][NS];
  const int p = blockIdx.y;
  SlotShape S;
  if (!slot_shape(in, p, S)) return;
  const int i0 = blockIdx.x * IC_THREADS, i = i0 + threadIdx.x;
  if (i0 >= S.ns) return;
  double a[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) a[k] = 0.0;
  if (i < S.ns) {
    const double bd = in.nn_d2[S.o0 + i];
    const int bj = in.nn_idx[S.o0 + i];
    const bool inl = bj >= 0 && bd < in.mc2 && (!PLANE || bj < in.ocap);      // bj < out_capacity before an address is formed
    if (inl) {
      const double* Tp = in.T + 12 * (size_t)p;
      const double* s = in.xyz_q + 3 * (size_t)(S.q0 + i);
      double pp[3];
      transform(Tp, s[0], s[1], s[2], pp);
      const double u[3] = {pp[0] - Tp[3], pp[1] - Tp[7], pp[2] - Tp[11]};     // the lever arm about the sensor position
      a[0] = 1.0; a[1] = bd;
      if (!PLANE) {
        a[2] = u[0]; a[3] = u[1]; a[4] = u[2];
        a[5] = u[0] * u[0]; a[6] = u[0] * u[1]; a[7] = u[0] * u[2]; a[8] = u[1] * u[1]; a[9] = u[1] * u[2]; a[10] = u[2] * u[2];
      } else if (in.ninfo[bj] > 0) {
        const double* q = in.world_xyz + 3 * (size_t)bj;
        const double nv[3] = {in.normals[3 * (size_t)bj], in.normals[3 * (size_t)bj + 1], in.normals[3 * (size_t)bj + 2]};
        const double e[3] = {pp[0] - q[0], pp[1] - q[1], pp[2] - q[2]};
        const double r = (nv[0] * e[0] + nv[1] * e[1]) + nv[2] * e[2];
        const double J[6] = {u[1] * nv[2] - u[2] * nv[1], u[2] * nv[0] - u[0] * nv[2], u[0] * nv[1] - u[1] * nv[0], nv[0], nv[1], nv[2]};
        a[2] = 1.0; a[3] = r * r;
        int m = 4;
#pragma unroll
        for (int r0 = 0; r0 < 6; r0++)
#pragma unroll
          for (int c0 = r0; c0 < 6; c0++) a[m++] = J[r0] * J[c0];
      }
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; k++) {
    double v = a[k];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS)
    part[((size_t)p * in.nchunks + blockIdx.x) * REGINFO_NS + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// eigenvalues l0 <= l1 <= l2 of the symmetric 3 x 3 block B[o .. o + 2][o .. o + 2] (its upper triangle is read) by mapplane_normal.hpp's
// Jacobi, and the unit eigenvector of l2 with its largest component positive
__device__ __forceinline__ void block_spectrum(const double (&B)[6][6], int o, double* l, double* dir) {
  double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = r; c < 3; c++) { A[r][c] = B[o + r][o + c]; A[c][r] = B[o + r][o + c]; }
  for (int sweep = 0; sweep < MP_SWEEPS; sweep++) {
    jacobi_rotate(A, V, 0, 1, 2);
    jacobi_rotate(A, V, 0, 2, 1);
    jacobi_rotate(A, V, 1, 2, 0);
  }
  double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2], t;
  int i0 = 0, i1 = 1, i2 = 2, ti;                                // a stable sort of three: the lower index first on ties
  if (l1 < l0) { t = l0; l0 = l1; l1 = t; ti = i0; i0 = i1; i1 = ti; }
  if (l2 < l1) { t = l1; l1 = l2; l2 = t; ti = i1; i1 = i2; i2 = ti; }
  if (l1 < l0) { t = l0; l0 = l1; l1 = t; ti = i0; i0 = i1; i1 = ti; }
  l[0] = l0; l[1] = l1; l[2] = l2;
  double e[3];
#pragma unroll
  for (int a = 0; a < 3; a++) e[a] = i2 == 0 ? V[a][0] : (i2 == 1 ? V[a][1] : V[a][2]);
  const double nrm = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
#pragma unroll
  for (int a = 0; a < 3; a++) e[a] = e[a] / nrm;
  double mag = fabs(e[0]), lead = e[0];                          // the component of largest magnitude, the lowest index on a tie
  if (fabs(e[1]) > mag) { mag = fabs(e[1]); lead = e[1]; }
  if (fabs(e[2]) > mag) lead = e[2];
  const bool flip = lead < 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++) dir[a] = flip ? -e[a] : e[a];
}

// one wave per slot
__global__ __launch_bounds__(64) void reginfo_finish_kernel(RegInfoIn in, int plane, const double* __restrict__ part, RegInfoParams prm,
                                                            RegInfoOut out) {
  __shared__ double sum[REGINFO_NS];
  const int p = blockIdx.x;
  SlotShape S;
  const bool on = slot_shape(in, p, S);
  const int ns = plane ? REGINFO_PLANE_SUMS : REGINFO_POINT_SUMS;
  if (threadIdx.x < REGINFO_NS) {
    double v = 0.0;
    if (on && (int)threadIdx.x < ns) {
      const int used = min(in.nchunks, (S.ns + IC_THREADS - 1) / IC_THREADS);
      const double* __restrict__ pp = part + (size_t)p * in.nchunks * REGINFO_NS + threadIdx.x;
      for (int k = 0; k < used; k++) v += pp[(size_t)k * REGINFO_NS];         // the chunks in index order
    }
    sum[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int flags = 0, n_inl = 0, n_used = 0, dof = 0;
  double H[6][6], Sg[6][6], spec[16], w_rot = 0.0, w_trans = 0.0;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c < 6; c++) { H[r][c] = 0.0; Sg[r][c] = 0.0; }
#pragma unroll
  for (int k = 0; k < 16; k++) spec[k] = 0.0;
  if (!on) {
    flags = REGINFO_OFF;
  } else {
    bool fin = true;
    for (int k = 0; k < 12; k++) fin = fin && isfinite(in.T[12 * (size_t)p + k]);
    for (int k = 0; k < ns; k++) fin = fin && isfinite(sum[k]);
    n_inl = (int)sum[0];                                         // the counts are sums of 1.0: always finite and exact
    n_used = plane ? (int)sum[2] : n_inl;
    dof = plane ? n_used - 6 : 3 * n_used - 6;
    if (!fin) {
      flags = REGINFO_NONFINITE;
    } else {
      double SSE;
      if (plane) {
        int m = 4;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
          for (int c = r; c < 6; c++) { H[r][c] = sum[m]; H[c][r] = sum[m]; m++; }
        SSE = sum[3];
      } else {
        // J = [-[u]x | I]: H_ww = (tr S) I - S (a diagonal entry is the sum of the other two diagonal sums), H_wv = [sum u]x, H_vv = n I
        const double n = sum[0], s0 = sum[2], s1 = sum[3], s2 = sum[4];
        H[0][0] = sum[8] + sum[10]; H[1][1] = sum[5] + sum[10]; H[2][2] = sum[5] + sum[8];
        H[0][1] = -sum[6]; H[1][0] = -sum[6]; H[0][2] = -sum[7]; H[2][0] = -sum[7]; H[1][2] = -sum[9]; H[2][1] = -sum[9];
        H[0][4] = -s2; H[0][5] = s1; H[1][3] = s2; H[1][5] = -s0; H[2][3] = -s1; H[2][4] = s0;
        H[4][0] = -s2; H[5][0] = s1; H[3][1] = s2; H[5][1] = -s0; H[3][2] = -s1; H[4][2] = s0;
        H[3][3] = n; H[4][4] = n; H[5][5] = n;
        SSE = sum[1];
      }
      spec[12] = SSE;
      if (n_used < prm.min_inliers || dof <= 0) {
        flags = REGINFO_TOO_FEW;
      } else {
        // L D L^T without pivoting in the order (w0, w1, w2, v0, v1, v2): mapplane_update_kernel's operations and test
        double L[6][6], d[6];
        bool ok = true;                                          // (no early exit: a failed pivot leaves values nobody reads)
#pragma unroll
        for (int k = 0; k < 6; k++) {
          double v = H[k][k];
#pragma unroll
          for (int m = 0; m < k; m++) v = v - (L[k][m] * d[m]) * L[k][m];
          d[k] = v;
          if (!isfinite(v) || !(v > 1e-12 * H[k][k])) ok = false;
#pragma unroll
          for (int i = k + 1; i < 6; i++) {
            double l = H[i][k];
#pragma unroll
            for (int m = 0; m < k; m++) l = l - (L[i][m] * d[m]) * L[k][m];
            L[i][k] = l / v;
          }
        }
        // Sigma = H^-1 by six solves, column j from the unit vector e_j: forward, the division by d, backward
        double X[6][6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
          double x[6];
#pragma unroll
          for (int i = 0; i < 6; i++) {
            double y = i == j ? 1.0 : 0.0;
#pragma unroll
            for (int m = 0; m < i; m++) y = y - L[i][m] * x[m];
            x[i] = y;
          }
#pragma unroll
          for (int i = 0; i < 6; i++) x[i] = x[i] / d[i];
#pragma unroll
          for (int i = 5; i >= 0; i--) {
            double z = x[i];
#pragma unroll
            for (int m = i + 1; m < 6; m++) z = z - L[m][i] * x[m];
            x[i] = z;
          }
#pragma unroll
          for (int i = 0; i < 6; i++) { X[i][j] = x[i]; ok = ok && isfinite(x[i]); }
        }
        if (!ok) {
          flags = REGINFO_SINGULAR;
        } else {
#pragma unroll
          for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) Sg[r][c] = X[r][c];
          block_spectrum(Sg, 0, spec, spec + 6);                 // cr0 <= cr1 <= cr2, dir_r
          block_spectrum(Sg, 3, spec + 3, spec + 9);             // ct0 <= ct1 <= ct2, dir_t
          if (!(spec[0] >= prm.min_ratio * spec[2])) flags |= REGINFO_WEAK_ROT;
          if (!(spec[3] >= prm.min_ratio * spec[5])) flags |= REGINFO_WEAK_TRANS;
          const double q = SSE / (double)dof, sm2 = prm.sigma_min * prm.sigma_min, s2 = q > sm2 ? q : sm2;
          spec[13] = s2;
          if (flags == 0) {
            const double xr = 1.0 / (s2 * spec[2]), xt = 1.0 / (s2 * spec[5]);
            w_rot = xr < prm.w_max ? xr : prm.w_max;
            w_trans = xt < prm.w_max ? xt : prm.w_max;
          }
        }
      }
    }
  }
  double* Ho = out.H + 36 * (size_t)p;
  double* Co = out.cov + 36 * (size_t)p;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c < 6; c++) { Ho[6 * r + c] = H[r][c]; Co[6 * r + c] = Sg[r][c]; }
#pragma unroll
  for (int k = 0; k < 16; k++) out.spec[16 * (size_t)p + k] = spec[k];
  out.w[2 * (size_t)p] = w_rot; out.w[2 * (size_t)p + 1] = w_trans;
  out.stat[4 * (size_t)p] = n_inl; out.stat[4 * (size_t)p + 1] = n_used; out.stat[4 * (size_t)p + 2] = dof; out.stat[4 * (size_t)p + 3] = flags;
  out.ok[p] = flags == 0 ? 1 : 0;
}

}  // namespace

void launch_reginfo_sums(hipStream_t st, const RegInfoIn& in, int plane, double* part) {
  if (in.c <= 0 || in.max_src <= 0) return;
  const dim3 grid((unsigned)in.nchunks, (unsigned)in.c), blk(IC_THREADS);
  if (plane) hipLaunchKernelGGL(reginfo_sums_kernel<1>, grid, blk, 0, st, in, part);
  else hipLaunchKernelGGL(reginfo_sums_kernel<0>, grid, blk, 0, st, in, part);
}

void launch_reginfo_finish(hipStream_t st, const RegInfoIn& in, int plane, const double* part, const RegInfoParams& prm, const RegInfoOut& out) {
  if (in.c > 0) hipLaunchKernelGGL(reginfo_finish_kernel, dim3((unsigned)in.c), dim3(64), 0, st, in, plane, part, prm, out);
}

}  // namespace pr
