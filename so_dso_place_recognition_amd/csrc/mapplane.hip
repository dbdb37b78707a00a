// mapplane.hip — point-to-plane scan-to-map registration (no reference counterpart): per-row normals of the world map
// through the localiser's voxel hash index, and a plane-metric refinement whose correspondence search IS maploc.hip's probe - the same
// launch, the same (j, d2) bytes.  Every launch's grid depends on the create sizes and c only; the row count and every decision are read
// and made on the device.  Compiled with -ffp-contract=off.
//
// The rule (normative: include/place_recognition.h; restated in fp64, without hashing, in tests/mapplane_np.py).
//   normals one lane per row of out_capacity.  R = state[0] clamped into 0 .. out_capacity.  Row j is processed iff it is INDEXED (j < R,
//           finite, in range and the row the table holds for its own key); every other row gets ninfo 0 and the normal 0.  The 27 keys
//           around floor(x_a / cell) in the probe's order, each contributing the row the table holds; kept iff d2 < fl(radius^2) with
//           d = q - x_j.  Sums of d and d d^T from 0.0 in visit order, C_ab = S_ab - (s_a s_b) / k, cyclic Jacobi (MP_SWEEPS sweeps, pivots
//           (0,1), (0,2), (1,2), a rotation skipped when the entry is exactly 0), eigenvalues sorted ascending with the lower index first
//           on ties, the validity test, the unit eigenvector of l0 with its largest component positive.
//   sums    grid (chunks of 256 source points, c) behind maploc.hip's probe: the chunk's 30 sums - inliers, sum d2, plane correspondents,
//           the 21 entries of sum J J^T (upper triangle, row-major) and the 6 of sum J r - by a fixed tree: 64-lane shuffle tree per wave,
//           then the four waves in order.  No floating-point atomics.
//   update  one wave per pair: lane k < 30 adds sum k over the chunks in index order; lane 0: statistics, stop rules, L D L^T, Rodrigues.
// A row word read from the table, and a correspondent read from the probe's rows, is compared with out_capacity before an address is
// formed.  Probes are bounded for loops; no workgroup waits for another; plain C++, vector stores.
#include "icp_common.hpp"
#include "kernels.hpp"
#include "mapplane_normal.hpp"

namespace pr {
namespace {

using namespace icp_dev;

// The normal of one row is mapplane_normal.hpp's row_normal, shared with mapgrow.hip (the rows around a keyframe's new rows): held_row's
// probe from the home slot (key * 0x9E3779B97F4A7C15ull) >> (64 - log2T) is a for loop of `step < Tn` steps, a row word is dropped by
// `row >= (u64)v.ocap` before an address is formed, and the Jacobi runs MP_SWEEPS = 8 sweeps.
using namespace mapplane_dev;

// one lane per world row
__global__ __launch_bounds__(256) void mapplane_normals_kernel(TableView v, double r2, int min_nbrs, double max_ratio,
                                                                double* __restrict__ normals, int* __restrict__ ninfo) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= v.ocap) return;
  int64_t R = v.state[0];
  R = R < 0 ? 0 : (R > v.ocap ? v.ocap : R);                     // a scribbled count must not turn into a row outside the buffers
  double n[3];
  int info;
  row_normal(v, j, R, r2, min_nbrs, max_ratio, n, &info);
  normals[3 * (size_t)j] = n[0]; normals[3 * (size_t)j + 1] = n[1]; normals[3 * (size_t)j + 2] = n[2];
  ninfo[j] = info;
}

// grid (chunks of 256 source points, pairs), behind the probe that left (nn_d, nn_j) at pair * ld
__global__ __launch_bounds__(IC_THREADS) void mapplane_sums_kernel(IcpClouds A, const double* __restrict__ T, const int* __restrict__ done,
                                                                    const double* __restrict__ nn_d, const int* __restrict__ nn_j, int ld,
                                                                    int nchunks, double mc2, const double* __restrict__ normals,
                                                                    const int* __restrict__ ninfo, double* __restrict__ part) {
  __shared__ double red[IC_THREADS / 64][MAPPLANE_SUMS];
  const int pair = blockIdx.y;
  if (done && done[pair]) return;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  const int i0 = blockIdx.x * IC_THREADS, i = i0 + threadIdx.x;
  if (i0 >= S.ns) return;
  double a[MAPPLANE_SUMS];
#pragma unroll
  for (int k = 0; k < MAPPLANE_SUMS; k++) a[k] = 0.0;
  if (i < S.ns) {
    const double bd = nn_d[(size_t)pair * ld + i];
    const int bj = nn_j[(size_t)pair * ld + i];
    if (bd < mc2 && bj >= 0 && bj < A.max_dst) {                 // bj < out_capacity before an address is formed
      a[0] = 1.0; a[1] = bd;
      if (ninfo[bj] > 0) {
        const double* Tp = T + 12 * (size_t)pair;
        const double* s = A.xyz_q + 3 * (size_t)(S.q0 + i);
        const double* q = A.xyz_d + 3 * (size_t)bj;
        const double nv[3] = {normals[3 * (size_t)bj], normals[3 * (size_t)bj + 1], normals[3 * (size_t)bj + 2]};
        double p[3];
        transform(Tp, s[0], s[1], s[2], p);
        const double u[3] = {p[0] - Tp[3], p[1] - Tp[7], p[2] - Tp[11]};       // the lever arm about the sensor position
        const double e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
        const double r = (nv[0] * e[0] + nv[1] * e[1]) + nv[2] * e[2];
        const double J[6] = {u[1] * nv[2] - u[2] * nv[1], u[2] * nv[0] - u[0] * nv[2], u[0] * nv[1] - u[1] * nv[0], nv[0], nv[1], nv[2]};
        a[2] = 1.0;
        int m = 3;
#pragma unroll
        for (int r0 = 0; r0 < 6; r0++)
#pragma unroll
          for (int c0 = r0; c0 < 6; c0++) a[m++] = J[r0] * J[c0];
#pragma unroll
        for (int r0 = 0; r0 < 6; r0++) a[24 + r0] = J[r0] * r;
      }
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < MAPPLANE_SUMS; k++) {
    double v = a[k];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < MAPPLANE_SUMS)
    part[((size_t)pair * nchunks + blockIdx.x) * MAPPLANE_SUMS + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// one wave per pair
__global__ __launch_bounds__(64) void mapplane_update_kernel(IcpClouds A, const double* __restrict__ part, int nchunks, IcpParams P, int final_pass,
                                                              double* __restrict__ T, IcpStats* __restrict__ stats, int* __restrict__ done,
                                                              double* __restrict__ prev) {
  __shared__ double sum[MAPPLANE_SUMS];
  const int pair = blockIdx.x;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  if (!final_pass && done[pair]) return;
  const int used = min(nchunks, (S.ns + IC_THREADS - 1) / IC_THREADS);
  if (threadIdx.x < MAPPLANE_SUMS) {
    const double* __restrict__ pp = part + (size_t)pair * nchunks * MAPPLANE_SUMS + threadIdx.x;
    double v = 0.0;
    for (int k = 0; k < used; k++) v += pp[(size_t)k * MAPPLANE_SUMS];        // the chunks in index order
    sum[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = sum[0];
  const double fitness = S.ns > 0 ? n / (double)S.ns : 0.0, rmse = n > 0.0 ? sqrt(sum[1] / n) : 0.0;
  IcpStats& st = stats[pair];
  if (final_pass) {
    st.fitness = fitness; st.rmse = rmse; st.n_inl = (int)n;
    if (st.status == ICP_RUNNING) st.status = ICP_MAX_ITER;
    return;
  }
  if (sum[2] < (double)P.min_inliers) { st.status = ICP_TOO_FEW; done[pair] = 1; return; }
  // A x = -b by L D L^T without pivoting, in the order (w0, w1, w2, v0, v1, v2)
  double M[6][6], L[6][6], d[6], x[6];
  {
    int m = 3;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = r; c < 6; c++) { M[r][c] = sum[m]; M[c][r] = sum[m]; m++; }
  }
  bool ok = true;                                                  // (no early exit: a failed pivot leaves values nobody reads)
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double v = M[k][k];
#pragma unroll
    for (int m = 0; m < k; m++) v = v - (L[k][m] * d[m]) * L[k][m];
    d[k] = v;
    if (!isfinite(v) || !(v > 1e-12 * M[k][k])) ok = false;
#pragma unroll
    for (int i = k + 1; i < 6; i++) {
      double l = M[i][k];
#pragma unroll
      for (int m = 0; m < k; m++) l = l - (L[i][m] * d[m]) * L[k][m];
      L[i][k] = l / v;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double y = -sum[24 + i];
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
  for (int i = 0; i < 6; i++) ok = ok && isfinite(x[i]);
  if (!ok) { st.status = ICP_DEGENERATE; done[pair] = 1; return; }
  // R <- Exp(w) R by Rodrigues: E = I + a K + b K^2 with K^2 = w w^T - th2 I; the series below th2 = 1e-4
  const double w[3] = {x[0], x[1], x[2]};
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double ca, cb;
  if (th2 < 1e-4) {
    ca = 1.0 - (th2 / 6.0) * (1.0 - (th2 / 20.0) * (1.0 - th2 / 42.0));
    cb = 0.5 - (th2 / 24.0) * (1.0 - (th2 / 30.0) * (1.0 - th2 / 56.0));
  } else {
    const double th = sqrt(th2);
    ca = sin(th) / th;
    cb = (1.0 - cos(th)) / th2;
  }
  double E[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) E[r][c] = cb * (w[r] * w[c]);
  for (int r = 0; r < 3; r++) E[r][r] = (1.0 - cb * th2) + E[r][r];
  E[0][1] = E[0][1] - ca * w[2]; E[0][2] = E[0][2] + ca * w[1];
  E[1][0] = E[1][0] + ca * w[2]; E[1][2] = E[1][2] - ca * w[0];
  E[2][0] = E[2][0] - ca * w[1]; E[2][1] = E[2][1] + ca * w[0];
  double* Tp = T + 12 * (size_t)pair;
  double Tn[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tn[4 * r + c] = (E[r][0] * Tp[c] + E[r][1] * Tp[4 + c]) + E[r][2] * Tp[8 + c];
    Tn[4 * r + 3] = Tp[4 * r + 3] + x[3 + r];
  }
  for (int k = 0; k < 12; k++) Tp[k] = Tn[k];
  const int it = st.iters;
  st.iters = it + 1;
  if (it > 0 && fabs(rmse - prev[2 * (size_t)pair]) < P.tol_rmse && fabs(fitness - prev[2 * (size_t)pair + 1]) < P.tol_fitness) {
    st.status = ICP_CONVERGED;
    done[pair] = 1;
  }
  prev[2 * (size_t)pair] = rmse;
  prev[2 * (size_t)pair + 1] = fitness;
}

}  // namespace

void launch_mapplane_normals(hipStream_t st, const MapLocView& v, double r2, int min_nbrs, double max_ratio, double* normals, int* ninfo) {
  const TableView tv{reinterpret_cast<const ulonglong2*>(v.table), v.xyz, v.state, v.ocap, v.cell, v.log2T};
  hipLaunchKernelGGL(mapplane_normals_kernel, dim3((unsigned)((v.ocap + 255) / 256)), dim3(256), 0, st, tv, r2, min_nbrs, max_ratio, normals, ninfo);
}

void launch_mapplane_sums(hipStream_t st, const IcpClouds& A, const double* T, const int* done, const double* nn_d, const int* nn_j, int ld,
                          int nchunks, double mc2, const double* normals, const int* ninfo, double* part) {
  if (A.c <= 0 || A.max_src <= 0) return;
  hipLaunchKernelGGL(mapplane_sums_kernel, dim3((A.max_src + IC_THREADS - 1) / IC_THREADS, A.c), dim3(IC_THREADS), 0, st, A, T, done, nn_d, nn_j, ld,
                     nchunks, mc2, normals, ninfo, part);
}

void launch_mapplane_update(hipStream_t st, const IcpClouds& A, const double* part, int nchunks, const IcpParams& P, int final_pass, double* T,
                            IcpStats* stats, int* done, double* prev) {
  if (A.c > 0) hipLaunchKernelGGL(mapplane_update_kernel, dim3(A.c), dim3(64), 0, st, A, part, nchunks, P, final_pass, T, stats, done, prev);
}

}  // namespace pr
