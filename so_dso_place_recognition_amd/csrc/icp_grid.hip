// icp_grid.hip — the exact uniform-grid correspondence search of the ICP refinement (the normative arithmetic is
// tests/icp_grid_np.py = tests/icp_np.py masked to d2 < max_corr^2).  Compiled with -ffp-contract=off.
//
// Only correspondences with d2 < max_corr^2 enter an update or a statistic, and the target does not move during a refinement: a grid over
// the finite target points, built once per call and per pair slot (box -> clear -> count -> scan -> scatter, integer atomics only), is
// probed in the 27 cells around every transformed source point.  The cell edge h = max(max_corr (1 + 2^-10), largest extent / G) makes
// d2 < max_corr^2 imply a cell-index difference of at most 1 per axis despite the rounding of (x - x0) / h on both sides (the containment
// argument of DESIGN.md 4.14), so the probe sees every candidate the brute-force scan would have kept, forms d2 by the same operations on
// the same rounded p' and keeps "smaller d2, then smaller j": the first-minimum rule, whatever order the scatter left inside a cell.  The
// chunk's 17 inlier sums come from icp_common.hpp's chunk_sums - the code the brute-force combining launch runs - over chunks of 256
// source points, so a refinement returns the bytes of the brute-force split path.
#include "icp_common.hpp"
#include "kernels.hpp"

namespace pr {
namespace {

using namespace icp_dev;

constexpr int SCAN_THREADS = 1024;

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the cell edge and a coordinate's (unclamped) cell along one axis: the two formulas of the containment argument
__device__ __forceinline__ double cell_edge(double max_corr, double ext, int G) { return fmax(max_corr * ICP_GRID_SLACK, ext / (double)G); }
__device__ __forceinline__ double cell_coord(double x, double x0, double h) { return floor((x - x0) / h); }

// a finite target point's cell: every axis clamped into the grid (a NaN quotient - h infinite, one cell - goes to cell 0)
__device__ __forceinline__ int target_cell(const IcpGridBox& B, double x, double y, double z) {
  const int cx = (int)fmin(fmax(cell_coord(x, B.x0[0], B.h), 0.0), (double)(B.n[0] - 1));
  const int cy = (int)fmin(fmax(cell_coord(y, B.x0[1], B.h), 0.0), (double)(B.n[1] - 1));
  const int cz = (int)fmin(fmax(cell_coord(z, B.x0[2], B.h), 0.0), (double)(B.n[2] - 1));
  return (cz * B.n[1] + cy) * B.n[0] + cx;
}

// one workgroup per pair slot: the box of the target's finite points, h and the cells per axis (n = 0: no finite point, or no pair)
__global__ __launch_bounds__(IC_THREADS) void icp_grid_box_kernel(IcpClouds A, IcpGrid gr, double max_corr) {
  __shared__ double lo[3][IC_THREADS], hi[3][IC_THREADS];
  const int pair = blockIdx.x;
  PairShape S;
  const bool has = pair_shape(A, pair, S);
  double l[3] = {INFINITY, INFINITY, INFINITY}, u[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (has) {
    const double* __restrict__ xd = A.xyz_d + 3 * (size_t)S.d0;
    for (int j = threadIdx.x; j < S.nd; j += IC_THREADS) {
      const double q[3] = {xd[3 * (size_t)j], xd[3 * (size_t)j + 1], xd[3 * (size_t)j + 2]};
      if (!finite3(q[0], q[1], q[2])) continue;
#pragma unroll
      for (int a = 0; a < 3; a++) { l[a] = fmin(l[a], q[a]); u[a] = fmax(u[a], q[a]); }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) { lo[a][threadIdx.x] = l[a]; hi[a][threadIdx.x] = u[a]; }
  __syncthreads();
  for (int o = IC_THREADS / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        lo[a][threadIdx.x] = fmin(lo[a][threadIdx.x], lo[a][threadIdx.x + o]);
        hi[a][threadIdx.x] = fmax(hi[a][threadIdx.x], hi[a][threadIdx.x + o]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  IcpGridBox B;
  B.flags = 0;
  if (!(lo[0][0] <= hi[0][0])) {                       // no finite point
    for (int a = 0; a < 3; a++) { B.x0[a] = 0.0; B.n[a] = 0; }
    B.h = 0.0;
  } else {
    double ext = 0.0;
    for (int a = 0; a < 3; a++) { B.x0[a] = lo[a][0]; ext = fmax(ext, hi[a][0] - lo[a][0]); }
    B.h = cell_edge(max_corr, ext, gr.G);
    if (!(B.h < INFINITY)) {                           // an extent or max_corr past the doubles' range: one cell, the probe scans it whole
      B.flags = 1;
      for (int a = 0; a < 3; a++) B.n[a] = 1;
    } else {
      for (int a = 0; a < 3; a++) {                    // the largest point's own cell + 1: <= G + 1
        const double top = cell_coord(hi[a][0], B.x0[a], B.h);
        B.n[a] = (int)fmin(fmax(top, 0.0), (double)gr.G) + 1;
      }
    }
  }
  gr.box[pair] = B;
}

// grid (target chunks of 256 points, pairs): a finite target point adds one to its cell, or (scatter) takes the cell's next place
template <bool SCATTER>
__global__ __launch_bounds__(IC_THREADS) void icp_grid_fill_kernel(IcpClouds A, IcpGrid gr) {
  const int pair = blockIdx.y;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  const int j = blockIdx.x * IC_THREADS + threadIdx.x;
  if (j >= S.nd) return;
  const IcpGridBox B = gr.box[pair];
  if (B.n[0] <= 0) return;
  const double* q = A.xyz_d + 3 * (size_t)(S.d0 + j);
  const double x = q[0], y = q[1], z = q[2];
  if (!finite3(x, y, z)) return;
  int* cell = gr.ends + (size_t)pair * gr.cells + target_cell(B, x, y, z);
  if (!SCATTER) { atomicAdd(cell, 1); return; }
  const int pos = atomicAdd(cell, 1);
  if (pos >= 0 && pos < A.max_dst) gr.sorted[(size_t)pair * A.max_dst + pos] = j;
}

// one workgroup per pair slot: counts -> exclusive starts, in place (a lane sums a run of cells, the runs' sums are scanned in LDS)
__global__ __launch_bounds__(SCAN_THREADS) void icp_grid_scan_kernel(IcpGrid gr) {
  __shared__ int sc[SCAN_THREADS];
  const int pair = blockIdx.x;
  const IcpGridBox B = gr.box[pair];
  const long long used = (long long)B.n[0] * B.n[1] * B.n[2];
  const int n = (int)(used < gr.cells ? used : gr.cells);
  int* __restrict__ e = gr.ends + (size_t)pair * gr.cells;
  const int per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
  const long long b0 = (long long)threadIdx.x * per;
  const int k0 = (int)(b0 < n ? b0 : n), k1 = (int)(b0 + per < n ? b0 + per : n);
  int sum = 0;
  for (int k = k0; k < k1; k++) sum += e[k];
  sc[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < SCAN_THREADS; o <<= 1) {
    const int t = threadIdx.x >= o ? sc[threadIdx.x - o] : 0;
    __syncthreads();
    sc[threadIdx.x] += t;
    __syncthreads();
  }
  int run = sc[threadIdx.x] - sum;
  for (int k = k0; k < k1; k++) { const int v = e[k]; e[k] = run; run += v; }
}

// grid (chunks of 256 source points, pairs)
__global__ __launch_bounds__(IC_THREADS) void icp_grid_probe_kernel(IcpClouds A, IcpGrid gr, const double* __restrict__ T, const int* __restrict__ done,
                                                                     int ld, const long long* __restrict__ base, double* __restrict__ nn_d,
                                                                     int* __restrict__ nn_j, double mc2, double* __restrict__ part, int nchunks) {
  __shared__ double red[IC_THREADS / 64][ICP_PARTIAL];
  const int pair = blockIdx.y;
  if (done && done[pair]) return;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  const int i0 = blockIdx.x * IC_THREADS, i = i0 + threadIdx.x;
  if (i0 >= S.ns) return;
  double bd = INFINITY;
  int bj = -1;
  if (i < S.ns) {
    const IcpGridBox B = gr.box[pair];
    const double* s = A.xyz_q + 3 * (size_t)(S.q0 + i);
    double p[3];
    transform(T + 12 * (size_t)pair, s[0], s[1], s[2], p);
    bool ok = B.n[0] > 0 && finite3(p[0], p[1], p[2]);
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (ok && !(B.flags & 1)) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double t = cell_coord(p[a], B.x0[a], B.h);               // the range test in floating point: 1e300 never reaches an int
        const bool in = t >= -1.0 && t <= (double)B.n[a];              // at most one cell outside the box (a NaN fails)
        ok = ok && in;
        const int c = in ? (int)t : 0;
        lo[a] = c > 0 ? c - 1 : 0;
        hi[a] = c + 1 < B.n[a] ? c + 1 : B.n[a] - 1;
      }
    }
    if (ok) {
      const int* __restrict__ e = gr.ends + (size_t)pair * gr.cells;
      const int* __restrict__ sorted = gr.sorted + (size_t)pair * A.max_dst;
      const double* __restrict__ xd = A.xyz_d + 3 * (size_t)S.d0;
      for (int z = lo[2]; z <= hi[2]; z++)
        for (int y = lo[1]; y <= hi[1]; y++) {
          const int row = (z * B.n[1] + y) * B.n[0];                     // the row's (up to) three cells are one run of `sorted`
          const int c0 = row + lo[0], c1 = row + hi[0];
          const int k0 = c0 > 0 ? e[c0 - 1] : 0, k1 = e[c1];
          for (int k = k0; k < k1; k++) {
            const int j = sorted[k];
            const double* q = xd + 3 * (size_t)j;
            const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
            const double d = ((dx * dx) + dy * dy) + dz * dz;
            if (d < bd || (d == bd && j < bj)) { bd = d; bj = j; }
          }
        }
    }
    if (!(bd < mc2)) { bd = INFINITY; bj = -1; }
    const size_t row = base ? (size_t)base[pair] : (size_t)pair * ld;
    nn_d[row + i] = bd;
    nn_j[row + i] = bj;
  }
  if (part) chunk_sums(A, S, T, pair, i, i < S.ns, bd, bj, mc2, red, part + ((size_t)pair * nchunks + blockIdx.x) * ICP_PARTIAL);
}

// grid (chunks of 256 source points, pairs): the rows of a brute-force pass at base[pair] -> (-1, +Inf) unless d2 < mc2
__global__ __launch_bounds__(IC_THREADS) void icp_radius_mask_kernel(IcpClouds A, const long long* __restrict__ base, double* __restrict__ nn_d,
                                                                      int* __restrict__ nn_j, double mc2) {
  const int pair = blockIdx.y;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  const int i = blockIdx.x * IC_THREADS + threadIdx.x;
  if (i >= S.ns) return;
  const size_t e = (size_t)base[pair] + i;
  if (!(nn_d[e] < mc2)) { nn_d[e] = INFINITY; nn_j[e] = -1; }
}

}  // namespace

void launch_icp_grid_build(hipStream_t st, const IcpClouds& A, const IcpGrid& gr, double max_corr) {
  if (A.c <= 0) return;
  const dim3 fill((A.max_dst + IC_THREADS - 1) / IC_THREADS, A.c);
  hipLaunchKernelGGL(icp_grid_box_kernel, dim3(A.c), dim3(IC_THREADS), 0, st, A, gr, max_corr);
  (void)hipMemsetAsync(gr.ends, 0, (size_t)A.c * gr.cells * sizeof(int), st);
  if (A.max_dst > 0) hipLaunchKernelGGL((icp_grid_fill_kernel<false>), fill, dim3(IC_THREADS), 0, st, A, gr);
  hipLaunchKernelGGL(icp_grid_scan_kernel, dim3(A.c), dim3(SCAN_THREADS), 0, st, gr);
  if (A.max_dst > 0) hipLaunchKernelGGL((icp_grid_fill_kernel<true>), fill, dim3(IC_THREADS), 0, st, A, gr);
}

void launch_icp_grid_probe(hipStream_t st, const IcpClouds& A, const IcpGrid& gr, const double* T, const int* done, int ld, const long long* base,
                           double* nn_d, int* nn_j, double mc2, double* part, int nchunks) {
  if (A.c <= 0 || A.max_src <= 0) return;
  hipLaunchKernelGGL(icp_grid_probe_kernel, dim3((A.max_src + IC_THREADS - 1) / IC_THREADS, A.c), dim3(IC_THREADS), 0, st, A, gr, T, done, ld, base,
                     nn_d, nn_j, mc2, part, nchunks);
}

void launch_icp_radius_mask(hipStream_t st, const IcpClouds& A, const long long* base, double* nn_d, int* nn_j, double mc2) {
  if (A.c <= 0 || A.max_src <= 0) return;
  hipLaunchKernelGGL(icp_radius_mask_kernel, dim3((A.max_src + IC_THREADS - 1) / IC_THREADS, A.c), dim3(IC_THREADS), 0, st, A, base, nn_d, nn_j, mc2);
}

}  // namespace pr
