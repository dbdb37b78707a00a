// icp.hip — point-to-point ICP refinement of matched cloud pairs on the device (no reference counterpart; the normative arithmetic is
// tests/icp_np.py).  Compiled with -ffp-contract=off: every product and every sum below is rounded on its own.
//
// Correspondence: a brute-force nearest neighbour in fp64 with the FIRST-minimum rule of run_test.m:5-16 (eval.hip follows the same one).
// A workgroup of 256 lanes owns 256 R source points of one pair (R = 1 | 4 per lane), transformed once by the pair's [R | t] and kept in
// registers, and a range of whole tiles of the target cloud (grid.z splits the target when few pairs would leave CUs idle), staged through
// LDS ICP_TILE rows at a time; every lane reads the same row (a broadcast read) and walks j upwards with the strict update `best > d2`
// from (+Inf, -1): a NaN or +Inf distance never wins.  Per-split partials are combined by "smaller d2, then smaller j": the first-minimum
// rule under any partition, so indices and d2 bits do not depend on the launch geometry.
//
// Update: the launch that knows a chunk's final correspondences (the scan itself without a split, the combine with one) reduces the
// chunk's inliers (d2 < max_corr^2) to 17 fp64 sums - n, sum d2, sum p', sum q, sum p' q^T - by a fixed shuffle tree and writes them to
// scratch: no floating-point atomics.  icp_finish_kernel (one wave per pair) adds the chunks in order, forms H, solves the 3 x 3 problem
// (Jacobi on H^T H, frames.hpp; left vectors as H v / |H v|, the third pair by cross products, which is Kabsch's det correction),
// applies the stop rules and updates T, the statistics and the pair's `done` word.  A finished pair's later launches return at once.
#include "frames.hpp"
#include "icp_common.hpp"
#include "kernels.hpp"

namespace pr {
namespace {

using namespace icp_dev;

// grid (source chunks of 256 R points, pairs, target splits).  nsplit = 1: nn_d / nn_j are the results (row base of a pair: base[pair]
// or pair * ld) and part (or null) receives the chunk's sums; nsplit > 1: nn_d / nn_j are the slots [split][pair][ld]
template <int R>
__global__ __launch_bounds__(IC_THREADS) void icp_nn_kernel(IcpClouds A, const double* __restrict__ T, const int* __restrict__ done, int nsplit,
                                                             int ld, const long long* __restrict__ base, double* __restrict__ nn_d,
                                                             int* __restrict__ nn_j, double mc2, double* __restrict__ part, int nchunks) {
  __shared__ double tile[ICP_TILE * 3];
  __shared__ double red[IC_THREADS / 64][ICP_PARTIAL];
  const int pair = blockIdx.y;
  if (done && done[pair]) return;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  const int i0 = blockIdx.x * (IC_THREADS * R);
  if (i0 >= S.ns) return;
  const double* __restrict__ Tp = T + 12 * (size_t)pair;
  double p[R][3], bd[R];
  int bj[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int i = i0 + r * IC_THREADS + threadIdx.x;
    const double* s = A.xyz_q + 3 * (size_t)(S.q0 + (i < S.ns ? i : 0));
    transform(Tp, s[0], s[1], s[2], p[r]);
    bd[r] = INFINITY; bj[r] = -1;
  }
  const int tiles = (S.nd + ICP_TILE - 1) / ICP_TILE, per = (tiles + nsplit - 1) / nsplit;
  const long long jb = (long long)blockIdx.z * per * ICP_TILE;
  const int jbeg = (int)(jb < S.nd ? jb : S.nd), jend = (int)(jb + (long long)per * ICP_TILE < S.nd ? jb + (long long)per * ICP_TILE : S.nd);
  const double* __restrict__ xd = A.xyz_d + 3 * (size_t)S.d0;
  for (int j0 = jbeg; j0 < jend; j0 += ICP_TILE) {
    const int jn = min(ICP_TILE, jend - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < jn * 3; e += IC_THREADS) tile[e] = xd[(size_t)j0 * 3 + e];
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < jn; jj++) {
      const double gx = tile[jj * 3], gy = tile[jj * 3 + 1], gz = tile[jj * 3 + 2];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const double dx = p[r][0] - gx, dy = p[r][1] - gy, dz = p[r][2] - gz;
        const double d = ((dx * dx) + dy * dy) + dz * dz;
        if (bd[r] > d) { bd[r] = d; bj[r] = j0 + jj; }
      }
    }
  }
  const size_t row = nsplit > 1 ? ((size_t)blockIdx.z * A.c + pair) * (size_t)ld : (base ? (size_t)base[pair] : (size_t)pair * ld);
  double a[ICP_PARTIAL];
#pragma unroll
  for (int k = 0; k < ICP_PARTIAL; k++) a[k] = 0.0;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int i = i0 + r * IC_THREADS + threadIdx.x;
    if (i >= S.ns) continue;
    nn_d[row + i] = bd[r];
    nn_j[row + i] = bj[r];
    if (part && bd[r] < mc2) add_inlier(a, p[r], xd + 3 * (size_t)bj[r], bd[r]);
  }
  if (part) reduce_partial(a, red, part + ((size_t)pair * nchunks + blockIdx.x) * ICP_PARTIAL);
}

// grid (chunks of 256 points, pairs): the nsplit slots of a point -> its result (smaller d2, then smaller j; (+Inf, -1) = no candidate),
// and with part the chunk's sums (the point is transformed again: the same operations, the same bits)
__global__ __launch_bounds__(IC_THREADS) void icp_combine_kernel(IcpClouds A, const double* __restrict__ T, const int* __restrict__ done, int nsplit,
                                                                  int ld, const double* __restrict__ slot_d, const int* __restrict__ slot_j,
                                                                  const long long* __restrict__ base, double* __restrict__ nn_d,
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
    for (int s = 0; s < nsplit; s++) {
      const size_t e = ((size_t)s * A.c + pair) * (size_t)ld + i;
      const double d = slot_d[e];
      const int j = slot_j[e];
      if (j >= 0 && (d < bd || (d == bd && j < bj))) { bd = d; bj = j; }
    }
    const size_t row = base ? (size_t)base[pair] : (size_t)pair * ld;
    nn_d[row + i] = bd;
    nn_j[row + i] = bj;
  }
  if (part) chunk_sums(A, S, T, pair, i, i < S.ns, bd, bj, mc2, red, part + ((size_t)pair * nchunks + blockIdx.x) * ICP_PARTIAL);
}

// out_offs[0 .. c]: prefix of the pairs' (clamped) source sizes, 0 for a pair of -1.  One workgroup.
__global__ __launch_bounds__(IC_THREADS) void icp_offsets_kernel(IcpClouds A, long long* __restrict__ out_offs) {
  __shared__ long long sc[IC_THREADS];
  __shared__ long long carry;
  if (threadIdx.x == 0) { carry = 0; out_offs[0] = 0; }
  __syncthreads();
  for (int b0 = 0; b0 < A.c; b0 += IC_THREADS) {
    const int pair = b0 + threadIdx.x;
    PairShape S;
    long long v = (pair < A.c && pair_shape(A, pair, S)) ? S.ns : 0;
    sc[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < IC_THREADS; o <<= 1) {
      const long long t = threadIdx.x >= o ? sc[threadIdx.x - o] : 0;
      __syncthreads();
      sc[threadIdx.x] += t;
      __syncthreads();
    }
    if (pair < A.c) out_offs[pair + 1] = carry + sc[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) carry += sc[IC_THREADS - 1];
    __syncthreads();
  }
}

// T = T0, statistics cleared, done = 1 / status no_pair for a pair of -1
__global__ void icp_init_kernel(IcpClouds A, const double* __restrict__ T0, double* __restrict__ T, IcpStats* __restrict__ stats,
                                int* __restrict__ done, double* __restrict__ prev) {
  const int pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= A.c) return;
  for (int k = 0; k < 12; k++) T[12 * (size_t)pair + k] = T0[12 * (size_t)pair + k];
  PairShape S;
  const bool has = pair_shape(A, pair, S);
  IcpStats s;
  s.fitness = 0.0; s.rmse = 0.0; s.n_inl = 0; s.iters = 0; s.status = has ? ICP_RUNNING : ICP_NO_PAIR; s.pad = 0;
  stats[pair] = s;
  done[pair] = has ? 0 : 1;
  prev[2 * (size_t)pair] = 0.0; prev[2 * (size_t)pair + 1] = 0.0;
}

__device__ __forceinline__ double norm3(const double (&v)[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// Kabsch: the rotation dR that maximises trace(dR H), H = sum (p - mu_p)(q - mu_q)^T.  With H = U S V^T: dR = V diag(1, 1, det(V U^T)) U^T.
// V from the Jacobi eigenvectors of H^T H (two leading ones), u_k = H v_k / |H v_k|, and u_3 = u_1 x u_2, v_3 = v_1 x v_2: both triples
// right-handed, which is the det correction.  s1 >= s2: the two leading singular values.  noinline: one copy, off the callers' registers.
__device__ __attribute__((noinline)) void kabsch(const double (&H)[3][3], double (&dR)[3][3], double& s1, double& s2) {
  double hmax = 0.0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) hmax = fmax(hmax, fabs(H[a][b]));
  s1 = s2 = 0.0;
  if (!(hmax > 0.0) || !(hmax < INFINITY)) return;
  double G[3][3], A[3][3], V[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) G[a][b] = H[a][b] / hmax;
  for (int a = 0; a < 3; a++)
    for (int b = a; b < 3; b++) A[a][b] = A[b][a] = (G[0][a] * G[0][b] + G[1][a] * G[1][b]) + G[2][a] * G[2][b];
  jacobi_eig3(A, V);
  int o[3] = {0, 1, 2};
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2 - i; j++)
      if (A[o[j + 1]][o[j + 1]] > A[o[j]][o[j]]) { const int t = o[j]; o[j] = o[j + 1]; o[j + 1] = t; }
  double v[3][3], u[3][3];
  for (int k = 0; k < 2; k++)
    for (int a = 0; a < 3; a++) v[k][a] = V[a][o[k]];
  for (int k = 0; k < 2; k++)
    for (int a = 0; a < 3; a++) u[k][a] = (G[a][0] * v[k][0] + G[a][1] * v[k][1]) + G[a][2] * v[k][2];
  const double n1 = norm3(u[0]), n2 = norm3(u[1]);
  s1 = n1 * hmax; s2 = n2 * hmax;
  if (!(n2 > 1e-12 * n1)) return;
  for (int a = 0; a < 3; a++) u[0][a] /= n1;
  const double dot = (u[1][0] * u[0][0] + u[1][1] * u[0][1]) + u[1][2] * u[0][2];
  for (int a = 0; a < 3; a++) u[1][a] -= dot * u[0][a];
  const double m2 = norm3(u[1]);
  for (int a = 0; a < 3; a++) u[1][a] /= m2;
  cross3(u[0], u[1], u[2]);
  cross3(v[0], v[1], v[2]);
  const double m3 = norm3(v[2]);
  for (int a = 0; a < 3; a++) v[2][a] /= m3;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) dR[a][b] = (v[0][a] * u[0][b] + v[1][a] * u[1][b]) + v[2][a] * u[2][b];
}

// one wave per pair: the chunks' sums in chunk order, then lane 0: statistics, stop rules, update (final: the reported statistics only)
__global__ __launch_bounds__(64) void icp_finish_kernel(IcpClouds A, const double* __restrict__ part, int nchunks, int chunk_pts, IcpParams P,
                                                         int final_pass, double* __restrict__ T, IcpStats* __restrict__ stats,
                                                         int* __restrict__ done, double* __restrict__ prev) {
  __shared__ double sum[ICP_PARTIAL];
  const int pair = blockIdx.x;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  if (!final_pass && done[pair]) return;
  const int used = min(nchunks, (S.ns + chunk_pts - 1) / chunk_pts);
  if (threadIdx.x < ICP_PARTIAL) {
    double v = 0.0;
    for (int k = 0; k < used; k++) v += part[((size_t)pair * nchunks + k) * ICP_PARTIAL + threadIdx.x];
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
  if (n < (double)P.min_inliers) { st.status = ICP_TOO_FEW; done[pair] = 1; return; }
  double H[3][3], dR[3][3], s1, s2;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) H[a][b] = sum[8 + 3 * a + b] - sum[2 + a] * sum[5 + b] / n;
  kabsch(H, dR, s1, s2);
  if (!(s2 > 1e-12 * s1)) { st.status = ICP_DEGENERATE; done[pair] = 1; return; }
  double* Tp = T + 12 * (size_t)pair;
  double Tn[12];
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) Tn[4 * a + b] = (dR[a][0] * Tp[b] + dR[a][1] * Tp[4 + b]) + dR[a][2] * Tp[8 + b];
    const double rt = (dR[a][0] * Tp[3] + dR[a][1] * Tp[7]) + dR[a][2] * Tp[11];
    const double rm = (dR[a][0] * sum[2] + dR[a][1] * sum[3]) + dR[a][2] * sum[4];
    Tn[4 * a + 3] = rt + (sum[5 + a] / n - rm / n);
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

void launch_icp_offsets(hipStream_t st, const IcpClouds& A, long long* out_offs) {
  hipLaunchKernelGGL(icp_offsets_kernel, dim3(1), dim3(IC_THREADS), 0, st, A, out_offs);
}

void launch_icp_init(hipStream_t st, const IcpClouds& A, const double* T0, double* T, IcpStats* stats, int* done, double* prev) {
  if (A.c > 0) hipLaunchKernelGGL(icp_init_kernel, dim3((A.c + 63) / 64), dim3(64), 0, st, A, T0, T, stats, done, prev);
}

void launch_icp_nn(hipStream_t st, const IcpClouds& A, const IcpGeometry& g, const double* T, const int* done, double* slot_d, int* slot_j,
                   const long long* base, double* nn_d, int* nn_j, double mc2, double* part) {
  if (A.c <= 0 || A.max_src <= 0) return;
  const int per = IC_THREADS * g.rq;
  const dim3 grid((A.max_src + per - 1) / per, A.c, g.nsplit);
  double* od = g.nsplit > 1 ? slot_d : nn_d;
  int* oj = g.nsplit > 1 ? slot_j : nn_j;
  double* kp = g.nsplit > 1 ? nullptr : part;      // with a split the combining launch knows the correspondences
  if (g.rq == 4) hipLaunchKernelGGL((icp_nn_kernel<4>), grid, dim3(IC_THREADS), 0, st, A, T, done, g.nsplit, g.ld, base, od, oj, mc2, kp, g.nchunks);
  else hipLaunchKernelGGL((icp_nn_kernel<1>), grid, dim3(IC_THREADS), 0, st, A, T, done, g.nsplit, g.ld, base, od, oj, mc2, kp, g.nchunks);
  if (g.nsplit > 1)
    hipLaunchKernelGGL(icp_combine_kernel, dim3((A.max_src + IC_THREADS - 1) / IC_THREADS, A.c), dim3(IC_THREADS), 0, st, A, T, done, g.nsplit, g.ld,
                       slot_d, slot_j, base, nn_d, nn_j, mc2, part, g.nchunks);
}

void launch_icp_finish(hipStream_t st, const IcpClouds& A, const IcpGeometry& g, const double* part, const IcpParams& P, int final_pass, double* T,
                       IcpStats* stats, int* done, double* prev) {
  if (A.c > 0) hipLaunchKernelGGL(icp_finish_kernel, dim3(A.c), dim3(64), 0, st, A, part, g.nchunks, g.chunk_pts, P, final_pass, T, stats, done, prev);
}

}  // namespace pr
