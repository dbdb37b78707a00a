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
// chunk's inliers (d2 < max_corr^2) to 17 fp64 sums - n, sum d2, sum p', sum q, sum p' q^T, with p' and q taken about the chunk's pivot
// (icp_common.hpp) - by a fixed shuffle tree and writes them to scratch: no floating-point atomics.  icp_finish_kernel (one wave per
// pair) adds the chunks in order about one pivot, forms H, solves the 3 x 3 problem (one-sided Jacobi on H itself: the singular
// triples at H's own conditioning; the third pair by cross products, which is Kabsch's det correction), applies the stop rules and
// updates T, the statistics and the pair's `done` word.  A finished pair's later launches return at once.
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
  unsigned first = 0xFFFFFFFFu;                    // the lane's first inlier: its index in the chunk and (fj) its target row
  int fj = -1;
#pragma unroll
  for (int r = R - 1; r >= 0; r--) {
    const int i = i0 + r * IC_THREADS + threadIdx.x;
    if (i >= S.ns) continue;
    nn_d[row + i] = bd[r];
    nn_j[row + i] = bj[r];
    if (bd[r] < mc2) { first = r * IC_THREADS + threadIdx.x; fj = bj[r]; }
  }
  if (!part) return;
  double a[ICP_SUMS], c[3];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; k++) a[k] = 0.0;
  chunk_pivot(first, fj, xd, red, c);
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int i = i0 + r * IC_THREADS + threadIdx.x;
    if (i < S.ns && bd[r] < mc2) add_inlier(a, p[r], xd + 3 * (size_t)bj[r], bd[r], c);
  }
  reduce_partial(a, c, red, part + ((size_t)pair * nchunks + blockIdx.x) * ICP_PARTIAL);
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

// exchange singular pairs j and k (column j / k of W = G V and of V, squared norm m) when k's is the larger
__device__ __forceinline__ void lead_first(double (&W)[3][3], double (&V)[3][3], double (&m)[3], int j, int k) {
  if (!(m[k] > m[j])) return;
  for (int a = 0; a < 3; a++) {
    const double w = W[a][j], v = V[a][j];
    W[a][j] = W[a][k]; V[a][j] = V[a][k];
    W[a][k] = w; V[a][k] = v;
  }
  const double t = m[j];
  m[j] = m[k]; m[k] = t;
}

// Kabsch: the rotation dR that maximises trace(dR H), H = sum (p - mu_p)(q - mu_q)^T.  With H = U S V^T: dR = V diag(1, 1, det(V U^T)) U^T.
// The singular triples come from ONE-SIDED Jacobi on G = H / max |H|: plane rotations of V's columns until the columns of W = G V are
// orthogonal; then W = U S.  H^T H is never formed (its eigenvectors carry eps (s1 / s2)^2, H's own singular vectors eps s1 / s2).  Every
// sweep takes its angles from a W formed afresh as G V, and so is the W the results are read from: w_k is one 3-term product sum off G,
// in error by a few eps s1 whatever the number of rotations.  A pair of columns whose inner product is below rounding is left alone
// (an exactly symmetric H or a multiple of a rotation ends at once); a sweep whose largest tangent is below 2^-50 is the last, and 12
// sweeps bound the equal-singular-value cases, where rounding alone picks the angles and any of them is right.
// u_k = w_k / |w_k| for the two leading pairs, and u_3 = u_1 x u_2, v_3 = v_1 x v_2: both triples right-handed, which is the det
// correction.  s1 >= s2: the two leading singular values (|w_k| max |H|).  noinline: one copy, off the callers' registers.
__device__ __attribute__((noinline)) void kabsch(const double (&H)[3][3], double (&dR)[3][3], double& s1, double& s2) {
  double hmax = 0.0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) hmax = fmax(hmax, fabs(H[a][b]));
  s1 = s2 = 0.0;
  if (!(hmax > 0.0) || !(hmax < INFINITY)) return;
  double G[3][3], V[3][3], W[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) { G[a][b] = H[a][b] / hmax; V[a][b] = a == b ? 1.0 : 0.0; }
  bool rotate = true;
  for (int sweep = 0;; sweep++) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int k = 0; k < 3; k++) W[a][k] = (G[a][0] * V[0][k] + G[a][1] * V[1][k]) + G[a][2] * V[2][k];
    if (!rotate || sweep == 12) break;
    double big = 0.0;
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int q = p + 1; q < 3; q++) {
        const double al = (W[0][p] * W[0][p] + W[1][p] * W[1][p]) + W[2][p] * W[2][p];
        const double be = (W[0][q] * W[0][q] + W[1][q] * W[1][q]) + W[2][q] * W[2][q];
        const double ga = (W[0][p] * W[0][q] + W[1][p] * W[1][q]) + W[2][p] * W[2][q];
        if (!(ga * ga > 1e-31 * (al * be))) continue;            // |cos| of the two columns <= 3.2e-16: orthogonal to rounding (or a zero column)
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const double x = W[a][p], y = W[a][q], vx = V[a][p], vy = V[a][q];
          W[a][p] = cs * x - sn * y; W[a][q] = sn * x + cs * y;
          V[a][p] = cs * vx - sn * vy; V[a][q] = sn * vx + cs * vy;
        }
        big = fmax(big, fabs(t));
      }
    rotate = big > 0x1p-50;                                      // if not: one more product G V and no more rotations
  }
  double m[3];
#pragma unroll
  for (int k = 0; k < 3; k++) m[k] = (W[0][k] * W[0][k] + W[1][k] * W[1][k]) + W[2][k] * W[2][k];
  lead_first(W, V, m, 0, 1); lead_first(W, V, m, 1, 2); lead_first(W, V, m, 0, 1);
  double v[3][3], u[3][3];
  for (int k = 0; k < 2; k++)
    for (int a = 0; a < 3; a++) { v[k][a] = V[a][k]; u[k][a] = W[a][k]; }
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
  __shared__ double sum[ICP_SUMS];
  __shared__ double piv[3];
  const int pair = blockIdx.x;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  if (!final_pass && done[pair]) return;
  const int used = min(nchunks, (S.ns + chunk_pts - 1) / chunk_pts);
  const double* __restrict__ pp = part + (size_t)pair * nchunks * ICP_PARTIAL;
  if (threadIdx.x < 3) {                          // the common pivot: that of the first chunk with an inlier
    int k0 = 0;
    while (k0 < used && !(pp[(size_t)k0 * ICP_PARTIAL] > 0.0)) k0++;
    piv[threadIdx.x] = k0 < used ? pp[(size_t)k0 * ICP_PARTIAL + ICP_SUMS + threadIdx.x] : 0.0;
  }
  __syncthreads();
  __shared__ double third[3][ICP_SUMS];
  if (threadIdx.x < 3 * ICP_SUMS) {
    // lane (g, t) adds sum t of the g-th third of the chunks in chunk order, each moved from its own pivot c_k to the common one by
    // d = c_k - piv:  sum (x - piv) = sum (x - c_k) + n_k d;  sum (p - piv)(q - piv)^T = sum (p - c_k)(q - c_k)^T + S_p d^T + d S_q^T + n_k d d^T
    const int g = threadIdx.x / ICP_SUMS, t = threadIdx.x % ICP_SUMS, per = (used + 2) / 3;
    const int a = t >= 8 ? (t - 8) / 3 : (t >= 5 ? t - 5 : (t >= 2 ? t - 2 : 0)), b = t >= 8 ? (t - 8) % 3 : 0;
    const int kend = min(used, (g + 1) * per);
    double v = 0.0;
#pragma unroll 8
    for (int k = g * per; k < kend; k++) {         // no branch on the chunk: a chunk without inliers holds zeros (pivot included) and adds +-0
      const double* __restrict__ ck = pp + (size_t)k * ICP_PARTIAL;
      const double nk = ck[0];
      double x = ck[t];
      if (t >= 2) {
        const double da = ck[ICP_SUMS + a] - piv[a];
        if (t < 8) x += nk * da;
        else {
          const double db = ck[ICP_SUMS + b] - piv[b];
          x += (ck[2 + a] * db + da * ck[5 + b]) + nk * (da * db);
        }
      }
      v += x;
    }
    third[g][t] = v;
  }
  __syncthreads();
  if (threadIdx.x < ICP_SUMS) sum[threadIdx.x] = (third[0][threadIdx.x] + third[1][threadIdx.x]) + third[2][threadIdx.x];
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
  double Tn[12], e[3];
  const double c[3] = {piv[0], piv[1], piv[2]};
  for (int b = 0; b < 3; b++) e[b] = (Tp[4 * b + 3] - c[b]) - sum[2 + b] / n;      // t - mu_p: the sums are about the pivot c
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) Tn[4 * a + b] = (dR[a][0] * Tp[b] + dR[a][1] * Tp[4 + b]) + dR[a][2] * Tp[8 + b];
    Tn[4 * a + 3] = ((dR[a][0] * e[0] + dR[a][1] * e[1]) + dR[a][2] * e[2]) + (c[a] + sum[5 + a] / n);      // dR (t - mu_p) + mu_q
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
