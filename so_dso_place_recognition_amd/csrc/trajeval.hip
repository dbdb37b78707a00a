// trajeval.hip — trajectory evaluation against ground truth on the device (no reference counterpart): ATE under an
// alignment, RPE per delta, KITTI's segment metric over keyframe rows and the error of logged closures, for B candidate pose arrays a call.
// The rule is in include/place_recognition.h and restated in tests/trajeval_np.py; apart from atan2 the device equals it bit for bit
// (fp64, no contraction, + x / sqrt only).  Every grid depends on the create sizes only and every count is read from device memory, so
// one captured run serves every count.
//   prepare   a lane per (row, b): used flags and camera centres; the last grid row does the ground truth
//   ate       one workgroup per b: the means, the centred covariance, the alignment S (lane 0: Jacobi SVD), the ATE statistics and
//             errors, then both path-length prefixes in 256 blocks
//   rpe       one workgroup per (delta, b)
//   seg       one workgroup per (length, b): a binary search of the prefix per start row; then a lane per b adds the lengths' sums
//   closures  one workgroup: every logged edge against the ground truth
// Every floating-point sum goes through ONE tree: lane t adds its terms i = t, t + 256, ... in that order (a term that does not count adds
// +0.0), then the 256 lane sums are folded by halving (lane t += lane t + s for s = 128, 64, .. 1).  No floating-point atomics, no
// workgroup waits for another, every loop is bounded by a create size.  Plain C++, vector stores only.
#include "trajeval.hpp"

namespace pr {
namespace {

using namespace traj;

constexpr int T = TRAJ_T;
constexpr int IMAX = 0x7fffffff;

template <int M>
__device__ __forceinline__ void tree_sum(double (&x)[M], double* lds, int tid) {
#pragma unroll
  for (int m = 0; m < M; m++) lds[m * T + tid] = x[m];
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int m = 0; m < M; m++) lds[m * T + tid] = lds[m * T + tid] + lds[m * T + tid + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < M; m++) x[m] = lds[m * T];
  __syncthreads();
}
template <int M>
__device__ __forceinline__ void tree_max(double (&x)[M], double* lds, int tid) {
#pragma unroll
  for (int m = 0; m < M; m++) lds[m * T + tid] = x[m];
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int m = 0; m < M; m++) lds[m * T + tid] = fmax(lds[m * T + tid], lds[m * T + tid + s]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < M; m++) x[m] = lds[m * T];
  __syncthreads();
}
__device__ __forceinline__ int tree_isum(int x, int* lds, int tid) {
  lds[tid] = x;
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s) lds[tid] += lds[tid + s];
    __syncthreads();
  }
  const int r = lds[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ int tree_imin(int x, int* lds, int tid) {
  lds[tid] = x;
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s) lds[tid] = lds[tid + s] < lds[tid] ? lds[tid + s] : lds[tid];
    __syncthreads();
  }
  const int r = lds[0];
  __syncthreads();
  return r;
}

// the relative motion between rows i and j of the ground truth in world-to-camera terms: G_i G_j^-1 (W2C rows), G_i^-1 G_j (C2W rows)
__device__ __forceinline__ void gt_rel(const TrajView& v, const double* gt, int i, int j, double* R, double* t) {
  double Ri[9], ti[3], Rj[9], tj[3], Rv[9], tv[3];
  load_pose(gt + (size_t)i * 12, Ri, ti);
  load_pose(gt + (size_t)j * 12, Rj, tj);
  if (v.gt_kind == TRAJ_GT_W2C) { rigid_inv(Rj, tj, Rv, tv); rigid_mul(Ri, ti, Rv, tv, R, t); }
  else { rigid_inv(Ri, ti, Rv, tv); rigid_mul(Rv, tv, Rj, tj, R, t); }
}

// E = A^-1 Q, and of E: c_rot = 3 - tr R_E, theta = atan2(|vee(R_E - R_E^T) / 2|, (tr R_E - 1) / 2), d = |t_E|
__device__ __forceinline__ void rel_error(const double* RA, const double* tA, const double* RQ, const double* tQ, double& c_rot, double& theta,
                                          double& d) {
  double Rv[9], tv[3], RE[9], tE[3];
  rigid_inv(RA, tA, Rv, tv);
  rigid_mul(Rv, tv, RQ, tQ, RE, tE);
  const double tr = (RE[0] + RE[4]) + RE[8];
  c_rot = 3.0 - tr;
  const double v0 = 0.5 * (RE[7] - RE[5]), v1 = 0.5 * (RE[2] - RE[6]), v2 = 0.5 * (RE[3] - RE[1]);
  theta = atan2(norm3(v0, v1, v2), 0.5 * (tr - 1.0));
  d = norm3(tE[0], tE[1], tE[2]);
}

// the error of candidate b's motion between its rows i and j (both used) against the ground truth's
__device__ __forceinline__ void pair_error(const TrajView& v, const TrajIn& in, int b, int i, int j, double s, double& c_rot, double& theta,
                                           double& d) {
  const double* est = in.est + (size_t)b * v.cap * 12;
  double Ri[9], ti[3], Rj[9], tj[3], Rv[9], tv[3], RQ[9], tQ[3], RG[9], tG[3];
  load_pose(est + (size_t)i * 12, Ri, ti);
  load_pose(est + (size_t)j * 12, Rj, tj);
  rigid_inv(Rj, tj, Rv, tv);
  rigid_mul(Ri, ti, Rv, tv, RQ, tQ);                             // P_i P_j^-1
  tQ[0] = s * tQ[0]; tQ[1] = s * tQ[1]; tQ[2] = s * tQ[2];       // s = 1 unless the mode is SIM3
  gt_rel(v, in.gt, i, j, RG, tG);
  rel_error(RG, tG, RQ, tQ, c_rot, theta, d);
}

// ------------------------------------------------------------------------------------------------ prepare
__global__ __launch_bounds__(T) void traj_prepare_kernel(TrajView v, TrajIn in, TrajOut out) {
  const int i = blockIdx.x * T + threadIdx.x, b = blockIdx.y, cap = v.cap;
  if (i >= cap) return;
  const int n = clampi(in.n[0], cap);                            // a scribbled count never forms an address
  const int gw = v.gt_kind == TRAJ_GT_POSITIONS ? 3 : 12;
  bool g = i < n && (in.valid == nullptr || in.valid[i] != 0);
  const double* gr = in.gt + (size_t)i * gw;
  if (g)
    for (int c = 0; c < gw; c++) g = g && fin(gr[c]);
  double c3[3] = {0.0, 0.0, 0.0};
  if (b == v.B) {                                                // the ground truth
    if (g) {
      if (v.gt_kind == TRAJ_GT_POSITIONS) { c3[0] = gr[0]; c3[1] = gr[1]; c3[2] = gr[2]; }
      else if (v.gt_kind == TRAJ_GT_C2W) { c3[0] = gr[3]; c3[1] = gr[7]; c3[2] = gr[11]; }
      else {
        double R[9], t[3], y[3];
        load_pose(gr, R, t);
        mtv3(R, t, y);
        c3[0] = -y[0]; c3[1] = -y[1]; c3[2] = -y[2];
      }
    }
    v.gtok[i] = g ? 1 : 0;
  } else {
    const double* er = in.est + ((size_t)b * cap + i) * 12;
    bool u = g;
    if (u)
      for (int c = 0; c < 12; c++) u = u && fin(er[c]);
    if (u) {
      double R[9], t[3], y[3];
      load_pose(er, R, t);
      mtv3(R, t, y);
      c3[0] = -y[0]; c3[1] = -y[1]; c3[2] = -y[2];
    }
    v.used[(size_t)b * cap + i] = u ? 1 : 0;
  }
  const size_t o = ((size_t)b * cap + i) * 3;
  v.cen[o] = c3[0]; v.cen[o + 1] = c3[1]; v.cen[o + 2] = c3[2];
  if (out.centres) { out.centres[o] = c3[0]; out.centres[o + 1] = c3[1]; out.centres[o + 2] = c3[2]; }
}

// ------------------------------------------------------------------------------------------------ the rotation of Umeyama's alignment
// A = U Sigma V^T by one-sided Jacobi on G = A / max |A|: TRAJ_SWEEPS sweeps over the column pairs (0, 1), (0, 2), (1, 2) of W = G V, W formed
// afresh in front of every sweep and once more at the end; the columns ordered by falling norm; u_1 = w_1 / |w_1|, u_2 = w_2 less its part
// along u_1, normalised, u_3 = u_1 x u_2, v_3' = v_1 x v_2 normalised: both triples right-handed, so R = sum u_k v_k'^T is U D V^T.
// dsign = the sign of det U det V = of (u_3 . w_3)(v_3' . v_3).  deg: |w_2| is not above 1e-12 |w_1|; then u_2 is the unit vector of the
// coordinate axis on which u_1 is smallest (the lowest on a tie), less its part along u_1, normalised, and dsign = 1.
__device__ __attribute__((noinline)) void umeyama_rot(const double* A, double* R, double* sig, int& deg, double& dsign) {
  double hmax = 0.0;
  for (int c = 0; c < 9; c++) hmax = fmax(hmax, fabs(A[c]));
  for (int c = 0; c < 9; c++) R[c] = (c % 4 == 0) ? 1.0 : 0.0;
  sig[0] = sig[1] = sig[2] = 0.0;
  deg = 1; dsign = 1.0;
  if (!(hmax > 0.0) || !fin(hmax)) return;
  double G[3][3], V[3][3], W[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) { G[a][b] = A[3 * a + b] / hmax; V[a][b] = a == b ? 1.0 : 0.0; }
  for (int sweep = 0;; sweep++) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int k = 0; k < 3; k++) W[a][k] = (G[a][0] * V[0][k] + G[a][1] * V[1][k]) + G[a][2] * V[2][k];
    if (sweep == TRAJ_SWEEPS) break;
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int q = p + 1; q < 3; q++) {
        const double al = (W[0][p] * W[0][p] + W[1][p] * W[1][p]) + W[2][p] * W[2][p];
        const double be = (W[0][q] * W[0][q] + W[1][q] * W[1][q]) + W[2][q] * W[2][q];
        const double ga = (W[0][p] * W[0][q] + W[1][p] * W[1][q]) + W[2][p] * W[2][q];
        if (!(ga * ga > 1e-31 * (al * be))) continue;            // orthogonal to rounding, or a zero column
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const double x = W[a][p], y = W[a][q], vx = V[a][p], vy = V[a][q];
          W[a][p] = cs * x - sn * y; W[a][q] = sn * x + cs * y;
          V[a][p] = cs * vx - sn * vy; V[a][q] = sn * vx + cs * vy;
        }
      }
  }
  double w[3][3], vv[3][3], m[3];                                // columns as rows
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int a = 0; a < 3; a++) { w[k][a] = W[a][k]; vv[k][a] = V[a][k]; }
    m[k] = (w[k][0] * w[k][0] + w[k][1] * w[k][1]) + w[k][2] * w[k][2];
  }
  auto lead = [&](int j, int k) {
    if (!(m[j] < m[k])) return;
    for (int a = 0; a < 3; a++) {
      const double x = w[j][a], y = vv[j][a];
      w[j][a] = w[k][a]; vv[j][a] = vv[k][a];
      w[k][a] = x; vv[k][a] = y;
    }
    const double x = m[j];
    m[j] = m[k]; m[k] = x;
  };
  lead(0, 1); lead(1, 2); lead(0, 1);
  const double n1 = sqrt(m[0]), n2 = sqrt(m[1]), n3 = sqrt(m[2]);
  sig[0] = n1 * hmax; sig[1] = n2 * hmax; sig[2] = n3 * hmax;
  deg = (n2 > 1e-12 * n1) ? 0 : 1;
  double u[3][3];
  for (int a = 0; a < 3; a++) u[0][a] = w[0][a] / n1;
  if (!deg) {
    for (int a = 0; a < 3; a++) u[1][a] = w[1][a];
  } else {
    int k = 0;
    if (fabs(u[0][1]) < fabs(u[0][k])) k = 1;
    if (fabs(u[0][2]) < fabs(u[0][k])) k = 2;
    for (int a = 0; a < 3; a++) u[1][a] = a == k ? 1.0 : 0.0;
  }
  const double dot = (u[1][0] * u[0][0] + u[1][1] * u[0][1]) + u[1][2] * u[0][2];
  for (int a = 0; a < 3; a++) u[1][a] = u[1][a] - dot * u[0][a];
  const double m2 = norm3(u[1][0], u[1][1], u[1][2]);
  for (int a = 0; a < 3; a++) u[1][a] = u[1][a] / m2;
  double v3[3];
  cross3(u[0], u[1], u[2]);
  cross3(vv[0], vv[1], v3);
  const double m3 = norm3(v3[0], v3[1], v3[2]);
  for (int a = 0; a < 3; a++) v3[a] = v3[a] / m3;
  if (!deg) {
    const double pu = (u[2][0] * w[2][0] + u[2][1] * w[2][1]) + u[2][2] * w[2][2];
    const double pv = (v3[0] * vv[2][0] + v3[1] * vv[2][1]) + v3[2] * vv[2][2];
    dsign = pu * pv < 0.0 ? -1.0 : 1.0;
  }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) R[3 * a + b] = (u[0][a] * vv[0][b] + u[1][a] * vv[1][b]) + u[2][a] * v3[b];
}

// ------------------------------------------------------------------------------------------------ alignment, ATE, prefixes
__global__ __launch_bounds__(T) void traj_ate_kernel(TrajView v, TrajIn in, TrajOut out) {
  __shared__ double lds[10 * T];
  __shared__ int ilds[T];
  __shared__ double sS[16];
  const int tid = threadIdx.x, b = blockIdx.x, cap = v.cap;
  const int n = clampi(in.n[0], cap);
  const int* used = v.used + (size_t)b * cap;
  const double* ce = v.cen + (size_t)b * cap * 3;
  const double* cg = v.cen + (size_t)v.B * cap * 3;
  // 1. the count, the first used row, the means
  double a6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int cnt = 0, first = IMAX;
  for (int i = tid; i < n; i += T) {
    const int u = used[i];
    cnt += u;
    if (u && i < first) first = i;
#pragma unroll
    for (int c = 0; c < 3; c++) { a6[c] += u ? ce[(size_t)i * 3 + c] : 0.0; a6[3 + c] += u ? cg[(size_t)i * 3 + c] : 0.0; }
  }
  const int N = tree_isum(cnt, ilds, tid);
  first = tree_imin(first, ilds, tid);
  tree_sum<6>(a6, lds, tid);
  const double Nd = (double)N;
  double mx[3] = {0.0, 0.0, 0.0}, my[3] = {0.0, 0.0, 0.0};
  if (N > 0)
    for (int c = 0; c < 3; c++) { mx[c] = a6[c] / Nd; my[c] = a6[3 + c] / Nd; }
  const bool umeyama = (v.align == TRAJ_ALIGN_SE3 || v.align == TRAJ_ALIGN_SIM3) && N >= 3;
  // 2. the centred covariance (1 / N) sum (y - my)(x - mx)^T and var_x, then S
  double q10[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (umeyama) {
    for (int i = tid; i < n; i += T) {
      const int u = used[i];
      double dx[3], dy[3];
#pragma unroll
      for (int c = 0; c < 3; c++) { dx[c] = ce[(size_t)i * 3 + c] - mx[c]; dy[c] = cg[(size_t)i * 3 + c] - my[c]; }
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) q10[3 * r + c] += u ? dy[r] * dx[c] : 0.0;
      q10[9] += u ? (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2] : 0.0;
    }
    tree_sum<10>(q10, lds, tid);
  }
  if (tid == 0) {
    double s = 1.0, R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, sig[3] = {0.0, 0.0, 0.0}, varx = 0.0;
    int flags = N < 3 ? TRAJ_FEW : 0;
    if (umeyama) {
      double A[9];
      for (int c = 0; c < 9; c++) A[c] = q10[c] / Nd;
      varx = q10[9] / Nd;
      int deg;
      double dsign;
      umeyama_rot(A, R, sig, deg, dsign);
      if (deg) flags |= TRAJ_DEGENERATE;
      if (!(varx > 0.0)) flags |= TRAJ_NO_SCALE;
      else if (v.align == TRAJ_ALIGN_SIM3) s = ((sig[0] + sig[1]) + dsign * sig[2]) / varx;
      double y[3];
      mv3(R, mx, y);
      for (int c = 0; c < 3; c++) t[c] = my[c] - s * y[c];
    } else if (v.align == TRAJ_ALIGN_FIRST && N >= 1) {          // the rigid map of the est world onto the gt world at the first used row
      double Re[9], te[3], Rg[9], tg[3], Rv[9], tv[3];
      load_pose(in.est + ((size_t)b * cap + first) * 12, Re, te);
      load_pose(in.gt + (size_t)first * 12, Rg, tg);
      if (v.gt_kind == TRAJ_GT_W2C) { rigid_inv(Rg, tg, Rv, tv); rigid_mul(Rv, tv, Re, te, R, t); }
      else rigid_mul(Rg, tg, Re, te, R, t);
    }
    sS[0] = s;
    for (int c = 0; c < 9; c++) sS[1 + c] = R[c];
    for (int c = 0; c < 3; c++) sS[10 + c] = t[c];
    sS[13] = sig[0]; sS[14] = sig[1]; sS[15] = sig[2];
    double* So = v.S + (size_t)b * 16;
    for (int c = 0; c < 13; c++) So[c] = sS[c];
    So[13] = 0.0; So[14] = 0.0; So[15] = 0.0;
    double* ao = out.ate + (size_t)b * TRAJ_ATE;
    ao[0] = Nd;
    for (int c = 0; c < 13; c++) ao[6 + c] = sS[c];
    ao[19] = (double)flags; ao[20] = sig[0]; ao[21] = sig[1]; ao[22] = sig[2]; ao[23] = varx;
  }
  __syncthreads();
  // 3. ATE
  const double s = sS[0];
  double R[9], t[3];
  for (int c = 0; c < 9; c++) R[c] = sS[1 + c];
  for (int c = 0; c < 3; c++) t[c] = sS[10 + c];
  double s2[2] = {0.0, 0.0}, best[1] = {0.0};
  int besti = IMAX;
  for (int i = tid; i < cap; i += T) {
    const int u = used[i];                                        // 0 for every row >= n
    double p[3];
    mv3(R, ce + (size_t)i * 3, p);
    const double ex = cg[(size_t)i * 3] - (s * p[0] + t[0]), ey = cg[(size_t)i * 3 + 1] - (s * p[1] + t[1]),
                 ez = cg[(size_t)i * 3 + 2] - (s * p[2] + t[2]);
    const double e2 = (ex * ex + ey * ey) + ez * ez, e = sqrt(e2);
    s2[0] += u ? e2 : 0.0; s2[1] += u ? e : 0.0;
    if (u && (besti == IMAX || e > best[0])) { best[0] = e; besti = i; }
    if (out.err) out.err[(size_t)b * cap + i] = u ? e : -1.0;
  }
  tree_sum<2>(s2, lds, tid);
  const double mine = best[0];
  tree_max<1>(best, lds, tid);
  const int arg = tree_imin(besti != IMAX && mine == best[0] ? besti : IMAX, ilds, tid);
  if (tid == 0) {
    double* ao = out.ate + (size_t)b * TRAJ_ATE;
    ao[1] = s2[0];
    ao[2] = N > 0 ? sqrt(s2[0] / Nd) : 0.0;
    ao[3] = N > 0 ? s2[1] / Nd : 0.0;
    ao[4] = best[0];
    ao[5] = N > 0 ? (double)arg : -1.0;
  }
  // 4. the path-length prefixes in T blocks of C rows: the running sum inside a block, the blocks' totals summed in block order,
  //    prefix = base of the block + running sum
  const int C = (cap + T - 1) / T;
  const int i0 = tid * C < cap ? tid * C : cap, i1 = i0 + C < cap ? i0 + C : cap;
  int last = -1;
  for (int i = i0; i < i1; i++)
    if (used[i]) last = i;
  ilds[tid] = last;
  __syncthreads();
  if (tid == 0) {
    int run = -1;
    for (int k = 0; k < T; k++) { const int x = ilds[k]; ilds[k] = run; if (x >= 0) run = x; }
  }
  __syncthreads();
  int prev = ilds[tid];
  double wg = 0.0, we = 0.0;
  double* pg = v.prefix + (size_t)b * 2 * cap;
  double* pe = pg + cap;
  for (int i = i0; i < i1; i++) {
    if (used[i]) {
      if (prev >= 0) {
        const double* a = cg + (size_t)i * 3;
        const double* c = cg + (size_t)prev * 3;
        wg += norm3(a[0] - c[0], a[1] - c[1], a[2] - c[2]);
        a = ce + (size_t)i * 3; c = ce + (size_t)prev * 3;
        we += norm3(a[0] - c[0], a[1] - c[1], a[2] - c[2]);
      }
      prev = i;
    }
    pg[i] = wg; pe[i] = we;
  }
  lds[tid] = wg; lds[T + tid] = we;
  __syncthreads();
  if (tid == 0) {
    double rg = 0.0, re = 0.0;
    for (int k = 0; k < T; k++) {
      const double x = lds[k], y = lds[T + k];
      lds[k] = rg; lds[T + k] = re;
      rg += x; re += y;
    }
  }
  __syncthreads();
  const double bg = lds[tid], be = lds[T + tid];
  for (int i = i0; i < i1; i++) {
    const double x = bg + pg[i], y = be + pe[i];
    pg[i] = x; pe[i] = y;
    if (out.prefix) { out.prefix[(size_t)b * 2 * cap + i] = x; out.prefix[((size_t)b * 2 + 1) * cap + i] = y; }
  }
}

// ------------------------------------------------------------------------------------------------ RPE
__global__ __launch_bounds__(T) void traj_rpe_kernel(TrajView v, TrajIn in, TrajOut out) {
  __shared__ double lds[6 * T];
  __shared__ int ilds[T];
  const int tid = threadIdx.x, k = blockIdx.x, b = blockIdx.y, cap = v.cap;
  const int n = clampi(in.n[0], cap), delta = v.deltas[k];
  const int* used = v.used + (size_t)b * cap;
  const double s = v.S[(size_t)b * 16];
  double sm[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, mxv[2] = {0.0, 0.0};
  int cnt = 0;
  const int last = n - delta;                                    // delta >= 1, n >= 0: no overflow
  for (int i = tid; i < last; i += T) {
    if (!(used[i] && used[i + delta])) continue;                 // i + delta < n <= cap
    double c_rot, th, d;
    pair_error(v, in, b, i, i + delta, s, c_rot, th, d);
    cnt++;
    sm[0] += d * d; sm[1] += d; sm[2] += th * th; sm[3] += th; sm[4] += c_rot;
    mxv[0] = fmax(mxv[0], d); mxv[1] = fmax(mxv[1], th);
  }
  const int Np = tree_isum(cnt, ilds, tid);
  tree_sum<5>(sm, lds, tid);
  tree_max<2>(mxv, lds, tid);
  if (tid != 0) return;
  double* o = out.rpe + ((size_t)b * v.K + k) * TRAJ_RPE;
  const double Nd = (double)Np;
  o[0] = Nd;
  o[1] = Np > 0 ? sqrt(sm[0] / Nd) : 0.0; o[2] = Np > 0 ? sm[1] / Nd : 0.0; o[3] = mxv[0];
  o[4] = Np > 0 ? sqrt(sm[2] / Nd) : 0.0; o[5] = Np > 0 ? sm[3] / Nd : 0.0; o[6] = mxv[1];
  o[7] = Np > 0 ? sm[4] / Nd : 0.0;
}

// ------------------------------------------------------------------------------------------------ segments
__global__ __launch_bounds__(T) void traj_seg_kernel(TrajView v, TrajIn in, TrajOut out) {
  __shared__ double lds[3 * T];
  __shared__ int ilds[T];
  const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y, cap = v.cap, L = v.L;
  const int n = clampi(in.n[0], cap);
  const int* used = v.used + (size_t)b * cap;
  const double* pg = v.prefix + (size_t)b * 2 * cap;
  const double* pe = pg + cap;
  const double s = v.S[(size_t)b * 16];
  const double len = v.lengths[l];
  double sm[3] = {0.0, 0.0, 0.0};
  int cnt = 0;
  for (int k = tid; k < v.slots; k += T) {
    const long long fl = (long long)k * v.step;                  // < cap by the definition of slots
    const int f = (int)fl;
    int end = -1;
    if (f < n && used[f]) {
      const double target = pg[f] + len;
      int lo = f + 1, hi = n;                                    // the first row j > f with prefix[j] > target: the prefix never falls
      while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (pg[mid] > target) hi = mid; else lo = mid + 1;
      }
      if (lo < n && used[lo]) {
        end = lo;
        double c_rot, th, d;
        pair_error(v, in, b, f, end, s, c_rot, th, d);
        cnt++;
        sm[0] += d / len; sm[1] += th / len; sm[2] += (pe[end] - pe[f]) / (pg[end] - pg[f]);
      }
    }
    if (out.seg_end) out.seg_end[((size_t)b * v.slots + k) * L + l] = end;
  }
  const int Ns = tree_isum(cnt, ilds, tid);
  tree_sum<3>(sm, lds, tid);
  if (tid != 0) return;
  double* o = out.seg + ((size_t)b * (L + 1) + l) * TRAJ_SEG;
  double* q = v.segsum + ((size_t)b * L + l) * 4;
  const double Nd = (double)Ns;
  o[0] = Nd; q[0] = Nd;
  for (int c = 0; c < 3; c++) { o[1 + c] = Ns > 0 ? sm[c] / Nd : 0.0; q[1 + c] = sm[c]; }
}

// the row over all segments: a lane per b adds the lengths' sums in table order
__global__ __launch_bounds__(64) void traj_segall_kernel(TrajView v, TrajOut out) {
  const int b = threadIdx.x, L = v.L;
  if (b >= v.B) return;
  double tot[3] = {0.0, 0.0, 0.0}, totn = 0.0;
  for (int l = 0; l < L; l++) {
    const double* q = v.segsum + ((size_t)b * L + l) * 4;
    totn += q[0];                                                // counts: exact in fp64
    for (int c = 0; c < 3; c++) tot[c] += q[1 + c];
  }
  double* o = out.seg + ((size_t)b * (L + 1) + L) * TRAJ_SEG;
  o[0] = totn;
  for (int c = 0; c < 3; c++) o[1 + c] = totn > 0.0 ? tot[c] / totn : 0.0;
}

// ------------------------------------------------------------------------------------------------ closures
__global__ __launch_bounds__(T) void traj_clo_kernel(TrajView v, TrajIn in, TrajOut out) {
  __shared__ double lds[2 * T];
  __shared__ int ilds[T];
  const int tid = threadIdx.x, EC = v.edge_capacity;
  const int n = clampi(in.n[0], v.cap), E = clampi(in.e_state[0], EC);
  double sm[2] = {0.0, 0.0}, mxv[2] = {0.0, 0.0};
  int cnt = 0, wrong = 0;
  for (int a = tid; a < EC; a += T) {
    bool ok = a < E;
    int i = 0, j = 0;
    if (ok) {
      i = in.e_ij[2 * (size_t)a]; j = in.e_ij[2 * (size_t)a + 1];
      ok = i >= 0 && i < n && j >= 0 && j < n && i != j;
      if (ok) ok = v.gtok[i] != 0 && v.gtok[j] != 0;             // 0 <= i, j < n <= cap
      for (int c = 0; c < 12; c++) ok = ok && fin(in.e_Z[(size_t)a * 12 + c]);
    }
    double th = -1.0, d = -1.0;
    if (ok) {
      double RG[9], tG[3], RZ[9], tZ[3], c_rot;
      gt_rel(v, in.gt, i, j, RG, tG);
      load_pose(in.e_Z + (size_t)a * 12, RZ, tZ);
      rel_error(RG, tG, RZ, tZ, c_rot, th, d);
      cnt++;
      wrong += (th > v.rot_thr || d > v.trans_thr) ? 1 : 0;
      sm[0] += th * th; sm[1] += d * d;
      mxv[0] = fmax(mxv[0], th); mxv[1] = fmax(mxv[1], d);
    }
    if (out.edge_err) { out.edge_err[2 * (size_t)a] = th; out.edge_err[2 * (size_t)a + 1] = d; }
  }
  const int Ne = tree_isum(cnt, ilds, tid), Nw = tree_isum(wrong, ilds, tid);
  tree_sum<2>(sm, lds, tid);
  tree_max<2>(mxv, lds, tid);
  if (tid != 0) return;
  const double Nd = (double)Ne;
  out.clo[0] = Nd; out.clo[1] = (double)Nw;
  out.clo[2] = Ne > 0 ? sqrt(sm[0] / Nd) : 0.0; out.clo[3] = mxv[0];
  out.clo[4] = Ne > 0 ? sqrt(sm[1] / Nd) : 0.0; out.clo[5] = mxv[1];
  out.clo[6] = (double)E; out.clo[7] = 0.0;
}

}  // namespace

void launch_trajeval(hipStream_t st, const TrajView& v, const TrajIn& in, const TrajOut& out) {
  const dim3 blk(T);
  hipLaunchKernelGGL(traj_prepare_kernel, dim3((v.cap + T - 1) / T, v.B + 1), blk, 0, st, v, in, out);
  hipLaunchKernelGGL(traj_ate_kernel, dim3(v.B), blk, 0, st, v, in, out);
  if (v.K > 0) hipLaunchKernelGGL(traj_rpe_kernel, dim3(v.K, v.B), blk, 0, st, v, in, out);
  if (v.L > 0) {
    hipLaunchKernelGGL(traj_seg_kernel, dim3(v.L, v.B), blk, 0, st, v, in, out);
    hipLaunchKernelGGL(traj_segall_kernel, dim3(1), dim3(64), 0, st, v, out);
  }
  if (v.edge_capacity > 0 && in.e_ij) hipLaunchKernelGGL(traj_clo_kernel, dim3(1), blk, 0, st, v, in, out);
}

}  // namespace pr
