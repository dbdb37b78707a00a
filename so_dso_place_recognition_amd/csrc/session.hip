// session.hip — drive sessions: where each drive begins in the map's rows, and the consensus rigid alignment of a later drive onto the
// earlier ones from the cross-drive closures of a log (the reference's two-drive setting, test_robotcar.m, has no pose
// stage).  The rule is in include/place_recognition.h and restated in tests/session_np.py; everything the rule decides in integers, every
// hypothesis G_a and every row that is only copied equals the restatement bit for bit (fp64 + and x only up to the choice, no
// contraction).  Every grid depends on the create sizes only and every count is read from device memory, so one captured call serves
// every count.
//   reset, begin   one thread: the table's rule
//   rows      a lane per row, the table's starts staged in LDS: sid and breaks alone (in front of a relaxation across breaks)
//   prepare   a lane per row and a lane per edge slot; the table's starts staged in LDS: sid and breaks of the rows; the counts, the
//             target, which slots are candidates, G_a, c_a, G_a c_a, zero sums
//   pairs     all ordered pairs: a lane per a holding G_a and q_a; tiles of 64 b (R_Gb, c_b, G_b c_b, q_b, candidate) staged in LDS and read
//             by every lane at the same address (a broadcast); the integer tests come before any floating-point work; the b range is
//             split over grid.y and the counts are combined by integer atomic adds, whose sum does not depend on their order
//   choose    ONE workgroup: does the target have a row, the integer argmax (ties to the lowest log index), the members of I, the sums
//             of the refinement by block_sum256's fixed tree, G and G^-1
//   apply     a lane per row and a lane per edge slot: P_r G^-1 or the row's bytes; hyp, support, inlier, info
// No floating-point atomics, no workgroup waits for another, every loop is bounded by a create size.  Plain C++, vector stores only.
#include "session.hpp"
#include "rerank_common.hpp"

namespace pr {
namespace {

constexpr double SESSION_SMALL = 1e-4;       // posegraph's one small-angle branch of log_SO3 and exp

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool fin(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }       // false for NaN and Inf

// ------------------------------------------------------------------------------------------------ 3 x 3 helpers (row-major), restated
// from gate.hip in the same operation order
__device__ __forceinline__ void mul33(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void mv3(const double* A, const double* x, double* y) {            // A x
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
__device__ __forceinline__ void mtv3(const double* A, const double* x, double* y) {           // A^T x
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = A[r] * x[0] + A[3 + r] * x[1] + A[6 + r] * x[2];
}
__device__ __forceinline__ void load_pose(const double* p, double* R, double* t) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    R[3 * r] = p[4 * r]; R[3 * r + 1] = p[4 * r + 1]; R[3 * r + 2] = p[4 * r + 2]; t[r] = p[4 * r + 3];
  }
}
__device__ __forceinline__ void store_pose(double* p, const double* R, const double* t) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    p[4 * r] = R[3 * r]; p[4 * r + 1] = R[3 * r + 1]; p[4 * r + 2] = R[3 * r + 2]; p[4 * r + 3] = t[r];
  }
}
// C = A B = [R_A R_B | R_A t_B + t_A]
__device__ __forceinline__ void rigid_mul(const double* RA, const double* tA, const double* RB, const double* tB, double* RC, double* tC) {
  double y[3];
  mul33(RA, RB, RC);
  mv3(RA, tB, y);
  tC[0] = y[0] + tA[0]; tC[1] = y[1] + tA[1]; tC[2] = y[2] + tA[2];
}
// A^-1 = [R^T | -(R^T t)]
__device__ __forceinline__ void rigid_inv(const double* R, const double* t, double* Ri, double* ti) {
  double y[3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Ri[3 * r + c] = R[3 * c + r];
  mtv3(R, t, y);
  ti[0] = -y[0]; ti[1] = -y[1]; ti[2] = -y[2];
}

// does b support a: the two floating-point tests of the rule (the integer tests are the caller's)
__device__ __forceinline__ bool supports(const double* Ra, const double* ta, const double* Rb, const double* cb, const double* pb, double rot_c_max,
                                         double trans2_max) {
  const double x00 = Ra[0] * Rb[0] + Ra[3] * Rb[3] + Ra[6] * Rb[6];                            // the diagonal of R_Ga^T R_Gb
  const double x11 = Ra[1] * Rb[1] + Ra[4] * Rb[4] + Ra[7] * Rb[7];
  const double x22 = Ra[2] * Rb[2] + Ra[5] * Rb[5] + Ra[8] * Rb[8];
  const double c_rot = 3.0 - ((x00 + x11) + x22);
  double y[3];
  mv3(Ra, cb, y);                                                                              // G_a c_b - G_b c_b
  const double dx = (y[0] + ta[0]) - pb[0], dy = (y[1] + ta[1]) - pb[1], dz = (y[2] + ta[2]) - pb[2];
  const double c_trans = (dx * dx + dy * dy) + dz * dz;
  return c_rot <= rot_c_max && c_trans <= trans2_max;                                          // a NaN supports nothing
}

// ------------------------------------------------------------------------------------------------ the table
__global__ void session_reset_kernel(SessionView v) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  v.start[0] = 0;
  v.state[0] = 1; v.state[1] = 0; v.state[2] = 0; v.state[3] = 0;
}

__global__ void session_begin_kernel(SessionView v, const int* __restrict__ n_dev, int* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int SC = v.session_capacity;
  const int S = clampi(v.state[0], 1, SC), n = clampi(n_dev[0], 0, v.node_capacity);          // a scribbled count never forms an address
  int flags = v.state[1] & SESSION_OVERFLOW;
  const int last = S > 1 ? v.start[S - 1] : 0;                                                 // session 0 begins at row 0 by definition
  if (n == last) {                                                                             // the last session is still empty
    info[0] = S - 1; info[1] = last; info[2] = S; info[3] = flags | SESSION_REUSED;
  } else if (S == SC) {
    flags |= SESSION_OVERFLOW;
    v.state[1] = flags;
    info[0] = S - 1; info[1] = last; info[2] = S; info[3] = flags;
  } else {
    v.start[S] = n;                                                                            // S < session_capacity
    v.state[0] = S + 1;
    info[0] = S; info[1] = n; info[2] = S + 1; info[3] = flags;
  }
}

// ------------------------------------------------------------------------------------------------ prepare
// sid(r) = #{q in 1 .. S - 1 : start[q] <= r} and the same for r - 1, from the starts in LDS
__device__ __forceinline__ void sid_pair(const int* sS, int S, int r, int& here, int& before) {
  int a = 0, b = 0;
  for (int q = 1; q < S; q++) { const int s = sS[q]; a += s <= r ? 1 : 0; b += s < r ? 1 : 0; }   // s <= r - 1 without the subtraction
  here = a; before = b;
}

// the starts of the table into LDS (every lane of the workgroup calls it) -> S
__device__ __forceinline__ int stage_starts(const SessionView& v, int* sS, int tid) {
  const int S = clampi(v.state[0], 1, v.session_capacity);                                     // <= SESSION_MAX
  for (int q = tid; q < S; q += 256) sS[q] = v.start[q];
  __syncthreads();
  return S;
}
// sid and break of row x
__device__ __forceinline__ void row_part(const SessionView& v, const int* sS, int S, int x) {
  if (x >= v.node_capacity) return;
  int here, before;
  sid_pair(sS, S, x, here, before);
  v.sid[x] = here;
  v.brk[x] = (x >= 1 && here != before) ? 1 : 0;
}

// the rows alone: what the relaxation across breaks needs of the table
__global__ __launch_bounds__(256) void session_rows_kernel(SessionView v) {
  __shared__ int sS[SESSION_MAX];
  const int S = stage_starts(v, sS, threadIdx.x);
  row_part(v, sS, S, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void session_prepare_kernel(SessionView v, SessionAlign al, const double* poses, const int* __restrict__ n_dev) {
  __shared__ int sS[SESSION_MAX];
  const int tid = threadIdx.x, x = blockIdx.x * 256 + tid, EC = v.edge_capacity;
  const int S = stage_starts(v, sS, tid);
  row_part(v, sS, S, x);
  const int n = clampi(n_dev[0], 0, v.node_capacity), E = clampi(al.e_state[0], 0, al.log_edge_capacity);   // log_edge_capacity <= EC
  const int t = al.session == -1 ? S - 1 : al.session;
  if (x == 0) {
    v.ctl[0] = n; v.ctl[1] = E; v.ctl[2] = S; v.ctl[3] = t;
    v.ctl[9] = (v.state[1] & SESSION_OVERFLOW) | ((al.e_state[1] & SESSION_POSEGRAPH_OVERFLOW) ? SESSION_LOG_OVERFLOW : 0);
  }
  if (x >= EC) return;
  const size_t a = (size_t)x;
  bool ok = x < E && t > 0 && t < S;
  int i = 0, j = 0;
  if (ok) {
    i = al.e_ij[2 * a]; j = al.e_ij[2 * a + 1];
    ok = i >= 0 && i < n && j >= 0 && j < n && i != j;
    for (int c = 0; c < 12; c++) ok = ok && fin(al.e_Z[a * 12 + c]);
    ok = ok && fin(al.e_w[2 * a]) && fin(al.e_w[2 * a + 1]);
    if (ok)                                                      // 0 <= i, j < n <= node_capacity
      for (int c = 0; c < 12; c++) ok = ok && fin(poses[(size_t)i * 12 + c]) && fin(poses[(size_t)j * 12 + c]);
  }
  bool j_in_t = false;
  if (ok) {
    int si, sj, unused;
    sid_pair(sS, S, i, si, unused);
    sid_pair(sS, S, j, sj, unused);
    j_in_t = sj == t && si < t;
    ok = j_in_t || (si == t && sj < t);                          // exactly one end in t, the other in an earlier session
  }
  const int qa = ok ? (j_in_t ? j : i) : 0;
  v.cand[a] = ok ? 1 : 0; v.q[a] = qa; v.sup[a] = 0; v.inl[a] = 0;
  double* hyp = v.hyp + a * 12;
  if (!ok) {
    for (int c = 0; c < 12; c++) hyp[c] = 0.0;
    for (int c = 0; c < 3; c++) { v.c[a * 3 + c] = 0.0; v.p[a * 3 + c] = 0.0; }
    return;
  }
  double Rz[9], tz[3], Ri[9], ti[3], Rj[9], tj[3], Rv[9], tv[3], Ra[9], ta[3], RG[9], tG[3], Rw[9], tw[3], cq[3], y[3];
  load_pose(al.e_Z + a * 12, Rz, tz);
  load_pose(poses + (size_t)i * 12, Ri, ti);
  load_pose(poses + (size_t)j * 12, Rj, tj);
  if (j_in_t) {                                                  // G = (P_i^-1 Z) P_j
    rigid_inv(Ri, ti, Rv, tv);
    rigid_mul(Rv, tv, Rz, tz, Ra, ta);
    rigid_mul(Ra, ta, Rj, tj, RG, tG);
    rigid_inv(Rj, tj, Rw, cq);                                   // c = -(R_j^T t_j)
  } else {                                                       // G = (P_j^-1 Z^-1) P_i
    rigid_inv(Rj, tj, Rv, tv);
    rigid_inv(Rz, tz, Rw, tw);
    rigid_mul(Rv, tv, Rw, tw, Ra, ta);
    rigid_mul(Ra, ta, Ri, ti, RG, tG);
    rigid_inv(Ri, ti, Rw, cq);
  }
  store_pose(hyp, RG, tG);
  mv3(RG, cq, y);
  for (int c = 0; c < 3; c++) { v.c[a * 3 + c] = cq[c]; v.p[a * 3 + c] = y[c] + tG[c]; }
}

// ------------------------------------------------------------------------------------------------ pairs
__global__ __launch_bounds__(256) void session_pairs_kernel(SessionView v, double rot_c_max, double trans2_max) {
  __shared__ double sR[SESSION_TILE * 9], sC[SESSION_TILE * 3], sP[SESSION_TILE * 3];
  __shared__ int sQ[SESSION_TILE], sK[SESSION_TILE];
  const int tid = threadIdx.x, a = blockIdx.x * 256 + tid;
  const int E = clampi(v.ctl[1], 0, v.edge_capacity);
  if (blockIdx.x * 256 >= E) return;                             // the whole workgroup: no lane of it is an edge
  const bool mine = a < E && v.cand[a] != 0;
  double Ra[9], ta[3];
  int qa = 0;
  if (mine) { load_pose(v.hyp + (size_t)a * 12, Ra, ta); qa = v.q[a]; }
  else {
#pragma unroll
    for (int c = 0; c < 9; c++) Ra[c] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) ta[c] = 0.0;
  }
  int count = 0;
  const int tiles = (E + SESSION_TILE - 1) / SESSION_TILE;       // <= ceil(edge_capacity / SESSION_TILE)
  for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
    const int b0 = t * SESSION_TILE;
    __syncthreads();                                             // the tile before this one has been read by every lane
    for (int w = tid; w < SESSION_TILE * 9; w += 256) {
      const int b = b0 + w / 9, e = w % 9;
      sR[w] = b < E ? v.hyp[(size_t)b * 12 + 4 * (e / 3) + e % 3] : 0.0;
    }
    if (tid < SESSION_TILE * 3) {
      const int b = b0 + tid / 3;
      sC[tid] = b < E ? v.c[(size_t)b * 3 + tid % 3] : 0.0;
      sP[tid] = b < E ? v.p[(size_t)b * 3 + tid % 3] : 0.0;
    }
    if (tid < SESSION_TILE) {
      const int b = b0 + tid;
      sQ[tid] = b < E ? v.q[b] : 0; sK[tid] = b < E ? v.cand[b] : 0;
    }
    __syncthreads();
    if (!mine) continue;
    for (int w = 0; w < SESSION_TILE; w++) {
      if (!sK[w] || b0 + w == a || sQ[w] == qa) continue;        // the integer tests first
      count += supports(Ra, ta, sR + w * 9, sC + w * 3, sP + w * 3, rot_c_max, trans2_max) ? 1 : 0;
    }
  }
  if (mine && count > 0) atomicAdd(&v.sup[a], count);
}

// ------------------------------------------------------------------------------------------------ choose + refine
__global__ __launch_bounds__(256) void session_choose_kernel(SessionView v, int min_inliers, double rot_c_max, double trans2_max, double* __restrict__ G_out) {
  __shared__ int sBest[256], sArg[256], sCnt[256], sHas[256];
  __shared__ double red[4];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  const int n = clampi(v.ctl[0], 0, v.node_capacity), E = clampi(v.ctl[1], 0, v.edge_capacity), S = v.ctl[2], t = v.ctl[3];
  int has = 0, best = -1, arg = -1, cnt = 0;
  for (int r = tid; r < n; r += 256) has |= v.sid[r] == t ? 1 : 0;
  for (int a = tid; a < E; a += 256) {                           // ascending a: the first of equal supports is the lowest
    if (!v.cand[a]) continue;
    cnt++;
    const int s = v.sup[a];
    if (s > best) { best = s; arg = a; }
  }
  sBest[tid] = best; sArg[tid] = arg; sCnt[tid] = cnt; sHas[tid] = has;
  __syncthreads();
  if (tid == 0) {
    int b = -1, g = -1, c = 0, h = 0;
    for (int w = 0; w < 256; w++) {
      c += sCnt[w]; h |= sHas[w];
      if (sArg[w] >= 0 && (sBest[w] > b || (sBest[w] == b && sArg[w] < g))) { b = sBest[w]; g = sArg[w]; }
    }
    sBest[0] = b; sArg[0] = g; sCnt[0] = c; sHas[0] = h;
  }
  __syncthreads();
  const int astar = sArg[0], support = astar >= 0 ? sBest[0] : 0, cands = sCnt[0];
  const bool target = t > 0 && t < S && sHas[0] != 0;
  int status = !target ? SESSION_NO_TARGET : (cands == 0 ? SESSION_NO_CANDIDATE : (support + 1 < min_inliers ? SESSION_WEAK : SESSION_ALIGNED));
  __syncthreads();                                               // everyone has read the four words before red and the arrays are used again
  // the members of I and the sums of the refinement, a lane's members in log order
  double Rs[9], ts[3], acc[9];
#pragma unroll
  for (int c = 0; c < 9; c++) { Rs[c] = c % 4 == 0 ? 1.0 : 0.0; acc[c] = 0.0; }
  ts[0] = ts[1] = ts[2] = 0.0;
  int members = 0;
  if (target && astar >= 0) {
    load_pose(v.hyp + (size_t)astar * 12, Rs, ts);
    const int qs = v.q[astar];
    for (int b = tid; b < E; b += 256) {
      bool in = b == astar;
      double Rb[9], tb[3];
      if (!in && v.cand[b] && v.q[b] != qs) {
        load_pose(v.hyp + (size_t)b * 12, Rb, tb);
        in = supports(Rs, ts, Rb, v.c + (size_t)b * 3, v.p + (size_t)b * 3, rot_c_max, trans2_max);
      }
      v.inl[b] = in ? 1 : 0;
      if (!in) continue;
      members++;
      load_pose(v.hyp + (size_t)b * 12, Rb, tb);
      double RE[9];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) RE[3 * r + c] = Rs[r] * Rb[c] + Rs[3 + r] * Rb[3 + c] + Rs[6 + r] * Rb[6 + c];      // R_Ga*^T R_Gb
      const double vv[3] = {0.5 * (RE[7] - RE[5]), 0.5 * (RE[2] - RE[6]), 0.5 * (RE[3] - RE[1])};
      const double sn = sqrt(vv[0] * vv[0] + vv[1] * vv[1] + vv[2] * vv[2]), cs = 0.5 * (RE[0] + RE[4] + RE[8] - 1.0);
      const double th = atan2(sn, cs);
      const double kf = th < SESSION_SMALL ? 1.0 + th * th / 6.0 : th / sn;
      for (int c = 0; c < 3; c++) { acc[c] += kf * vv[c]; acc[3 + c] += v.p[(size_t)b * 3 + c]; acc[6 + c] += v.c[(size_t)b * 3 + c]; }
    }
  }
  sCnt[tid] = members;
  __syncthreads();
  if (tid == 0) { int m = 0; for (int w = 0; w < 256; w++) m += sCnt[w]; sCnt[0] = m; }
  __syncthreads();
  const int m = sCnt[0];
  double sum[9];
  for (int c = 0; c < 9; c++) sum[c] = block_sum256(acc[c], red, tid);
  if (tid != 0) return;
  double RG[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tG[3] = {0.0, 0.0, 0.0};
  if (status == SESSION_ALIGNED) {
    const double dm = (double)m;                                 // >= 1: a* is a member
    const double w[3] = {sum[0] / dm, sum[1] / dm, sum[2] / dm}, mp[3] = {sum[3] / dm, sum[4] / dm, sum[5] / dm},
                 mc[3] = {sum[6] / dm, sum[7] / dm, sum[8] / dm};
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(t2);
    double ka, kb;
    if (th < SESSION_SMALL) { ka = 1.0 - t2 / 6.0; kb = 0.5 - t2 / 24.0; }
    else { ka = sin(th) / th; kb = (1.0 - cos(th)) / t2; }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double Ex[9], Rn[9], y[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) Ex[3 * r + c] = (r == c ? 1.0 : 0.0) + ka * K[3 * r + c] + kb * (w[r] * w[c] - (r == c ? t2 : 0.0));
    mul33(Rs, Ex, Rn);
    mv3(Rn, mc, y);
    const double tn[3] = {mp[0] - y[0], mp[1] - y[1], mp[2] - y[2]};
    bool f = true;
    for (int c = 0; c < 9; c++) f = f && fin(Rn[c]);
    for (int c = 0; c < 3; c++) f = f && fin(tn[c]);
    if (f) {
      for (int c = 0; c < 9; c++) RG[c] = Rn[c];
      for (int c = 0; c < 3; c++) tG[c] = tn[c];
    } else {
      status = SESSION_NONFINITE;
    }
  }
  double Rv[9], tv[3];
  rigid_inv(RG, tG, Rv, tv);
  store_pose(v.gd, RG, tG);
  store_pose(v.gd + 12, Rv, tv);
  store_pose(G_out, RG, tG);
  v.ctl[4] = status; v.ctl[5] = astar; v.ctl[6] = support; v.ctl[7] = cands; v.ctl[8] = m;
}

// ------------------------------------------------------------------------------------------------ apply
__global__ __launch_bounds__(256) void session_apply_kernel(SessionView v, const double* poses_in, double* poses_out, double* __restrict__ hyp,
                                                            int* __restrict__ support, unsigned char* __restrict__ inlier, int* __restrict__ info) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int n = clampi(v.ctl[0], 0, v.node_capacity);
  if (x < n) {                                                   // rows >= n are not written
    double row[12];
    bool f = true;
    for (int c = 0; c < 12; c++) { row[c] = poses_in[(size_t)x * 12 + c]; f = f && fin(row[c]); }
    if (v.ctl[4] == SESSION_ALIGNED && v.sid[x] == v.ctl[3] && f) {
      double R[9], t[3], Rv[9], tv[3], Rn[9], tn[3];
      load_pose(row, R, t);
      load_pose(v.gd + 12, Rv, tv);
      rigid_mul(R, t, Rv, tv, Rn, tn);                           // P_r G^-1
      store_pose(row, Rn, tn);
    }
    for (int c = 0; c < 12; c++) poses_out[(size_t)x * 12 + c] = row[c];
  }
  if (x < v.edge_capacity) {
    if (hyp)
      for (int c = 0; c < 12; c++) hyp[(size_t)x * 12 + c] = v.hyp[(size_t)x * 12 + c];
    if (support) support[x] = v.cand[x] ? v.sup[x] : -1;
    if (inlier) inlier[x] = v.inl[x] ? 1 : 0;
  }
  if (x == 0) {
    info[0] = v.ctl[4]; info[1] = v.ctl[5]; info[2] = v.ctl[6]; info[3] = v.ctl[7];
    info[4] = v.ctl[8]; info[5] = v.ctl[1]; info[6] = v.ctl[0]; info[7] = v.ctl[9];
  }
}

}  // namespace

void launch_session_reset(hipStream_t st, const SessionView& v) { hipLaunchKernelGGL(session_reset_kernel, dim3(1), dim3(64), 0, st, v); }

void launch_session_begin(hipStream_t st, const SessionView& v, const int* n, int* info) {
  hipLaunchKernelGGL(session_begin_kernel, dim3(1), dim3(64), 0, st, v, n, info);
}

void launch_session_rows(hipStream_t st, const SessionView& v) {
  hipLaunchKernelGGL(session_rows_kernel, dim3((v.node_capacity + 255) / 256), dim3(256), 0, st, v);
}

void launch_session_align(hipStream_t st, const SessionView& v, const SessionAlign& a, const double* poses_in, const int* n, double* poses_out,
                          double* G, double* hyp, int* support, unsigned char* inlier, int* info) {
  const int most = v.node_capacity > v.edge_capacity ? v.node_capacity : v.edge_capacity;
  const dim3 one(1), blk(256), both((most + 255) / 256), pairs((v.edge_capacity + 255) / 256, session_split(v.edge_capacity));
  hipLaunchKernelGGL(session_prepare_kernel, both, blk, 0, st, v, a, poses_in, n);
  hipLaunchKernelGGL(session_pairs_kernel, pairs, blk, 0, st, v, a.rot_c_max, a.trans2_max);
  hipLaunchKernelGGL(session_choose_kernel, one, blk, 0, st, v, a.min_inliers, a.rot_c_max, a.trans2_max, G);
  hipLaunchKernelGGL(session_apply_kernel, both, blk, 0, st, v, poses_in, poses_out, hyp, support, inlier, info);
}

}  // namespace pr
