// gate.hip — the closure consistency gate in front of the pose-graph relaxation (no reference counterpart).
// A logged closure is used only when enough other closures, carried along the odometry chain of the input poses, say the same thing.
// The rule is in include/place_recognition.h and restated in tests/gate_np.py; the device equals it bit for bit (fp64 + and x only,
// no contraction).  Every grid depends on the create sizes only and both counts are read from device memory, so one captured run
// serves every count.
//   prepare   a lane per edge slot: the counts, validity, L = Z^-1 P_i, M = (P_i^-1 Z) P_j, N = P_j^-1 (36 doubles), keep_0, zero sums
//   round     all ordered pairs: a lane per a holding L_a, N_a, i_a, j_a; tiles of 64 b (M_b, i_b, j_b, keep_{r-1}[b]) staged in LDS and
//             read by every lane at the same address (a broadcast); the integer tests come before any floating-point work; the b
//             range is split over grid.y and the counts are combined by integer atomic adds, whose sum does not depend on their order
//   decide    a lane per edge slot: keep_r = keep_{r-1} and s_r >= min_support; the last round's s_r is the support that is reported
//   scan      one workgroup: the ranks of the kept edges in log order, the counts, the flags, dst.state, info
//   copy      a lane per edge slot: row a of src to row map[a] of dst
// No floating-point atomics, no workgroup waits for another, every loop is bounded by a create size.  Plain C++, vector stores only.
#include "gate.hpp"

namespace pr {
namespace {

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ bool fin(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }       // false for NaN and Inf

// ------------------------------------------------------------------------------------------------ 3 x 3 helpers (row-major), restated
// from posegraph.hip in the same operation order
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
// pose row p [12] = [R | t] row-major 3 x 4
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

// ------------------------------------------------------------------------------------------------ prepare
__global__ __launch_bounds__(256) void gate_prepare_kernel(GateView v, const double* __restrict__ poses, const int* __restrict__ n_dev) {
  const int a = blockIdx.x * 256 + threadIdx.x, EC = v.edge_capacity;
  const int E = clampi(v.s_state[0], EC), n = clampi(n_dev[0], v.node_capacity);     // a scribbled count never forms an address
  if (a == 0) { v.ctl[0] = n; v.ctl[1] = E; v.ctl[2] = v.s_state[1] & GATE_LOG_OVERFLOW; v.ctl[3] = 0; }
  if (a >= EC) return;
  bool ok = a < E;
  int i = 0, j = 0;
  if (ok) {
    i = v.s_ij[2 * (size_t)a]; j = v.s_ij[2 * (size_t)a + 1];
    ok = i >= 0 && i < n && j >= 0 && j < n && i != j;
    for (int c = 0; c < 12; c++) ok = ok && fin(v.s_Z[(size_t)a * 12 + c]);
    ok = ok && fin(v.s_w[2 * (size_t)a]) && fin(v.s_w[2 * (size_t)a + 1]);
    if (ok)                                                      // 0 <= i, j < n <= node_capacity
      for (int c = 0; c < 12; c++) ok = ok && fin(poses[(size_t)i * 12 + c]) && fin(poses[(size_t)j * 12 + c]);
  }
  v.valid[a] = ok ? 1 : 0;
  v.keep[0][a] = ok ? 1 : 0;
  v.sup[a] = 0;
  v.eij[2 * (size_t)a] = ok ? i : 0; v.eij[2 * (size_t)a + 1] = ok ? j : 0;
  if (!ok) return;
  double Rz[9], tz[3], Ri[9], ti[3], Rj[9], tj[3], Rv[9], tv[3], Ra[9], ta[3], Rb[9], tb[3];
  load_pose(v.s_Z + (size_t)a * 12, Rz, tz);
  load_pose(poses + (size_t)i * 12, Ri, ti);
  load_pose(poses + (size_t)j * 12, Rj, tj);
  double* out = v.lmn + (size_t)a * GATE_LMN;
  rigid_inv(Rz, tz, Rv, tv);                                     // L = Z^-1 P_i
  rigid_mul(Rv, tv, Ri, ti, Ra, ta);
  store_pose(out, Ra, ta);
  rigid_inv(Ri, ti, Rv, tv);                                     // M = (P_i^-1 Z) P_j
  rigid_mul(Rv, tv, Rz, tz, Ra, ta);
  rigid_mul(Ra, ta, Rj, tj, Rb, tb);
  store_pose(out + 12, Rb, tb);
  rigid_inv(Rj, tj, Rv, tv);                                     // N = P_j^-1
  store_pose(out + 24, Rv, tv);
}

// ------------------------------------------------------------------------------------------------ round r (1-based)
__global__ __launch_bounds__(256) void gate_round_kernel(GateView v, int r) {
  __shared__ double sM[GATE_TILE * 12];
  __shared__ int sI[GATE_TILE], sJ[GATE_TILE], sK[GATE_TILE];
  const int tid = threadIdx.x, a = blockIdx.x * 256 + tid;
  const int E = clampi(v.ctl[1], v.edge_capacity);
  if (blockIdx.x * 256 >= E) return;                             // the whole workgroup: no lane of it is an edge
  const int* keep_prev = v.keep[(r - 1) & 1];
  const bool mine = a < E && v.valid[a] != 0;
  double RL[9], tL[3], RN[9], tN[3];
  int ia = 0, ja = 0;
  if (mine) {
    load_pose(v.lmn + (size_t)a * GATE_LMN, RL, tL);
    load_pose(v.lmn + (size_t)a * GATE_LMN + 24, RN, tN);
    ia = v.eij[2 * (size_t)a]; ja = v.eij[2 * (size_t)a + 1];
  } else {
#pragma unroll
    for (int c = 0; c < 9; c++) { RL[c] = 0.0; RN[c] = 0.0; }
#pragma unroll
    for (int c = 0; c < 3; c++) { tL[c] = 0.0; tN[c] = 0.0; }
  }
  int count = 0;
  const int tiles = (E + GATE_TILE - 1) / GATE_TILE;             // <= ceil(edge_capacity / GATE_TILE)
  for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
    const int b0 = t * GATE_TILE;
    __syncthreads();                                             // the tile before this one has been read by every lane
    for (int q = tid; q < GATE_TILE * 12; q += 256) {
      const int b = b0 + q / 12;
      sM[q] = b < E ? v.lmn[(size_t)b * GATE_LMN + 12 + q % 12] : 0.0;
    }
    if (tid < GATE_TILE) {
      const int b = b0 + tid;
      const bool in = b < E;
      sI[tid] = in ? v.eij[2 * (size_t)b] : 0; sJ[tid] = in ? v.eij[2 * (size_t)b + 1] : 0; sK[tid] = in ? keep_prev[b] : 0;
    }
    __syncthreads();
    if (!mine) continue;
    for (int q = 0; q < GATE_TILE; q++) {
      if (!sK[q]) continue;                                      // (kept implies valid)
      const int di = ia - sI[q], dj = ja - sJ[q];
      const int gap = (di < 0 ? -di : di) + (dj < 0 ? -dj : dj); // rows are below 2^20: no overflow
      if (b0 + q == a || gap > v.max_gap || dj == 0) continue;
      double RM[9], tM[3], RY[9], tY[3], y[3];
      load_pose(sM + q * 12, RM, tM);
      rigid_mul(RL, tL, RM, tM, RY, tY);                         // Y = L_a M_b
      // X = Y N_a: the diagonal of the rotation and the translation
      const double x00 = RY[0] * RN[0] + RY[1] * RN[3] + RY[2] * RN[6];
      const double x11 = RY[3] * RN[1] + RY[4] * RN[4] + RY[5] * RN[7];
      const double x22 = RY[6] * RN[2] + RY[7] * RN[5] + RY[8] * RN[8];
      mv3(RY, tN, y);
      const double tx = y[0] + tY[0], ty = y[1] + tY[1], tz = y[2] + tY[2];
      const double c_rot = 3.0 - ((x00 + x11) + x22), c_trans = (tx * tx + ty * ty) + tz * tz;
      count += (c_rot <= v.rot_tab[gap] && c_trans <= v.trans2_tab[gap]) ? 1 : 0;         // a NaN supports nothing
    }
  }
  if (mine && count > 0) atomicAdd(&v.sup[a], count);
}

// ------------------------------------------------------------------------------------------------ decide
__global__ __launch_bounds__(256) void gate_decide_kernel(GateView v, int r, int last, int* __restrict__ support_out) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= v.edge_capacity) return;
  const int s = v.sup[a];
  v.keep[r & 1][a] = (v.keep[(r - 1) & 1][a] != 0 && s >= v.min_support) ? 1 : 0;
  if (!last) v.sup[a] = 0;
  else if (support_out) support_out[a] = v.valid[a] ? s : -1;
}

// ------------------------------------------------------------------------------------------------ scan
__global__ __launch_bounds__(256) void gate_scan_kernel(GateView v, unsigned char* __restrict__ keep_out, int* __restrict__ map_out,
                                                        int* __restrict__ info) {
  __shared__ int part[256], pval[256], pdiff[256];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x, EC = v.edge_capacity;
  const int* kf = v.keep[v.rounds & 1];
  const int* kp = v.keep[(v.rounds - 1) & 1];
  const int chunk = (EC + 255) / 256, a0 = tid * chunk < EC ? tid * chunk : EC, a1 = a0 + chunk < EC ? a0 + chunk : EC;
  int kept = 0, val = 0, diff = 0;
  for (int a = a0; a < a1; a++) { kept += kf[a]; val += v.valid[a]; diff |= kf[a] != kp[a] ? 1 : 0; }
  part[tid] = kept; pval[tid] = val; pdiff[tid] = diff;
  __syncthreads();
  if (tid == 0) {
    int run = 0, vs = 0, ds = 0;
    for (int t = 0; t < 256; t++) { const int d = part[t]; part[t] = run; run += d; vs += pval[t]; ds |= pdiff[t]; }
    const int flags = (v.ctl[2] ? GATE_SRC_OVERFLOW : 0) | (ds ? GATE_UNSETTLED : 0);
    info[0] = vs; info[1] = run; info[2] = v.ctl[1]; info[3] = flags;
    v.d_state[0] = run; v.d_state[1] = v.ctl[2]; v.d_state[2] = 0; v.d_state[3] = 0;
  }
  __syncthreads();
  int run = part[tid];
  for (int a = a0; a < a1; a++) {
    const int k = kf[a], m = k ? run++ : -1;
    v.map[a] = m;
    if (map_out) map_out[a] = m;
    if (keep_out) keep_out[a] = k ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ copy
__global__ __launch_bounds__(256) void gate_copy_kernel(GateView v) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= v.edge_capacity) return;
  const int m = v.map[a];                                        // < kept <= edge_capacity <= dst_edge_capacity
  if (m < 0) return;
  v.d_ij[2 * (size_t)m] = v.s_ij[2 * (size_t)a]; v.d_ij[2 * (size_t)m + 1] = v.s_ij[2 * (size_t)a + 1];
  for (int c = 0; c < 12; c++) v.d_Z[(size_t)m * 12 + c] = v.s_Z[(size_t)a * 12 + c];
  v.d_w[2 * (size_t)m] = v.s_w[2 * (size_t)a]; v.d_w[2 * (size_t)m + 1] = v.s_w[2 * (size_t)a + 1];
}

}  // namespace

void launch_gate(hipStream_t st, const GateView& v, const double* poses, const int* n, unsigned char* keep, int* support, int* map, int* info) {
  const dim3 one(1), blk(256), slots((v.edge_capacity + 255) / 256), pairs((v.edge_capacity + 255) / 256, gate_split(v.edge_capacity));
  hipLaunchKernelGGL(gate_prepare_kernel, slots, blk, 0, st, v, poses, n);
  for (int r = 1; r <= v.rounds; r++) {
    hipLaunchKernelGGL(gate_round_kernel, pairs, blk, 0, st, v, r);
    hipLaunchKernelGGL(gate_decide_kernel, slots, blk, 0, st, v, r, r == v.rounds ? 1 : 0, support);
  }
  hipLaunchKernelGGL(gate_scan_kernel, one, blk, 0, st, v, keep, map, info);
  hipLaunchKernelGGL(gate_copy_kernel, slots, blk, 0, st, v);
}

}  // namespace pr
