// posegraph.hip — the loop-closure log and the pose-graph relaxation of the map's poses (no reference counterpart).
// The log is the sibling of map.hip / online.hip for verified closures: caller-owned buffers, a DEVICE-side count, one captured add per
// keyframe.  The relaxation runs damped Gauss-Newton over the odometry chain of the input poses plus the logged edges; every grid
// depends on the create sizes only, both counts are read from device memory, so one captured relax serves every count.
//   add        one workgroup: the accepted, finite slots of one verify, in slot order, to rows edges ..; then state and info
//   prepare    one workgroup: the counts, a copy of the poses, the odometry measurements, which slots are edges, and the incidence
//              list of the logged edges - a counting sort (integer counts, a scan, a fill, then every node's list ranked into log order)
//   linearize  a lane per edge slot: residual, the five non-zero 3 x 3 Jacobian blocks, cost
//   blocks     a lane per node: gradient and 6 x 6 diagonal block gathered over the node's edges in a fixed order (odometry edge
//              a - 1, odometry edge a, the logged edges in log order), the block inverted by Gauss-Jordan without pivoting
//   solve      ONE workgroup: `inner` iterations of preconditioned conjugate gradients behind __syncthreads(), the vectors in the
//              create-time scratch (served from L2), fixed lanes per node and per slot, block_sum256's construction over 16 waves for the dot products; then the update
//   finish     one workgroup: the final cost, the edge count, the poses of rows < n
// A per-node sum is a gather, never a scatter; there are no floating-point atomics (the only atomics are the integer counters of the
// counting sort, whose result - counts, then sorted lists - does not depend on their order), so two runs give the same bytes.  No
// kernel waits for another workgroup.  Plain C++, vector stores only.
#include "posegraph.hpp"
#include "rerank_common.hpp"

namespace pr {
namespace {

constexpr int PG_SOLVE = 1024;               // lanes of the one workgroup that runs the inner solve
constexpr double PG_SMALL = 1e-4;            // the small-angle branch of log, its Jacobian and exp: theta < PG_SMALL takes the series

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ bool fin(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }       // false for NaN and Inf

// ------------------------------------------------------------------------------------------------ the log
__global__ __launch_bounds__(128) void posegraph_add_kernel(PoseGraphView v, const int* __restrict__ idx, const double* __restrict__ T,
                                                            const unsigned char* __restrict__ accepted, const int* __restrict__ query_row,
                                                            int k, double w_rot, double w_trans, int* __restrict__ info) {
  __shared__ int ok[POSEGRAPH_MAX_K];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;                                   // k <= 128 = the block
  const int e0 = clampi(v.state[0], v.edge_capacity);            // a scribbled count never forms an address
  int flags = v.state[1] & POSEGRAPH_OVERFLOW;
  const int row = query_row[0];
  bool mine = false;
  if (tid < k && row >= 0) {
    mine = accepted[tid] != 0 && idx[tid] >= 0 && idx[tid] != row;
    for (int c = 0; c < 12; c++) mine = mine && fin(T[(size_t)tid * 12 + c]);
  }
  ok[tid] = mine ? 1 : 0;
  __syncthreads();                                               // every thread has read state
  int before = 0, total = 0;
  for (int q = 0; q < POSEGRAPH_MAX_K; q++) { before += q < tid ? ok[q] : 0; total += ok[q]; }
  const int room = v.edge_capacity - e0, stored = total < room ? total : room;
  if (mine && before < room) {                                   // row e0 + before < edge_capacity
    const size_t e = (size_t)e0 + before;
    v.edge_ij[e * 2] = idx[tid]; v.edge_ij[e * 2 + 1] = row;
    for (int c = 0; c < 12; c++) v.edge_Z[e * 12 + c] = T[(size_t)tid * 12 + c];
    v.edge_w[e * 2] = w_rot; v.edge_w[e * 2 + 1] = w_trans;
  }
  if (tid == 0) {
    if (row >= 0) {
      if (total > room) flags |= POSEGRAPH_OVERFLOW;
      v.state[0] = e0 + stored;
      v.state[1] = flags;
    }
    info[0] = stored; info[1] = stored > 0 ? e0 : -1; info[2] = e0 + stored; info[3] = flags;
  }
}

// posegraph_add_kernel's rule slot for slot with (w_rot, w_trans) = w[p] read from device memory (pr_reginfo's d_w); a slot is logged
// only if both of its weights are finite and >= 0
__global__ __launch_bounds__(128) void posegraph_add_weighted_kernel(PoseGraphView v, const int* __restrict__ idx, const double* __restrict__ T,
                                                                     const unsigned char* __restrict__ accepted, const int* __restrict__ query_row,
                                                                     int k, const double* __restrict__ w, int* __restrict__ info) {
  __shared__ int ok[POSEGRAPH_MAX_K];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;                                   // k <= 128 = the block
  const int e0 = clampi(v.state[0], v.edge_capacity);            // a scribbled count never forms an address
  int flags = v.state[1] & POSEGRAPH_OVERFLOW;
  const int row = query_row[0];
  bool mine = false;
  double wr = 0.0, wt = 0.0;
  if (tid < k && row >= 0) {
    mine = accepted[tid] != 0 && idx[tid] >= 0 && idx[tid] != row;
    for (int c = 0; c < 12; c++) mine = mine && fin(T[(size_t)tid * 12 + c]);
    wr = w[2 * (size_t)tid]; wt = w[2 * (size_t)tid + 1];
    mine = mine && fin(wr) && fin(wt) && wr >= 0.0 && wt >= 0.0;
  }
  ok[tid] = mine ? 1 : 0;
  __syncthreads();                                               // every thread has read state
  int before = 0, total = 0;
  for (int q = 0; q < POSEGRAPH_MAX_K; q++) { before += q < tid ? ok[q] : 0; total += ok[q]; }
  const int room = v.edge_capacity - e0, stored = total < room ? total : room;
  if (mine && before < room) {                                   // row e0 + before < edge_capacity
    const size_t e = (size_t)e0 + before;
    v.edge_ij[e * 2] = idx[tid]; v.edge_ij[e * 2 + 1] = row;
    for (int c = 0; c < 12; c++) v.edge_Z[e * 12 + c] = T[(size_t)tid * 12 + c];
    v.edge_w[e * 2] = wr; v.edge_w[e * 2 + 1] = wt;
  }
  if (tid == 0) {
    if (row >= 0) {
      if (total > room) flags |= POSEGRAPH_OVERFLOW;
      v.state[0] = e0 + stored;
      v.state[1] = flags;
    }
    info[0] = stored; info[1] = stored > 0 ? e0 : -1; info[2] = e0 + stored; info[3] = flags;
  }
}

#include "posegraph_batch.hpp"                                   // posegraph_add_batch_kernel (pr_posegraphb_add_dev)

// ------------------------------------------------------------------------------------------------ 3 x 3 helpers (row-major)
__device__ __forceinline__ void mul33(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void mul33nt(const double* A, const double* B, double* C) {        // A B^T
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}
__device__ __forceinline__ void mul33tn(const double* A, const double* B, double* C) {        // A^T B
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
__device__ __forceinline__ void mv3(const double* A, const double* x, double* y) {            // A x
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
__device__ __forceinline__ void mtv3(const double* A, const double* x, double* y) {           // A^T x
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = A[r] * x[0] + A[3 + r] * x[1] + A[6 + r] * x[2];
}
__device__ __forceinline__ void skew(const double* t, double* K) {
  K[0] = 0.0; K[1] = -t[2]; K[2] = t[1];
  K[3] = t[2]; K[4] = 0.0; K[5] = -t[0];
  K[6] = -t[1]; K[7] = t[0]; K[8] = 0.0;
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
// Q = Pi Pj^-1: Rq = Ri Rj^T, tq = ti - Rq tj
__device__ __forceinline__ void rel_pose(const double* Pi, const double* Pj, double* Rq, double* tq) {
  double Ri[9], ti[3], Rj[9], tj[3], y[3];
  load_pose(Pi, Ri, ti); load_pose(Pj, Rj, tj);
  mul33nt(Ri, Rj, Rq);
  mv3(Rq, tj, y);
  tq[0] = ti[0] - y[0]; tq[1] = ti[1] - y[1]; tq[2] = ti[2] - y[2];
}

__device__ __forceinline__ void slot_nodes(const PoseGraphView& v, int s, int& i, int& j) {
  if (s < v.node_capacity - 1) { i = s; j = s + 1; }
  else { const size_t l = (size_t)(s - (v.node_capacity - 1)); i = v.edge_ij[2 * l]; j = v.edge_ij[2 * l + 1]; }
}

// ------------------------------------------------------------------------------------------------ prepare
// brk: NULL, or [node_capacity] i32 where brk[r] != 0 says that row r begins another drive (pr_session): odometry slot r - 1 is no edge
__global__ __launch_bounds__(256) void posegraph_prepare_kernel(PoseGraphView v, const double* poses_in, const int* __restrict__ n_dev,
                                                                const int* __restrict__ brk) {
  __shared__ int part[256];
  __shared__ double red[4];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x, NC = v.node_capacity, odo = NC - 1;
  const int n = clampi(n_dev[0], NC), E = clampi(v.state[0], v.edge_capacity);
  for (int a = tid; a < NC; a += 256) {
    bool f = a < n;
    if (a < n)
      for (int c = 0; c < 12; c++) { const double x = poses_in[(size_t)a * 12 + c]; v.X[(size_t)a * 12 + c] = x; f = f && fin(x); }
    v.finite[a] = f ? 1 : 0;
    v.deg[a] = 0;
  }
  __syncthreads();
  double used = 0.0, used_logged = 0.0;
  for (int s = tid; s < odo; s += 256) {                         // odometry slots: Z from the input poses, before anything moves
    const bool ok = s + 1 < n && v.finite[s] && v.finite[s + 1] && !(brk && brk[s + 1]);        // s + 1 < n <= node_capacity
    if (ok) {
      double Rq[9], tq[3];
      rel_pose(v.X + (size_t)s * 12, v.X + (size_t)(s + 1) * 12, Rq, tq);
      store_pose(v.zodo + (size_t)s * 12, Rq, tq);
      used += 1.0;
    }
    v.valid[s] = ok ? 1 : 0;
  }
  for (int l = tid; l < v.edge_capacity; l += 256) {             // logged slots
    bool ok = l < E;
    if (ok) {
      const int i = v.edge_ij[2 * (size_t)l], j = v.edge_ij[2 * (size_t)l + 1];
      ok = i >= 0 && i < n && j >= 0 && j < n && i != j;
      if (ok) ok = v.finite[i] && v.finite[j];
      for (int c = 0; c < 12; c++) ok = ok && fin(v.edge_Z[(size_t)l * 12 + c]);
      ok = ok && fin(v.edge_w[2 * (size_t)l]) && fin(v.edge_w[2 * (size_t)l + 1]);
      if (ok) { atomicAdd(&v.deg[i], 1); atomicAdd(&v.deg[j], 1); used_logged += 1.0; }
    }
    v.valid[odo + l] = ok ? 1 : 0;
  }
  __syncthreads();
  // exclusive scan of deg: a contiguous chunk per lane
  const int chunk = (NC + 255) / 256, a0 = tid * chunk, a1 = a0 + chunk < NC ? a0 + chunk : NC;
  int sum = 0;
  for (int a = a0; a < a1; a++) sum += v.deg[a];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 256; t++) { const int d = part[t]; part[t] = run; run += d; }
    v.inc_off[NC] = run;                                         // <= 2 E <= 2 edge_capacity
  }
  __syncthreads();
  int run = part[tid];
  for (int a = a0; a < a1; a++) { v.inc_off[a] = run; v.cursor[a] = run; run += v.deg[a]; }
  __syncthreads();
  for (int l = tid; l < E; l += 256) {
    if (!v.valid[odo + l]) continue;
    const int i = v.edge_ij[2 * (size_t)l], j = v.edge_ij[2 * (size_t)l + 1];
    v.inc_raw[atomicAdd(&v.cursor[i], 1)] = 2 * l;
    v.inc_raw[atomicAdd(&v.cursor[j], 1)] = 2 * l + 1;
  }
  __syncthreads();
  // every node's list into log order by ranking, a lane per entry: an entry's place is the number of smaller keys in its node's
  // segment (the keys 2 l + side of one node are distinct) - O(degree) per entry, so a node that carries many edges is shared by lanes
  const int total = v.inc_off[NC];
  for (int q = tid; q < total; q += 256) {
    const int key = v.inc_raw[q], a = v.edge_ij[2 * (size_t)(key >> 1) + (key & 1)];       // the node whose segment holds entry q
    const int b = v.inc_off[a], e = b + v.deg[a];
    int rank = 0;
    for (int w = b; w < e; w++) rank += v.inc_raw[w] < key ? 1 : 0;
    v.inc[b + rank] = key;
  }
  const double UL = block_sum256(used_logged, red, tid), U = block_sum256(used, red, tid) + UL;
  if (tid == 0) { v.ctl[0] = n; v.ctl[1] = E; v.ctl[2] = (int)U; v.ctl[3] = (int)UL; }
}

// without a logged edge in use (or under two nodes) there is nothing to relax: the odometry edges have zero residual by construction
__device__ __forceinline__ bool pg_active(const PoseGraphView& v) { return v.ctl[0] >= 2 && v.ctl[3] > 0; }

// ------------------------------------------------------------------------------------------------ linearize
__global__ __launch_bounds__(256) void posegraph_linearize_kernel(PoseGraphView v, double w_odo_rot, double w_odo_trans) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= v.S || !pg_active(v) || !v.valid[s]) return;
  const int odo = v.node_capacity - 1;
  int i, j;
  slot_nodes(v, s, i, j);
  const double* Zp = s < odo ? v.zodo + (size_t)s * 12 : v.edge_Z + (size_t)(s - odo) * 12;
  const double wr = s < odo ? w_odo_rot : v.edge_w[2 * (size_t)(s - odo)], wt = s < odo ? w_odo_trans : v.edge_w[2 * (size_t)(s - odo) + 1];
  double Rq[9], tq[3], Rz[9], tz[3], RE[9], tE[3], d[3];
  rel_pose(v.X + (size_t)i * 12, v.X + (size_t)j * 12, Rq, tq);
  load_pose(Zp, Rz, tz);
  mul33tn(Rz, Rq, RE);                                           // E = Z^-1 Q: RE = Rz^T Rq, tE = Rz^T (tq - tz)
  d[0] = tq[0] - tz[0]; d[1] = tq[1] - tz[1]; d[2] = tq[2] - tz[2];
  mtv3(Rz, d, tE);
  // log_SO3: vv = sin(theta) axis, c = cos(theta), theta = atan2(|vv|, c); phi = theta / sin(theta) vv
  double vv[3] = {0.5 * (RE[7] - RE[5]), 0.5 * (RE[2] - RE[6]), 0.5 * (RE[3] - RE[1])};
  const double sn = sqrt(vv[0] * vv[0] + vv[1] * vv[1] + vv[2] * vv[2]), cs = 0.5 * (RE[0] + RE[4] + RE[8] - 1.0);
  const double th = atan2(sn, cs);
  double kf, cf;
  if (th < PG_SMALL) { kf = 1.0 + th * th / 6.0; cf = 1.0 / 12.0 + th * th / 720.0; }
  else { kf = th / sn; cf = 1.0 / (th * th) - (1.0 + cs) / (2.0 * th * sn); }
  const double phi[3] = {kf * vv[0], kf * vv[1], kf * vv[2]};
  const double p2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  double Jl[9], K[9];                                            // the inverse left Jacobian: I - [phi]x / 2 + cf [phi]x^2
  skew(phi, K);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Jl[3 * r + c] = (r == c ? 1.0 : 0.0) - 0.5 * K[3 * r + c] + cf * (phi[r] * phi[c] - (r == c ? p2 : 0.0));
  double* J = v.jac + (size_t)s * PG_BLOCKS;
  double M[9], Kt[9];
  mul33nt(Jl, Rz, M);                                            // Arw = Jl Rz^T
#pragma unroll
  for (int c = 0; c < 9; c++) J[c] = M[c];
  skew(tq, Kt);
  mul33tn(Rz, Kt, M);                                            // Atw = -Rz^T [tq]x
#pragma unroll
  for (int c = 0; c < 9; c++) J[9 + c] = -M[c];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) J[18 + 3 * r + c] = Rz[3 * c + r];                             // Atv = Rz^T
  mul33(Jl, RE, M);                                              // Brw = -Jl RE
#pragma unroll
  for (int c = 0; c < 9; c++) { J[27 + c] = -M[c]; J[36 + c] = -RE[c]; }                       // Btv = -RE
  double* rs = v.res + (size_t)s * 6;
  rs[0] = phi[0]; rs[1] = phi[1]; rs[2] = phi[2]; rs[3] = tE[0]; rs[4] = tE[1]; rs[5] = tE[2];
  v.wgt[2 * (size_t)s] = wr; v.wgt[2 * (size_t)s + 1] = wt;
  v.cost[s] = wr * p2 + wt * (tE[0] * tE[0] + tE[1] * tE[1] + tE[2] * tE[2]);
}

// ------------------------------------------------------------------------------------------------ blocks
// one edge's share of node a's gradient and diagonal block.  side 0: a is the edge's i (J = [Arw 0; Atw Atv]); side 1: its j (J = [Brw 0; 0 Btv])
__device__ __forceinline__ void block_visit(const PoseGraphView& v, int s, int side, double* g, double (*D)[6]) {
  if (!v.valid[s]) return;
  const double* J = v.jac + (size_t)s * PG_BLOCKS;
  const double* rs = v.res + (size_t)s * 6;
  const double wr = v.wgt[2 * (size_t)s], wt = v.wgt[2 * (size_t)s + 1];
  double Jrw[9], Jtv[9], y[3];
#pragma unroll
  for (int c = 0; c < 9; c++) { Jrw[c] = J[(side ? 27 : 0) + c]; Jtv[c] = J[(side ? 36 : 18) + c]; }
  const double rr[3] = {wr * rs[0], wr * rs[1], wr * rs[2]}, rt[3] = {wt * rs[3], wt * rs[4], wt * rs[5]};
  double M[9];
  mtv3(Jrw, rr, y); g[0] -= y[0]; g[1] -= y[1]; g[2] -= y[2];
  mtv3(Jtv, rt, y); g[3] -= y[0]; g[4] -= y[1]; g[5] -= y[2];
  mul33tn(Jrw, Jrw, M);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) D[r][c] += wr * M[3 * r + c];
  mul33tn(Jtv, Jtv, M);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) D[3 + r][3 + c] += wt * M[3 * r + c];
  if (side == 0) {
    double Jtw[9];
#pragma unroll
    for (int c = 0; c < 9; c++) Jtw[c] = J[9 + c];
    mtv3(Jtw, rt, y); g[0] -= y[0]; g[1] -= y[1]; g[2] -= y[2];
    mul33tn(Jtw, Jtw, M);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) D[r][c] += wt * M[3 * r + c];
    mul33tn(Jtw, Jtv, M);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) { D[r][3 + c] += wt * M[3 * r + c]; D[3 + c][r] += wt * M[3 * r + c]; }
  }
}

__global__ __launch_bounds__(256) void posegraph_blocks_kernel(PoseGraphView v, double lambda) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (!pg_active(v) || a >= v.ctl[0]) return;
  const int odo = v.node_capacity - 1;
  double g[6], D[6][6], I[6][6];
#pragma unroll
  for (int r = 0; r < 6; r++) {
    g[r] = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) { D[r][c] = r == c ? lambda : 0.0; I[r][c] = r == c ? 1.0 : 0.0; }
  }
  bool ok = true;
  if (a > 0) {                                                   // node 0 is the gauge: zero gradient, identity block
    block_visit(v, a - 1, 1, g, D);
    if (a < odo) block_visit(v, a, 0, g, D);
    const int b = v.inc_off[a], e = b + v.deg[a];
    for (int q = b; q < e; q++) { const int w = v.inc[q]; block_visit(v, odo + (w >> 1), w & 1, g, D); }
    // Gauss-Jordan without pivoting (the block is symmetric positive definite, or the node has no weighted edge and lambda = 0:
    // a pivot that is not positive makes the inverse the ZERO block, so the node does not move)
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double piv = D[k][k];
      ok = ok && piv > 0.0 && fin(piv);
      const double ip = 1.0 / piv;
#pragma unroll
      for (int c = 0; c < 6; c++) { D[k][c] *= ip; I[k][c] *= ip; }
#pragma unroll
      for (int r = 0; r < 6; r++) {
        if (r == k) continue;
        const double f = D[r][k];
#pragma unroll
        for (int c = 0; c < 6; c++) { D[r][c] -= f * D[k][c]; I[r][c] -= f * I[k][c]; }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 6; r++) {
    v.g[(size_t)a * 6 + r] = g[r];
#pragma unroll
    for (int c = 0; c < 6; c++) v.dinv[(size_t)a * 36 + 6 * r + c] = ok ? I[r][c] : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ solve
// node a's share of J^T u of one edge
__device__ __forceinline__ void mat_visit(const PoseGraphView& v, int s, int side, double* y) {
  if (!v.valid[s]) return;
  const double* J = v.jac + (size_t)s * PG_BLOCKS;
  const double* u = v.u + (size_t)s * 6;
  const double ur[3] = {u[0], u[1], u[2]}, ut[3] = {u[3], u[4], u[5]};
  double t[3];
  mtv3(J + (side ? 27 : 0), ur, t); y[0] += t[0]; y[1] += t[1]; y[2] += t[2];
  if (side == 0) { mtv3(J + 9, ut, t); y[0] += t[0]; y[1] += t[1]; y[2] += t[2]; }
  mtv3(J + (side ? 36 : 18), ut, t); y[3] += t[0]; y[4] += t[1]; y[5] += t[2];
}

__device__ __forceinline__ void dinv_apply(const double* Di, const double* r, double* z) {
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) s += Di[6 * a + c] * r[c];
    z[a] = s;
  }
}

// block_sum256's construction for the solve workgroup's PG_SOLVE lanes: wave shuffles, then the wave partials added pairwise in a fixed tree
__device__ __forceinline__ double block_sum_solve(double v, double* red, int tid) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double t[PG_SOLVE / 64];
#pragma unroll
  for (int w = 0; w < PG_SOLVE / 64; w++) t[w] = red[w];
#pragma unroll
  for (int h = PG_SOLVE / 128; h > 0; h >>= 1)                   // block_sum256's fixed tree: neighbours first
#pragma unroll
    for (int w = 0; w < h; w++) t[w] = t[2 * w] + t[2 * w + 1];
  __syncthreads();
  return t[0];
}

__global__ __launch_bounds__(PG_SOLVE) void posegraph_solve_kernel(PoseGraphView v, int inner, double lambda, double* report_slot) {
  __shared__ double red[PG_SOLVE / 64];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  if (!pg_active(v)) {
    if (tid == 0) report_slot[0] = 0.0;
    return;
  }
  const int n = v.ctl[0], odo = v.node_capacity - 1, L = (n - 1) + v.ctl[1];      // the slots that can be edges: n - 1 odometry, ctl[1] logged
  double c = 0.0;
  for (int w = tid; w < L; w += PG_SOLVE) {
    const int s = w < n - 1 ? w : odo + (w - (n - 1));
    c += v.valid[s] ? v.cost[s] : 0.0;
  }
  const double C = block_sum_solve(c, red, tid);
  if (tid == 0) report_slot[0] = C;
  double acc = 0.0;
  for (int a = tid; a < n; a += PG_SOLVE) {
    double r[6], z[6];
#pragma unroll
    for (int e = 0; e < 6; e++) r[e] = v.g[(size_t)a * 6 + e];
    dinv_apply(v.dinv + (size_t)a * 36, r, z);
#pragma unroll
    for (int e = 0; e < 6; e++) {
      v.x[(size_t)a * 6 + e] = 0.0; v.r[(size_t)a * 6 + e] = r[e]; v.z[(size_t)a * 6 + e] = z[e]; v.p[(size_t)a * 6 + e] = z[e];
      acc += r[e] * z[e];
    }
  }
  double rz = block_sum_solve(acc, red, tid);                       // (its barriers also publish p)
  for (int it = 0; it < inner; it++) {
    for (int w = tid; w < L; w += PG_SOLVE) {                    // u = W (A p_i + B p_j)
      const int s = w < n - 1 ? w : odo + (w - (n - 1));
      if (!v.valid[s]) continue;
      int i, j;
      slot_nodes(v, s, i, j);
      const double* J = v.jac + (size_t)s * PG_BLOCKS;
      const double* pi = v.p + (size_t)i * 6;
      const double* pj = v.p + (size_t)j * 6;
      const double wi[3] = {pi[0], pi[1], pi[2]}, vi[3] = {pi[3], pi[4], pi[5]}, wj[3] = {pj[0], pj[1], pj[2]}, vj[3] = {pj[3], pj[4], pj[5]};
      double a1[3], a2[3], a3[3], a4[3], a5[3];
      mv3(J, wi, a1); mv3(J + 27, wj, a2); mv3(J + 9, wi, a3); mv3(J + 18, vi, a4); mv3(J + 36, vj, a5);
      const double wr = v.wgt[2 * (size_t)s], wt = v.wgt[2 * (size_t)s + 1];
      double* u = v.u + (size_t)s * 6;
#pragma unroll
      for (int e = 0; e < 3; e++) { u[e] = wr * (a1[e] + a2[e]); u[3 + e] = wt * ((a3[e] + a4[e]) + a5[e]); }
    }
    __syncthreads();
    acc = 0.0;
    for (int a = tid; a < n; a += PG_SOLVE) {                         // q = lambda p + J^T u, gathered in the fixed order of the blocks kernel
      double y[6];
#pragma unroll
      for (int e = 0; e < 6; e++) y[e] = a > 0 ? lambda * v.p[(size_t)a * 6 + e] : 0.0;
      if (a > 0) {
        mat_visit(v, a - 1, 1, y);
        if (a < odo) mat_visit(v, a, 0, y);
        const int b = v.inc_off[a], e1 = b + v.deg[a];
        for (int q = b; q < e1; q++) { const int w = v.inc[q]; mat_visit(v, odo + (w >> 1), w & 1, y); }
      }
#pragma unroll
      for (int e = 0; e < 6; e++) { v.q[(size_t)a * 6 + e] = y[e]; acc += v.p[(size_t)a * 6 + e] * y[e]; }
    }
    const double pq = block_sum_solve(acc, red, tid);
    const double alpha = pq > 0.0 ? rz / pq : 0.0;
    acc = 0.0;
    for (int a = tid; a < n; a += PG_SOLVE) {
      double r[6], z[6];
#pragma unroll
      for (int e = 0; e < 6; e++) {
        v.x[(size_t)a * 6 + e] += alpha * v.p[(size_t)a * 6 + e];
        r[e] = v.r[(size_t)a * 6 + e] - alpha * v.q[(size_t)a * 6 + e];
        v.r[(size_t)a * 6 + e] = r[e];
      }
      dinv_apply(v.dinv + (size_t)a * 36, r, z);
#pragma unroll
      for (int e = 0; e < 6; e++) { v.z[(size_t)a * 6 + e] = z[e]; acc += r[e] * z[e]; }
    }
    const double rzn = block_sum_solve(acc, red, tid);
    const double beta = rz > 0.0 ? rzn / rz : 0.0;
    for (int a = tid; a < n; a += PG_SOLVE)
#pragma unroll
      for (int e = 0; e < 6; e++) v.p[(size_t)a * 6 + e] = v.z[(size_t)a * 6 + e] + beta * v.p[(size_t)a * 6 + e];
    rz = rzn;
    __syncthreads();                                             // p is read by other lanes in the next product
  }
  for (int a = tid; a < n; a += PG_SOLVE) {                           // R <- exp(w) R, t <- exp(w) t + v; an exact zero step touches nothing
    if (a == 0) continue;
    double dl[6];
    bool any = false;
#pragma unroll
    for (int e = 0; e < 6; e++) { dl[e] = v.x[(size_t)a * 6 + e]; any = any || dl[e] != 0.0; }
    if (!any) continue;
    const double t2 = dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2], th = sqrt(t2);
    double ka, kb;
    if (th < PG_SMALL) { ka = 1.0 - t2 / 6.0; kb = 0.5 - t2 / 24.0; }
    else { ka = sin(th) / th; kb = (1.0 - cos(th)) / t2; }
    double K[9], Ex[9], R[9], t[3], R2[9], t2v[3];
    skew(dl, K);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int cc = 0; cc < 3; cc++) Ex[3 * r + cc] = (r == cc ? 1.0 : 0.0) + ka * K[3 * r + cc] + kb * (dl[r] * dl[cc] - (r == cc ? t2 : 0.0));
    load_pose(v.X + (size_t)a * 12, R, t);
    mul33(Ex, R, R2);
    mv3(Ex, t, t2v);
    t2v[0] += dl[3]; t2v[1] += dl[4]; t2v[2] += dl[5];
    store_pose(v.X + (size_t)a * 12, R2, t2v);
  }
}

// ------------------------------------------------------------------------------------------------ finish
__global__ __launch_bounds__(256) void posegraph_finish_kernel(PoseGraphView v, double* poses_out, double* report_tail) {
  __shared__ double red[4];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x, n = v.ctl[0];
  double c = 0.0;
  if (pg_active(v)) {
    const int odo = v.node_capacity - 1, L = (n - 1) + v.ctl[1];
    for (int w = tid; w < L; w += 256) {
      const int s = w < n - 1 ? w : odo + (w - (n - 1));
      c += v.valid[s] ? v.cost[s] : 0.0;
    }
  }
  const double C = block_sum256(c, red, tid);
  if (tid == 0) { report_tail[0] = C; report_tail[1] = (double)v.ctl[2]; }
  for (int q = tid; q < n * 12; q += 256) poses_out[q] = v.X[q];                               // rows >= n are not written
}

}  // namespace

void launch_posegraph_add(hipStream_t st, const PoseGraphView& v, const int* idx, const double* T, const unsigned char* accepted,
                          const int* query_row, int k, double w_rot, double w_trans, int* info) {
  hipLaunchKernelGGL(posegraph_add_kernel, dim3(1), dim3(128), 0, st, v, idx, T, accepted, query_row, k, w_rot, w_trans, info);
}

void launch_posegraph_add_weighted(hipStream_t st, const PoseGraphView& v, const int* idx, const double* T, const unsigned char* accepted,
                                   const int* query_row, int k, const double* w, int* info) {
  hipLaunchKernelGGL(posegraph_add_weighted_kernel, dim3(1), dim3(128), 0, st, v, idx, T, accepted, query_row, k, w, info);
}

void launch_posegraph_add_batch(hipStream_t st, const PoseGraphView& v, const int* i, const int* j, const double* T, const unsigned char* accepted,
                                const double* w, double w_rot, double w_trans, int c, int* info) {
  hipLaunchKernelGGL(posegraph_add_batch_kernel, dim3(1), dim3(256), 0, st, v, i, j, T, accepted, w, w_rot, w_trans, c, info);
}

void launch_posegraph_relax(hipStream_t st, const PoseGraphView& v, const double* poses_in, const int* n, const PoseGraphParams& prm,
                            double* poses_out, double* report, const int* brk) {
  const dim3 one(1), blk(256), slots((v.S + 255) / 256), nodes((v.node_capacity + 255) / 256);
  hipLaunchKernelGGL(posegraph_prepare_kernel, one, blk, 0, st, v, poses_in, n, brk);
  for (int s = 0; s < prm.outer; s++) {
    hipLaunchKernelGGL(posegraph_linearize_kernel, slots, blk, 0, st, v, prm.w_odo_rot, prm.w_odo_trans);
    hipLaunchKernelGGL(posegraph_blocks_kernel, nodes, blk, 0, st, v, prm.lambda);
    hipLaunchKernelGGL(posegraph_solve_kernel, one, dim3(PG_SOLVE), 0, st, v, prm.inner, prm.lambda, report + s);
  }
  hipLaunchKernelGGL(posegraph_linearize_kernel, slots, blk, 0, st, v, prm.w_odo_rot, prm.w_odo_trans);
  hipLaunchKernelGGL(posegraph_finish_kernel, one, blk, 0, st, v, poses_out, report + prm.outer);
}

}  // namespace pr
