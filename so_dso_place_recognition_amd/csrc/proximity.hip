// proximity.hip — loop-closure candidates from the poses themselves (no reference counterpart): for every query row the
// earlier keyframes whose camera centre lies within a drift-aware radius and whose viewing axis agrees, one per bucket of `stride` rows,
// the k nearest of those, with the seed T0 = P_i P_q^-1 and the pair lists pr_icp_pairs_dev takes.  The rule is in
// include/place_recognition.h and restated in tests/proximity_np.py; the device equals it bit for bit (fp64, no contraction, + x sqrt
// only).  Every grid depends on the create sizes only and every count is read from device memory, so one captured run serves every count.
//   prepare   a lane per row: validity, camera centre, viewing axis; one lane clears info and forms the flags
//   prefix    one workgroup: the path length over the valid rows in 256 blocks of C rows - the steps and the running sum of a block,
//             then the blocks' totals summed in block order (trajeval's order)
//   search    a workgroup per (tile of 16 query rows, run): the DB rows 0 .. q_max - min_gap of the tile, cut into `runs` runs at bucket
//             borders, walked in slabs of 256 rows staged through LDS; a wave keeps the lists of 4 rows in its registers, lane t
//             holding entry t, and carries every row's open bucket across slab borders
//   emit      a wave per query row: the runs' lists merged by the same insertion, the known test against the log, seeds, pair lists,
//             counts (integer atomics)
// No floating-point atomics, no workgroup waits for another, every loop is bounded by a create size.  Plain C++, vector stores only.
#include "proximity.hpp"
#include "trajeval.hpp"

namespace pr {
namespace {

using namespace traj;

constexpr int T = PROX_T;
constexpr int IMAX = 0x7fffffff;
constexpr int WAVES = PROX_T / 64;
static_assert(WAVES * PROX_RPW == PROX_ROWS && PROX_COLS == PROX_T && PROX_MAX_K <= 64, "the tile");

struct Range { int n, mq; long long q0; };

__device__ __forceinline__ Range read_range(const ProxView& v, const ProxIn& in) {
  Range g;
  g.n = clampi(in.n[0], v.node_capacity);                        // a scribbled count never forms an address
  g.q0 = in.qrange[0];
  g.mq = clampi(in.qrange[1], v.query_capacity);
  return g;
}

// (d, i) into the ascending list whose entry t lane t holds; order: d2, then the row
__device__ __forceinline__ void insert(double& ld, int& li, double d, int i, int lane) {
  const bool less = ld < d || (ld == d && li < i);
  const double ud = __shfl_up(ld, 1);
  const int ui = __shfl_up(li, 1);
  const int below = __shfl_up(less ? 1 : 0, 1);                  // every lane takes part in the shuffle: no lane reads an idle one
  const int uless = lane == 0 ? 1 : below;
  if (!less) {
    ld = uless ? d : ud;
    li = uless ? i : ui;
  }
}

// ------------------------------------------------------------------------------------------------ prepare
__global__ __launch_bounds__(T) void prox_prepare_kernel(ProxView v, ProxIn in, ProxOut out) {
  const int i = blockIdx.x * T + threadIdx.x;
  const Range g = read_range(v, in);
  if (i == 0) {
    int flags = in.qrange[1] != g.mq ? PROX_QRANGE_CLAMPED : 0;
    if (g.mq > 0 && (g.q0 < 0 || g.q0 + g.mq - 1 > (long long)g.n - 1)) flags |= PROX_QRANGE_CLAMPED;
    out.info[0] = 0; out.info[1] = 0; out.info[2] = 0; out.info[3] = flags;
  }
  if (i >= v.node_capacity) return;
  bool ok = i < g.n;
  const double* p = in.poses + (size_t)i * 12;
  if (ok)
    for (int c = 0; c < 12; c++) ok = ok && fin(p[c]);
  double c3[3] = {0.0, 0.0, 0.0}, a3[3] = {0.0, 0.0, 0.0};
  if (ok) {
    double R[9], t[3], y[3];
    load_pose(p, R, t);
    mtv3(R, t, y);
    c3[0] = -y[0]; c3[1] = -y[1]; c3[2] = -y[2];
    a3[0] = R[6]; a3[1] = R[7]; a3[2] = R[8];
  }
  v.valid[i] = ok ? 1 : 0;
  for (int c = 0; c < 3; c++) { v.cen[(size_t)i * 3 + c] = c3[c]; v.axis[(size_t)i * 3 + c] = a3[c]; }
}

// ------------------------------------------------------------------------------------------------ the path length
__global__ __launch_bounds__(T) void prox_prefix_kernel(ProxView v) {
  __shared__ double lds[T];
  __shared__ int ilds[T];
  const int tid = threadIdx.x, cap = v.node_capacity;
  const int C = (cap + T - 1) / T;
  const long long b0 = (long long)tid * C;
  const int i0 = b0 < cap ? (int)b0 : cap, i1 = i0 + C < cap ? i0 + C : cap;
  int last = -1;
  for (int i = i0; i < i1; i++)
    if (v.valid[i]) last = i;
  ilds[tid] = last;
  __syncthreads();
  if (tid == 0) {                                                // the last valid row in front of every block
    int run = -1;
    for (int k = 0; k < T; k++) { const int x = ilds[k]; ilds[k] = run; if (x >= 0) run = x; }
  }
  __syncthreads();
  int prev = ilds[tid];
  double w = 0.0;
  for (int i = i0; i < i1; i++) {
    if (v.valid[i]) {
      if (prev >= 0) {
        const double* a = v.cen + (size_t)i * 3;
        const double* c = v.cen + (size_t)prev * 3;
        w += norm3(a[0] - c[0], a[1] - c[1], a[2] - c[2]);
      }
      prev = i;
    }
    v.s[i] = w;
  }
  lds[tid] = w;
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int k = 0; k < T; k++) { const double x = lds[k]; lds[k] = run; run += x; }
  }
  __syncthreads();
  const double base = lds[tid];
  for (int i = i0; i < i1; i++) v.s[i] = base + v.s[i];
}

// ------------------------------------------------------------------------------------------------ the search
__global__ __launch_bounds__(T) void prox_search_kernel(ProxView v, ProxIn in, ProxParams prm) {
  __shared__ double s_c[PROX_COLS * 3];
  __shared__ double s_a[PROX_COLS * 3];
  __shared__ double s_s[PROX_COLS];
  __shared__ int s_v[PROX_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, run = blockIdx.y, runs = v.runs;
  const Range g = read_range(v, in);
  const int r_first = tile * PROX_ROWS;
  // the DB rows of this tile: 0 .. hi - 1 with hi = q_max - min_gap + 1, q_max the tile's largest query row below n
  long long hi = 0;
  if (r_first < g.mq) {
    const int r_end = r_first + PROX_ROWS < g.mq ? r_first + PROX_ROWS : g.mq;
    long long q_max = g.q0 + r_end - 1;
    if (q_max > (long long)g.n - 1) q_max = (long long)g.n - 1;
    hi = q_max - prm.min_gap + 1;
    if (hi < 0) hi = 0;
    if (hi > g.n) hi = g.n;
  }
  // this run: whole buckets, so no bucket is ever split between two lists
  const long long stride = prm.stride;
  const long long NB = (hi + stride - 1) / stride, BPR = (NB + runs - 1) / runs;
  long long lo_row = (long long)run * BPR * stride, end_row = ((long long)run + 1) * BPR * stride;
  if (lo_row > hi) lo_row = hi;
  if (end_row > hi) end_row = hi;

  double cq[PROX_RPW][3], aq[PROX_RPW][3], sq[PROX_RPW];
  long long q[PROX_RPW];
  bool searched[PROX_RPW];
  double ld[PROX_RPW], rd[PROX_RPW];
  int li[PROX_RPW], ri[PROX_RPW], ob[PROX_RPW];
#pragma unroll
  for (int j = 0; j < PROX_RPW; j++) {
    const int r = r_first + wave * PROX_RPW + j;
    q[j] = g.q0 + r;
    searched[j] = r < g.mq && q[j] >= 0 && q[j] < g.n;
    if (searched[j]) searched[j] = v.valid[q[j]] != 0;           // 0 <= q < n <= node_capacity
    for (int c = 0; c < 3; c++) {
      cq[j][c] = searched[j] ? v.cen[(size_t)q[j] * 3 + c] : 0.0;
      aq[j][c] = searched[j] ? v.axis[(size_t)q[j] * 3 + c] : 0.0;
    }
    sq[j] = searched[j] ? v.s[q[j]] : 0.0;
    ld[j] = __builtin_inf(); li[j] = IMAX; ob[j] = -1; rd[j] = 0.0; ri[j] = 0;
  }
  const bool heading = prm.cos_min > -1.0;

  for (long long c0 = lo_row; c0 < end_row; c0 += PROX_COLS) {   // block-uniform bounds
    __syncthreads();                                             // the slab before has been read
    {
      const long long i = c0 + tid;
      const bool in_run = i < end_row;                           // end_row <= n <= node_capacity
      s_v[tid] = in_run ? v.valid[i] : 0;
      for (int c = 0; c < 3; c++) {
        s_c[tid * 3 + c] = in_run ? v.cen[(size_t)i * 3 + c] : 0.0;
        s_a[tid * 3 + c] = in_run ? v.axis[(size_t)i * 3 + c] : 0.0;
      }
      s_s[tid] = in_run ? v.s[i] : 0.0;
    }
    __syncthreads();
    for (int ch = 0; ch < PROX_COLS / 64; ch++) {
      const int col = ch * 64 + lane;
      const long long i = c0 + col;
      const int vi = s_v[col];
      const double ci0 = s_c[col * 3], ci1 = s_c[col * 3 + 1], ci2 = s_c[col * 3 + 2], si = s_s[col];
      const double ai0 = s_a[col * 3], ai1 = s_a[col * 3 + 1], ai2 = s_a[col * 3 + 2];
#pragma unroll
      for (int j = 0; j < PROX_RPW; j++) {
        bool cand = searched[j] && vi != 0 && i + prm.min_gap <= q[j];
        const double dx0 = ci0 - cq[j][0], dx1 = ci1 - cq[j][1], dx2 = ci2 - cq[j][2];
        const double d2 = (dx0 * dx0 + dx1 * dx1) + dx2 * dx2;
        double rad = prm.radius + prm.growth * (sq[j] - si);
        if (!(rad < prm.radius_max)) rad = prm.radius_max;
        cand = cand && d2 < rad * rad;
        if (heading) cand = cand && (ai0 * aq[j][0] + ai1 * aq[j][1]) + ai2 * aq[j][2] >= prm.cos_min;
        unsigned long long mask = __ballot(cand);
        while (mask) {                                           // the candidates of this chunk in ascending row order
          const int l = __builtin_ctzll(mask);
          mask &= mask - 1;
          const double d = __shfl(d2, l);
          const int row = (int)(c0 + ch * 64 + l);
          const int b = (int)(row / stride);
          if (b != ob[j]) {
            if (ob[j] >= 0) insert(ld[j], li[j], rd[j], ri[j], lane);
            ob[j] = b; rd[j] = d; ri[j] = row;
          } else if (d < rd[j]) { rd[j] = d; ri[j] = row; }      // the lowest row on a tie: the walk ascends
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < PROX_RPW; j++) {
    if (ob[j] >= 0) insert(ld[j], li[j], rd[j], ri[j], lane);
    const int r = r_first + wave * PROX_RPW + j;
    if (searched[j] && lane < v.k_max) {                         // r < mq <= query_capacity
      const size_t o = ((size_t)r * runs + run) * v.k_max + lane;
      v.part_d2[o] = ld[j]; v.part_idx[o] = li[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------ merge, known test, seeds, counts
__global__ __launch_bounds__(T) void prox_emit_kernel(ProxView v, ProxIn in, ProxParams prm, ProxOut out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * WAVES + wave, k = prm.k;
  if (r >= v.query_capacity) return;                             // a whole wave; the kernel has no barrier
  const Range g = read_range(v, in);
  const long long q = g.q0 + r;
  bool searched = r < g.mq && q >= 0 && q < g.n;
  if (searched) searched = v.valid[q] != 0;
  double ld = __builtin_inf();
  int li = IMAX;
  if (searched) {
    const size_t o = (size_t)r * v.runs * v.k_max;
    if (lane < v.k_max) { ld = v.part_d2[o + lane]; li = v.part_idx[o + lane]; }
    for (int run = 1; run < v.runs; run++)
      for (int e = 0; e < v.k_max; e++) {
        const int i = v.part_idx[o + (size_t)run * v.k_max + e];
        if (i == IMAX) break;                                    // a list is ascending: nothing behind an empty entry
        insert(ld, li, v.part_d2[o + (size_t)run * v.k_max + e], i, lane);
      }
  }
  const int idx = li == IMAX ? -1 : li;
  const bool filled = lane < k && idx >= 0;
  unsigned known_mask = 0;
  if (in.e_ij != nullptr && __ballot(filled)) {
    const int E = clampi(in.e_state[0], in.log_edge_capacity);
    const long long w = prm.known_window;
    for (int a0 = 0; a0 < E; a0 += 64) {
      const int a = a0 + lane;
      bool near_q = false;
      long long lo = 0;
      if (a < E) {
        const int ei = in.e_ij[2 * (size_t)a], ej = in.e_ij[2 * (size_t)a + 1];
        lo = ei < ej ? ei : ej;
        const long long hi = ei < ej ? ej : ei, dq = hi - q;
        near_q = ei >= 0 && ej >= 0 && (dq < 0 ? -dq : dq) <= w;
      }
      if (!__ballot(near_q)) continue;
      for (int t = 0; t < k; t++) {
        const int it = __shfl(idx, t);
        if (it < 0) break;                                       // the filled slots come first
        const long long di = lo - it;
        if (__ballot(near_q && (di < 0 ? -di : di) <= w)) known_mask |= 1u << t;
      }
    }
  }
  const bool known = filled && ((known_mask >> lane) & 1u) != 0;
  if (lane < k) {
    const size_t o = (size_t)r * k + lane;
    out.idx[o] = idx;
    out.d2[o] = ld;
    double RT[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tT[3] = {0.0, 0.0, 0.0};
    if (filled && !known) {                                      // P_i P_q^-1: idx and q are valid rows < n
      double Ri[9], ti[3], Rq[9], tq[3], Rv[9], tv[3];
      load_pose(in.poses + (size_t)idx * 12, Ri, ti);
      load_pose(in.poses + (size_t)q * 12, Rq, tq);
      rigid_inv(Rq, tq, Rv, tv);
      rigid_mul(Ri, ti, Rv, tv, RT, tT);
    }
    double* To = out.T0 + o * 12;
    for (int a = 0; a < 3; a++) { To[4 * a] = RT[3 * a]; To[4 * a + 1] = RT[3 * a + 1]; To[4 * a + 2] = RT[3 * a + 2]; To[4 * a + 3] = tT[a]; }
    out.pair_src[o] = filled && !known ? (int)q : -1;
    out.pair_dst[o] = filled && !known ? idx : -1;
    if (out.known) out.known[o] = known ? 1 : 0;
  }
  const int nf = __popcll(__ballot(filled)), nk = __popcll(__ballot(known));
  if (lane == 0) {
    if (searched) atomicAdd(out.info, 1);
    if (nf) atomicAdd(out.info + 1, nf);
    if (nk) atomicAdd(out.info + 2, nk);
  }
}

}  // namespace

void launch_proximity(hipStream_t st, const ProxView& v, const ProxIn& in, const ProxParams& prm, const ProxOut& out) {
  const dim3 blk(T);
  hipLaunchKernelGGL(prox_prepare_kernel, dim3((v.node_capacity + T - 1) / T), blk, 0, st, v, in, out);
  hipLaunchKernelGGL(prox_prefix_kernel, dim3(1), blk, 0, st, v);
  hipLaunchKernelGGL(prox_search_kernel, dim3(prox_tiles(v.query_capacity), v.runs), blk, 0, st, v, in, prm);
  hipLaunchKernelGGL(prox_emit_kernel, dim3((v.query_capacity + WAVES - 1) / WAVES), blk, 0, st, v, in, prm, out);
}

}  // namespace pr
