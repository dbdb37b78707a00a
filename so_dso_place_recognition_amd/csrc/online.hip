// online.hip — the online engine (no reference counterpart): the raw signature rows of the keyframes seen so far in
// caller-owned buffers with ONE DEVICE-side count, matched exactly in fp64 and grown on the stream.  Four kinds: SC and M2DP (pr_online),
// FUSED = SC + M2DP in one selection (BASELINE config 5) and DELIGHT (pr_onlineset).  The sibling of map.hip for signatures: every grid
// depends on the create sizes only; the count and whether the push in front emitted at all are read from device memory, so one captured
// match + append serves every keyframe.  With C channels (SC 2, M2DP 2, FUSED 4, DELIGHT 1):
//   rows    NB workgroups.  Z-scored kinds: workgroup b takes entries b, b + NB, ... < count and every channel of each - the reference's
//           pair formulation (rerank_common.hpp: sc_pair_exact / m2dp_pair_exact; FUSED makes SC's calls and M2DP's, so the same bits) -
//           and ALWAYS writes its partial (entries that are not NaN, sum of d - 0.5) per channel.  DELIGHT: batches of 16 entries
//           through exact_batch (delight_exact.hpp: the text the DelightMatcher's exact rows use)
//   stats   C > 1, one workgroup: the partials in workgroup order -> mean; a second pass about that mean -> sd (N - 1, NaN left out)
//   select  one workgroup: f = 0; f += p_weight z_0; f += z_1; ... (the oracle's order), THEN +Inf under the mask (the query is row
//           `count`; a masked NaN becomes a selectable +Inf), and the k smallest by (score, index) in k sweeps; NaN is never selected.
//           DELIGHT: the distance is the score, no statistics (run_test.m:26-41), so one row is enough
//   append  one workgroup: every part to row `count`, then - behind its own barrier - ONE thread commits state and info
// No kernel waits for another workgroup: no atomics, no tickets.  Fixed-order reductions.  Plain C++, vector stores only.
#include "online.hpp"
#include "delight_exact.hpp"
#include "rerank_common.hpp"

namespace pr {
namespace {

static_assert(ONLINE_NB == ONLINESET_NB_FUSED, "online_blocks() uses one number for the three z-scored kinds");
__device__ __forceinline__ bool emitted_off(const int* emitted) { return emitted && emitted[0] == 0; }
// a scribbled state word must not turn into a row outside the buffers
__device__ __forceinline__ int online_count(const OnlineView& v) {
  const int n = v.state[0];
  return n < 0 ? 0 : (n > v.capacity ? v.capacity : n);
}
__device__ __forceinline__ bool sel_less(double av, int aj, double bv, int bj) { return av < bv || (av == bv && aj < bj); }

// The LDS of the z-scored rows kernels, at namespace scope: all three instantiations hand the pair functions the SAME two addresses, so
// the compiler knows them inside sc_pair_exact / m2dp_pair_exact.  With arrays of its own in every instantiation the SC and FUSED kernels
// need 28 and 12 more VGPRs (a wave per SIMD less each).  The M2DP kernel does not touch rows_buf: its LDS is rows_red alone, 2 048 B.
__shared__ double rows_buf[60 * 21 + 1200];
__shared__ double rows_red[256];

// q0, q1: the query's parts in the view's order (q1 only for FUSED)
template <bool SC, bool M2DP>
__global__ __launch_bounds__(256) void online_rows_kernel(OnlineView v, const double* __restrict__ q0, const double* __restrict__ q1,
                                                          const int* __restrict__ emitted, double* __restrict__ rows) {
  constexpr int C = 2 * (SC + M2DP), M = SC ? 2 : 0;             // M: the first M2DP channel
  if (emitted_off(emitted)) return;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = online_count(v);
  const double* qm = SC ? q1 : q0;
  const double* dm = v.part[SC ? 1 : 0];
  double cnt[C] = {}, sum[C] = {};
  for (int j = b; j < n; j += v.NB) {                            // j < capacity: row j of every part and of every channel of rows exists
    double d[C];
    if constexpr (SC) {
      d[0] = sc_pair_exact(q0, 0, 0, v.part[0], 0, (size_t)j * 2400, rows_buf, rows_red, tid);
      d[1] = sc_pair_exact(q0, 0, 1200, v.part[0], 0, (size_t)j * 2400 + 1200, rows_buf, rows_red, tid);
    }
    if constexpr (M2DP) {
      d[M] = m2dp_pair_exact(qm, 0, 0, dm, 0, (size_t)j * 1536, 0, rows_red, tid);
      d[M + 1] = m2dp_pair_exact(qm, 0, 0, dm, 0, (size_t)j * 1536, 1, rows_red, tid);
    }
    if (tid == 0) {                                              // (every thread holds the block-wide value)
#pragma unroll
      for (int c = 0; c < C; c++) rows[(size_t)c * v.capacity + j] = d[c];
    }
#pragma unroll
    for (int c = 0; c < C; c++)
      if (d[c] == d[c]) { cnt[c] += 1.0; sum[c] += d[c] - 0.5; }
  }
  if (tid == 0) {
    double* p = v.partial + (size_t)b * (2 * C);                 // b < NB = the grid
#pragma unroll
    for (int c = 0; c < C; c++) { p[2 * c] = cnt[c]; p[2 * c + 1] = sum[c]; }
  }
}

__global__ __launch_bounds__(256) void online_delight_rows_kernel(OnlineView v, const double* __restrict__ sig, const int* __restrict__ emitted,
                                                                  double* __restrict__ rows) {
  __shared__ XShared sh;
  __shared__ const double* pa[XB];
  __shared__ const double* pb[XB];
  __shared__ double dd[XB];
  if (emitted_off(emitted)) return;
  const int tid = threadIdx.x;
  const int n = online_count(v);
  for (int rb = blockIdx.x * XB; rb < n; rb += v.NB * XB) {      // uniform over the workgroup
    const int np = n - rb < XB ? n - rb : XB;                    // rb + np <= n <= capacity
    if (tid < XB) { pa[tid] = sig; pb[tid] = v.part[0] + (size_t)(rb + (tid < np ? tid : 0)) * 4096; }
    __syncthreads();
    exact_batch(sh, tid, np, pa, pb, dd);
    if (tid < np) rows[rb + tid] = dd[tid];
    __syncthreads();
  }
}

template <int C>
__global__ __launch_bounds__(256) void online_stats_kernel(OnlineView v, const int* __restrict__ emitted, const double* __restrict__ rows) {
  __shared__ double tot[2 * C];
  __shared__ double red[4];
  if (blockIdx.x != 0 || emitted_off(emitted)) return;
  const int tid = threadIdx.x;
  const int n = online_count(v);
  if (tid < 2 * C) {
    double s = 0.0;
    for (int b = 0; b < v.NB; b++) s += v.partial[(size_t)b * (2 * C) + tid];      // workgroup order: deterministic
    tot[tid] = s;
  }
  __syncthreads();
  for (int ch = 0; ch < C; ch++) {
    const double N = tot[2 * ch], mean = 0.5 + tot[2 * ch + 1] / N;          // no entry: 0 / 0 = NaN
    const double* r = rows + (size_t)ch * v.capacity;
    double a = 0.0, c = 0.0;
    for (int j = tid; j < n; j += 256) {
      const double d = r[j];
      if (d == d) { const double x = d - mean; a += x * x; c += x; }
    }
    const double A = block_sum256(a, red, tid), S = block_sum256(c, red, tid);
    if (tid == 0) {
      v.stats[2 * ch] = mean;
      v.stats[2 * ch + 1] = sqrt((A - S * S / N) / (N - 1.0));               // one entry: 0 / 0 = NaN
    }
  }
}

template <int C>
__global__ __launch_bounds__(256) void online_select_kernel(OnlineView v, const int* __restrict__ emitted, const double* __restrict__ rows,
                                                            int mask_width, double p_weight, int k, int* __restrict__ idx,
                                                            double* __restrict__ score) {
  __shared__ double red[4];
  __shared__ int ired[4];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  if (emitted_off(emitted)) {
    if (tid < k) { idx[tid] = -1; score[tid] = __builtin_nan(""); }          // k <= 128
    return;
  }
  const int n = online_count(v);
  const int nn = C > 1 && n < 2 ? 0 : n;                         // z-scored, under two entries: no row statistics, nothing is reported, masked or not
  double mean[C], sd[C];
#pragma unroll
  for (int c = 0; c < C; c++) { mean[c] = C > 1 ? v.stats[2 * c] : 0.0; sd[c] = C > 1 ? v.stats[2 * c + 1] : 1.0; }
  const size_t cap = (size_t)v.capacity;
  constexpr int U = C == 2 ? 4 : 2;                              // the unroll factor of the sweep
  double pv = -__builtin_inf();
  int pj = -1;
  for (int t = 0; t < k; t++) {
    double bv = __builtin_nan("");
    int bj = 0x7fffffff;
#pragma unroll U
    for (int j = tid; j < nn; j += 256) {
      double f = C == 1 ? rows[j] : 0.0;                         // C > 1: run_test.m:40 in the oracle's order of additions, then the mask (:47-53)
#pragma unroll
      for (int c = 0; C > 1 && c < C; c++) f += (c & 1 ? 1.0 : p_weight) * ((rows[c * cap + j] - mean[c]) / sd[c]);
      if (n - j < mask_width) f = __builtin_inf();               // the query is row n
      if (f != f || !sel_less(pv, pj, f, j)) continue;           // NaN, or selected already
      if (bj == 0x7fffffff || sel_less(f, j, bv, bj)) { bv = f; bj = j; }
    }
    int sj;
    const double sv = block_argmin256(bv, bj, red, ired, tid, &sj);
    if (sj < 0) {                                                // fewer than k candidates: -1 / NaN fill the rest
      if (tid == 0) for (int u = t; u < k; u++) { idx[u] = -1; score[u] = __builtin_nan(""); }
      break;
    }
    if (tid == 0) { idx[t] = sj; score[t] = sv; }
    pv = sv; pj = sj;
  }
}

__global__ __launch_bounds__(256) void online_append_kernel(OnlineView v, OnlineParts src, const int* __restrict__ emitted, int* __restrict__ info) {
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  const int n = online_count(v);
  int flags = v.state[1] & ONLINE_OVERFLOW;
  const bool off = emitted_off(emitted), store = !off && n < v.capacity;
  if (store) {                                                   // row n < capacity of every part (len[1] = 0: there is no second)
#pragma unroll
    for (int p = 0; p < 2; p++) {
      double* dst = v.part[p] + (size_t)n * v.len[p];
      for (int i = tid; i < v.len[p]; i += 256) dst[i] = src.p[p][i];
    }
  }
  __syncthreads();                                               // every thread has read state
  if (tid == 0) {                                                // the ONE commit
    if (!off) {
      if (!store) flags |= ONLINE_OVERFLOW;
      v.state[0] = n + (store ? 1 : 0);
      v.state[1] = flags;
    }
    info[0] = store ? 1 : 0; info[1] = store ? n : -1; info[2] = n + (store ? 1 : 0); info[3] = flags;
  }
}

}  // namespace

void launch_online_match(hipStream_t st, const OnlineView& v, const OnlineParts& q, const int* emitted, int mask_width, double p_weight, int k,
                         int* idx, double* score, double* rows) {
  const dim3 grid(v.NB), one(1), block(256);
  const double* r = rows;
  switch (v.kind) {
    case ONLINE_SC: hipLaunchKernelGGL((online_rows_kernel<true, false>), grid, block, 0, st, v, q.p[0], q.p[1], emitted, rows); break;
    case ONLINE_M2DP: hipLaunchKernelGGL((online_rows_kernel<false, true>), grid, block, 0, st, v, q.p[0], q.p[1], emitted, rows); break;
    case ONLINE_FUSED: hipLaunchKernelGGL((online_rows_kernel<true, true>), grid, block, 0, st, v, q.p[0], q.p[1], emitted, rows); break;
    default: hipLaunchKernelGGL(online_delight_rows_kernel, grid, block, 0, st, v, q.p[0], emitted, rows); break;
  }
  if (v.kind == ONLINE_FUSED) hipLaunchKernelGGL(online_stats_kernel<4>, one, block, 0, st, v, emitted, r);
  else if (v.kind != ONLINE_DELIGHT) hipLaunchKernelGGL(online_stats_kernel<2>, one, block, 0, st, v, emitted, r);
  if (v.kind == ONLINE_FUSED) hipLaunchKernelGGL(online_select_kernel<4>, one, block, 0, st, v, emitted, r, mask_width, p_weight, k, idx, score);
  else if (v.kind == ONLINE_DELIGHT) hipLaunchKernelGGL(online_select_kernel<1>, one, block, 0, st, v, emitted, r, mask_width, p_weight, k, idx, score);
  else hipLaunchKernelGGL(online_select_kernel<2>, one, block, 0, st, v, emitted, r, mask_width, p_weight, k, idx, score);
}

void launch_online_append(hipStream_t st, const OnlineView& v, const OnlineParts& src, const int* emitted, int* info) {
  hipLaunchKernelGGL(online_append_kernel, dim3(1), dim3(256), 0, st, v, src, emitted, info);
}

}  // namespace pr
