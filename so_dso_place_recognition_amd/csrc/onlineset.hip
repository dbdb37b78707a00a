// onlineset.hip — the online signature SETS (no reference counterpart): what online.hip is for one SC or M2DP database,
// for the two configurations that need more than one: FUSED (BASELINE config 5: the SC and the M2DP rows of every keyframe, the four row
// z-scores in ONE selection) and DELIGHT.  All parts of a set share ONE device-side count, committed by one thread of one launch, so
// the parts can never disagree about it.  Every grid depends on the create sizes only; the count and whether the push in front emitted
// are read from device memory, so one captured match + append serves every keyframe.
//   FUSED   rows    NB workgroups: workgroup b takes entries b, b + NB, ... < count and makes online_rows_kernel's four pair calls
//                   (rerank_common.hpp: sc_pair_exact twice, m2dp_pair_exact twice - the same calls, so the same bits) and ALWAYS writes
//                   its partial (entries that are not NaN, sum of d - 0.5) per channel
//           stats   one workgroup: online_stats_kernel's rule for four channels
//           select  f = 0; f += p z0; f += 1 z1; f += p z2; f += 1 z3 (the oracle's order), THEN +Inf under the mask (a masked NaN
//                   becomes a selectable +Inf, as in pr_ref_match_topk_fused), the k smallest by (score, index) in k sweeps
//   DELIGHT rows    NB workgroups: workgroup b takes the batches b, b + NB, ... of 16 entries below the count through exact_batch
//                   (delight_exact.hpp: the text the DelightMatcher's exact rows use)
//           select  the distance is the score: no statistics (run_test.m:26-41), the mask, the same k sweeps; one row is enough
//   append  one workgroup: every part to row `count`, then - behind its own barrier - ONE thread commits state and info
// No kernel waits for another workgroup: no atomics, no tickets.  Fixed-order reductions.  Plain C++, vector stores only.
#include "onlineset.hpp"
#include "delight_exact.hpp"
#include "rerank_common.hpp"

namespace pr {
namespace {

__device__ __forceinline__ bool set_off(const int* emitted) { return emitted && emitted[0] == 0; }
// a scribbled state word must not turn into a row outside the buffers
__device__ __forceinline__ int set_count(const OnlineSetView& v) {
  const int n = v.state[0];
  return n < 0 ? 0 : (n > v.capacity ? v.capacity : n);
}

__global__ __launch_bounds__(256) void onlineset_fused_rows_kernel(OnlineSetView v, const double* __restrict__ sc, const double* __restrict__ m2dp,
                                                                   const int* __restrict__ emitted, double* __restrict__ rows) {
  __shared__ double buf[60 * 21 + 1200];
  __shared__ double red[256];
  if (set_off(emitted)) return;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = set_count(v);
  double cnt[4] = {0.0, 0.0, 0.0, 0.0}, sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = b; j < n; j += v.NB) {                            // j < capacity: the rows of both buffers and the four quarters of rows exist
    double d[4];
    d[0] = sc_pair_exact(sc, 0, 0, v.sc, 0, (size_t)j * 2400, buf, red, tid);
    d[1] = sc_pair_exact(sc, 0, 1200, v.sc, 0, (size_t)j * 2400 + 1200, buf, red, tid);
    d[2] = m2dp_pair_exact(m2dp, 0, 0, v.m2dp, 0, (size_t)j * 1536, 0, red, tid);
    d[3] = m2dp_pair_exact(m2dp, 0, 0, v.m2dp, 0, (size_t)j * 1536, 1, red, tid);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (tid == 0) rows[(size_t)c * v.capacity + j] = d[c];     // (every thread holds the block-wide value)
      if (d[c] == d[c]) { cnt[c] += 1.0; sum[c] += d[c] - 0.5; }
    }
  }
  if (tid == 0) {
    double* p = v.partial + (size_t)b * 8;                       // b < NB = the grid
#pragma unroll
    for (int c = 0; c < 4; c++) { p[2 * c] = cnt[c]; p[2 * c + 1] = sum[c]; }
  }
}

__global__ __launch_bounds__(256) void onlineset_fused_stats_kernel(OnlineSetView v, const int* __restrict__ emitted, const double* __restrict__ rows) {
  __shared__ double tot[8];
  __shared__ double red[4];
  if (blockIdx.x != 0 || set_off(emitted)) return;
  const int tid = threadIdx.x;
  const int n = set_count(v);
  if (tid < 8) {
    double s = 0.0;
    for (int b = 0; b < v.NB; b++) s += v.partial[(size_t)b * 8 + tid];      // workgroup order: deterministic
    tot[tid] = s;
  }
  __syncthreads();
  for (int ch = 0; ch < 4; ch++) {
    const double N = tot[2 * ch], mean = 0.5 + tot[2 * ch + 1] / N;          // no entry: 0 / 0 = NaN
    const double* r = rows + (size_t)ch * v.capacity;
    double a = 0.0, c = 0.0;
    for (int j = tid; j < n; j += 256) {
      const double d = r[j];
      if (d == d) { const double x = d - mean; a += x * x; c += x; }
    }
    const double A = block_sum256(a, red, tid), C = block_sum256(c, red, tid);
    if (tid == 0) {
      v.stats[2 * ch] = mean;
      v.stats[2 * ch + 1] = sqrt((A - C * C / N) / (N - 1.0));               // one entry: 0 / 0 = NaN
    }
  }
}

__global__ __launch_bounds__(256) void onlineset_delight_rows_kernel(OnlineSetView v, const double* __restrict__ sig, const int* __restrict__ emitted,
                                                                     double* __restrict__ rows) {
  __shared__ XShared sh;
  __shared__ const double* pa[XB];
  __shared__ const double* pb[XB];
  __shared__ double dd[XB];
  if (set_off(emitted)) return;
  const int tid = threadIdx.x;
  const int n = set_count(v);
  for (int rb = blockIdx.x * XB; rb < n; rb += v.NB * XB) {      // uniform over the workgroup
    const int np = n - rb < XB ? n - rb : XB;                    // rb + np <= n <= capacity
    if (tid < XB) { pa[tid] = sig; pb[tid] = v.delight + (size_t)(rb + (tid < np ? tid : 0)) * 4096; }
    __syncthreads();
    exact_batch(sh, tid, np, pa, pb, dd);
    if (tid < np) rows[rb + tid] = dd[tid];
    __syncthreads();
  }
}

__device__ __forceinline__ bool sel_less(double av, int aj, double bv, int bj) { return av < bv || (av == bv && aj < bj); }

template <bool FUSED>
__global__ __launch_bounds__(256) void onlineset_select_kernel(OnlineSetView v, const int* __restrict__ emitted, const double* __restrict__ rows,
                                                               int mask_width, double p_weight, int k, int* __restrict__ idx,
                                                               double* __restrict__ score) {
  __shared__ double red[4];
  __shared__ int ired[4];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  if (set_off(emitted)) {
    if (tid < k) { idx[tid] = -1; score[tid] = __builtin_nan(""); }          // k <= 128
    return;
  }
  const int n = set_count(v);
  const int nn = FUSED && n < 2 ? 0 : n;                         // FUSED under two entries: no row statistics, nothing is reported, masked or not
  double mean[4] = {0.0, 0.0, 0.0, 0.0}, sd[4] = {1.0, 1.0, 1.0, 1.0};
  if (FUSED) {
#pragma unroll
    for (int c = 0; c < 4; c++) { mean[c] = v.stats[2 * c]; sd[c] = v.stats[2 * c + 1]; }
  }
  const size_t cap = (size_t)v.capacity;
  double pv = -__builtin_inf();
  int pj = -1;
  for (int t = 0; t < k; t++) {
    double bv = __builtin_nan("");
    int bj = 0x7fffffff;
#pragma unroll 2
    for (int j = tid; j < nn; j += 256) {
      double f;
      if (FUSED) {                                               // pr_ref_match_topk_fused's order of additions, then the mask
        f = 0.0;
        f += p_weight * ((rows[j] - mean[0]) / sd[0]);
        f += 1.0 * ((rows[cap + j] - mean[1]) / sd[1]);
        f += p_weight * ((rows[2 * cap + j] - mean[2]) / sd[2]);
        f += 1.0 * ((rows[3 * cap + j] - mean[3]) / sd[3]);
      } else {
        f = rows[j];
      }
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

__global__ __launch_bounds__(256) void onlineset_append_kernel(OnlineSetView v, const double* __restrict__ sc, const double* __restrict__ m2dp,
                                                               const double* __restrict__ delight, const int* __restrict__ emitted,
                                                               int* __restrict__ info) {
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  const int n = set_count(v);
  int flags = v.state[1] & ONLINESET_OVERFLOW;
  const bool off = set_off(emitted), store = !off && n < v.capacity;
  if (store) {                                                   // row n < capacity of every part
    if (v.kind == ONLINESET_FUSED) {
      double* d0 = v.sc + (size_t)n * ONLINESET_SC;
      double* d1 = v.m2dp + (size_t)n * ONLINESET_M2DP;
      for (int i = tid; i < ONLINESET_SC; i += 256) d0[i] = sc[i];
      for (int i = tid; i < ONLINESET_M2DP; i += 256) d1[i] = m2dp[i];
    } else {
      double* d2 = v.delight + (size_t)n * ONLINESET_DELIGHT_LEN;
      for (int i = tid; i < ONLINESET_DELIGHT_LEN; i += 256) d2[i] = delight[i];
    }
  }
  __syncthreads();                                               // every thread has read state
  if (tid == 0) {                                                // the ONE commit of the set
    if (!off) {
      if (!store) flags |= ONLINESET_OVERFLOW;
      v.state[0] = n + (store ? 1 : 0);
      v.state[1] = flags;
    }
    info[0] = store ? 1 : 0; info[1] = store ? n : -1; info[2] = n + (store ? 1 : 0); info[3] = flags;
  }
}

}  // namespace

void launch_onlineset_match(hipStream_t st, const OnlineSetView& v, const double* sc, const double* m2dp, const double* delight,
                            const int* emitted, int mask_width, double p_weight, int k, int* idx, double* score, double* rows) {
  if (v.kind == ONLINESET_FUSED) {
    hipLaunchKernelGGL(onlineset_fused_rows_kernel, dim3(v.NB), dim3(256), 0, st, v, sc, m2dp, emitted, rows);
    hipLaunchKernelGGL(onlineset_fused_stats_kernel, dim3(1), dim3(256), 0, st, v, emitted, (const double*)rows);
    hipLaunchKernelGGL(onlineset_select_kernel<true>, dim3(1), dim3(256), 0, st, v, emitted, (const double*)rows, mask_width, p_weight, k, idx, score);
  } else {
    hipLaunchKernelGGL(onlineset_delight_rows_kernel, dim3(v.NB), dim3(256), 0, st, v, delight, emitted, rows);
    hipLaunchKernelGGL(onlineset_select_kernel<false>, dim3(1), dim3(256), 0, st, v, emitted, (const double*)rows, mask_width, p_weight, k, idx, score);
  }
}

void launch_onlineset_append(hipStream_t st, const OnlineSetView& v, const double* sc, const double* m2dp, const double* delight,
                             const int* emitted, int* info) {
  hipLaunchKernelGGL(onlineset_append_kernel, dim3(1), dim3(256), 0, st, v, sc, m2dp, delight, emitted, info);
}

}  // namespace pr
