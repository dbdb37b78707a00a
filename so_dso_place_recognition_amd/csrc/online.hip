// online.hip — the online signature database (no reference counterpart): the raw SC or M2DP rows of the keyframes seen so
// far in a caller-owned buffer with a DEVICE-side count, matched exactly in fp64 and grown on the stream.  The sibling of map.hip for
// signatures: every grid depends on the create sizes only, everything that varies (how many rows the database holds, whether the push
// in front emitted at all) is read from device memory, so one captured match + append serves every keyframe.
//   rows    NB workgroups: workgroup b takes entries b, b + NB, ... < count and both channels of each - the reference's own pair
//           formulation (rerank_common.hpp: sc_pair_exact / m2dp_pair_exact, processSC.m:15-33 / processM2DP.m:12-22) - and ALWAYS
//           writes its partial (entries that are not NaN, sum of d - 0.5) per channel, zeros included
//   stats   one workgroup: the partials in workgroup order -> mean; a second pass over the row about that mean -> sd (N - 1, NaN left
//           out: normalize(.,2)).  Deterministic: fixed lanes, fixed order.
//   select  one workgroup: fused = p_weight z_p + z_i in xrow_select_kernel's operation order, +Inf under the mask (the query is row
//           `count`), and the k smallest by (score, index) in k sweeps; NaN is never selected
//   append  one workgroup: the row to `count`, then - behind its own barrier - state and info
// No kernel waits for another workgroup: no atomics, no tickets.  Plain C++, vector stores only.
#include "online.hpp"
#include "rerank_common.hpp"

namespace pr {
namespace {

__device__ __forceinline__ bool online_off(const int* emitted) { return emitted && emitted[0] == 0; }
// a scribbled state word must not turn into a row outside the buffers
__device__ __forceinline__ int online_count(const OnlineView& v) {
  const int n = v.state[0];
  return n < 0 ? 0 : (n > v.capacity ? v.capacity : n);
}

template <bool SC>
__global__ __launch_bounds__(256) void online_rows_kernel(OnlineView v, const double* __restrict__ sig, const int* __restrict__ emitted,
                                                          double* __restrict__ rows) {
  __shared__ double buf[SC ? 60 * 21 + 1200 : 1];
  __shared__ double red[256];
  if (online_off(emitted)) return;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = online_count(v);
  double c0 = 0.0, s0 = 0.0, c1 = 0.0, s1 = 0.0;
  for (int j = b; j < n; j += v.NB) {                            // j < capacity: the rows of sig and both halves of rows exist
    const double dp = SC ? sc_pair_exact(sig, 0, 0, v.sig, 0, (size_t)j * 2400, buf, red, tid)
                         : m2dp_pair_exact(sig, 0, 0, v.sig, 0, (size_t)j * 1536, 0, red, tid);
    const double di = SC ? sc_pair_exact(sig, 0, 1200, v.sig, 0, (size_t)j * 2400 + 1200, buf, red, tid)
                         : m2dp_pair_exact(sig, 0, 0, v.sig, 0, (size_t)j * 1536, 1, red, tid);
    if (tid == 0) { rows[j] = dp; rows[(size_t)v.capacity + j] = di; }      // (every thread holds the block-wide value)
    if (dp == dp) { c0 += 1.0; s0 += dp - 0.5; }
    if (di == di) { c1 += 1.0; s1 += di - 0.5; }
  }
  if (tid == 0) {
    double* p = v.partial + (size_t)b * 4;                       // b < NB = the grid
    p[0] = c0; p[1] = s0; p[2] = c1; p[3] = s1;
  }
}

__global__ __launch_bounds__(256) void online_stats_kernel(OnlineView v, const int* __restrict__ emitted, const double* __restrict__ rows) {
  __shared__ double tot[4];
  __shared__ double red[4];
  if (blockIdx.x != 0 || online_off(emitted)) return;
  const int tid = threadIdx.x;
  const int n = online_count(v);
  if (tid < 4) {
    double s = 0.0;
    for (int b = 0; b < v.NB; b++) s += v.partial[(size_t)b * 4 + tid];      // workgroup order: deterministic
    tot[tid] = s;
  }
  __syncthreads();
  for (int ch = 0; ch < 2; ch++) {
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

__device__ __forceinline__ bool sel_less(double av, int aj, double bv, int bj) { return av < bv || (av == bv && aj < bj); }

__global__ __launch_bounds__(256) void online_select_kernel(OnlineView v, const int* __restrict__ emitted, const double* __restrict__ rows,
                                                            int mask_width, double p_weight, int k, int* __restrict__ idx,
                                                            double* __restrict__ score) {
  __shared__ double red[4];
  __shared__ int ired[4];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  if (online_off(emitted)) {
    if (tid < k) { idx[tid] = -1; score[tid] = __builtin_nan(""); }          // k <= 128
    return;
  }
  const int n = online_count(v);
  const int nn = n < 2 ? 0 : n;                                  // under two entries there are no row statistics: nothing is reported, masked or not
  const double m0 = v.stats[0], sd0 = v.stats[1], m1 = v.stats[2], sd1 = v.stats[3];
  const double* r0 = rows;
  const double* r1 = rows + (size_t)v.capacity;
  double pv = -__builtin_inf();
  int pj = -1;
  for (int t = 0; t < k; t++) {
    double bv = __builtin_nan("");
    int bj = 0x7fffffff;
#pragma unroll 4
    for (int j = tid; j < nn; j += 256) {
      double f = 0.0;                                            // run_test.m:40 in xrow_select_kernel's operation order, then the mask (:47-53)
      f += p_weight * ((r0[j] - m0) / sd0);
      f += 1.0 * ((r1[j] - m1) / sd1);
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

__global__ __launch_bounds__(256) void online_append_kernel(OnlineView v, const double* __restrict__ sig, const int* __restrict__ emitted,
                                                            int* __restrict__ info) {
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  const int n = online_count(v);
  int flags = v.state[1] & ONLINE_OVERFLOW;
  const bool off = online_off(emitted), store = !off && n < v.capacity;
  if (store) {
    double* dst = v.sig + (size_t)n * v.sig_doubles;             // row n < capacity
    for (int i = tid; i < v.sig_doubles; i += 256) dst[i] = sig[i];
  }
  __syncthreads();                                               // every thread has read state
  if (tid == 0) {
    if (!off) {
      if (!store) flags |= ONLINE_OVERFLOW;
      v.state[0] = n + (store ? 1 : 0);
      v.state[1] = flags;
    }
    info[0] = store ? 1 : 0; info[1] = store ? n : -1; info[2] = n + (store ? 1 : 0); info[3] = flags;
  }
}

}  // namespace

void launch_online_match(hipStream_t st, const OnlineView& v, const double* sig, const int* emitted, int mask_width, double p_weight, int k,
                         int* idx, double* score, double* rows) {
  if (v.type == 0) hipLaunchKernelGGL(online_rows_kernel<true>, dim3(v.NB), dim3(256), 0, st, v, sig, emitted, rows);
  else hipLaunchKernelGGL(online_rows_kernel<false>, dim3(v.NB), dim3(256), 0, st, v, sig, emitted, rows);
  hipLaunchKernelGGL(online_stats_kernel, dim3(1), dim3(256), 0, st, v, emitted, (const double*)rows);
  hipLaunchKernelGGL(online_select_kernel, dim3(1), dim3(256), 0, st, v, emitted, (const double*)rows, mask_width, p_weight, k, idx, score);
}

void launch_online_append(hipStream_t st, const OnlineView& v, const double* sig, const int* emitted, int* info) {
  hipLaunchKernelGGL(online_append_kernel, dim3(1), dim3(256), 0, st, v, sig, emitted, info);
}

}  // namespace pr
