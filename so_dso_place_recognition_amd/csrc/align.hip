// align.hip — which variant of the query lines up best with a matched DB entry, on gfx950 in fp64.  The reference computes every
// variant's distance of a pair and keeps only the minimum (processSC.m:22-33, processM2DP.m:12-22, processDELIGHT.m:7-37); these kernels
// keep its position too: for SC the winning sector shift / mirror is the yaw between the two clouds (pr_sc_relative_pose), the
// initial guess a SLAM front end hands to ICP.
//
//   align          one workgroup per (pair, channel), as rerank_kernel<1>: the SC / M2DP variant arithmetic is rerank_common.hpp's own
//                  (sc_pair_exact / m2dp_pair_exact with ARG = true: the same distances, bit for bit, plus an (index, value) reduction)
//   delight_align  one workgroup per pair, thread = bin column: chi-square of processDELIGHT.m:16-31 for the 4 octant permutations
//
// A pair whose entry is not this shard's (idx = -1, or outside [db_row0, db_row0 + n_local)) gets variant -1 / distance NaN, and its
// workgroups leave at once.  Stream-ordered, no allocation, no host synchronisation: a launch can be captured in a hipGraph.
#include "kernels.hpp"
#pragma clang diagnostic ignored "-Wunused-function"   // (rerank_common.hpp's moments helpers are not used here)
#include "rerank_common.hpp"

namespace pr {
namespace {

struct AlignArgs {
  const void* q_sc; const void* db_sc; int sc_dt;               // raw SC signatures [m][2400] / [n_local][2400] or null
  const void* q_m2; const void* db_m2; int m2_dt;               // raw M2DP signatures [4 m][384] / [4 n_local][384] or null
  int m, n_local, db_row0, k;
  const int32_t* idx;                                           // [m][k] global DB rows, -1 = none
  int32_t* variant; double* dist;                               // [m][k][4]: SC structure, SC intensity, M2DP count, M2DP intensity
};

__global__ __launch_bounds__(256) void align_kernel(AlignArgs A) {
  __shared__ double buf[60 * 21 + 1200];
  __shared__ double red[256];
  __shared__ int ired[4];
  const int tid = threadIdx.x;
  const int nch = (A.q_sc ? 2 : 0) + (A.q_m2 ? 2 : 0);
  const int pair = (int)(blockIdx.x / nch), cl = (int)(blockIdx.x % nch);
  const int c = A.q_sc ? cl : 2 + cl;
  const int q = pair / A.k;
  int32_t* vout = A.variant + (size_t)pair * 4;
  double* dout = A.dist + (size_t)pair * 4;
  if (cl == 0 && tid < 4 && (tid < 2 ? !A.q_sc : !A.q_m2)) { vout[tid] = -1; dout[tid] = __builtin_nan(""); }   // absent descriptor type
  const int jg = A.idx[pair];
  const int jl = jg - A.db_row0;
  if (jg < 0 || jl < 0 || jl >= A.n_local) {                    // no candidate, or another shard's entry
    if (tid == 0) { vout[c] = -1; dout[c] = __builtin_nan(""); }
    return;
  }
  int v;
  const double d = c < 2
      ? sc_pair_exact<true>(A.q_sc, A.sc_dt, (size_t)q * 2400 + c * 1200, A.db_sc, A.sc_dt, (size_t)jl * 2400 + c * 1200, buf, red, tid, ired, &v)
      : m2dp_pair_exact<true>(A.q_m2, A.m2_dt, (size_t)q * 4 * 384, A.db_m2, A.m2_dt, (size_t)jl * 4 * 384, c - 2, red, tid, ired, &v);
  if (tid == 0) { vout[c] = v; dout[c] = d; }
}

// processDELIGHT.m:2-5: row r of permutation k is Mut(k, r + 1) - 1 = r ^ {0, 5, 6, 3}[k]
__device__ __forceinline__ int delight_mut(int k, int r) { return r ^ ((0x3650 >> (4 * k)) & 15); }

// processDELIGHT.m:7-37 for one pair: thread t holds bin column t of the 16 histograms of both signatures; per permutation k the sum of
// 2 (A - B)^2 / (A + B) over the occupied bins (A + B > 0) and their count, block-reduced; the mean of each, and the first strictly smaller
// one wins (`min_dist > ts`: ties -> lower k, a NaN mean - no occupied bin - never wins; none: -1 / +Inf, the untouched min_dist = Inf).
__global__ __launch_bounds__(256) void delight_align_kernel(const void* __restrict__ qh, const void* __restrict__ dbh, int dt, int n_local,
                                                             int db_row0, int k, const int32_t* __restrict__ idx, int32_t* __restrict__ variant,
                                                             double* __restrict__ dist) {
  __shared__ double red[4][8];
  const int tid = threadIdx.x, pair = blockIdx.x, q = pair / k;
  const int jg = idx[pair];
  const int jl = jg - db_row0;
  if (jg < 0 || jl < 0 || jl >= n_local) {
    if (tid == 0) { variant[pair] = -1; dist[pair] = __builtin_nan(""); }
    return;
  }
  double a[16], b[16];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    a[r] = ld(qh, dt, ((size_t)q * 16 + r) * 256 + tid);
    b[r] = ld(dbh, dt, ((size_t)jl * 16 + r) * 256 + tid);
  }
  double acc[8];                                                // [k]: sum of the terms, [4 + k]: occupied bins
#pragma unroll
  for (int p = 0; p < 4; p++) {
    double ts = 0.0, tc = 0.0;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const double x = a[r], y = b[delight_mut(p, r)], s = x + y;
      if (s > 0) {
        const double e = x - y;
        ts += 2.0 * (e * e) / s;                                // processDELIGHT.m:24
        tc += 1.0;
      }
    }
    acc[p] = ts;
    acc[4 + p] = tc;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc[i] += __shfl_xor(acc[i], s, 64);
  }
  if ((tid & 63) == 0)
    for (int i = 0; i < 8; i++) red[tid >> 6][i] = acc[i];
  __syncthreads();
  if (tid == 0) {
    double best = __builtin_inf();
    int v = -1;
    for (int p = 0; p < 4; p++) {
      const double ts = (red[0][p] + red[1][p]) + (red[2][p] + red[3][p]);
      const double tc = (red[0][4 + p] + red[1][4 + p]) + (red[2][4 + p] + red[3][4 + p]);
      const double mean = ts / tc;                              // processDELIGHT.m:29 (0 / 0 = NaN when no bin is occupied)
      if (best > mean) { best = mean; v = p; }                  // processDELIGHT.m:30-32
    }
    variant[pair] = v;
    dist[pair] = best;
  }
}

}  // namespace

void launch_align(hipStream_t st, const void* q_sc, const void* db_sc, int sc_dt, const void* q_m2, const void* db_m2, int m2_dt, int m,
                  int n_local, int db_row0, int k, const int32_t* idx, int32_t* variant, double* dist) {
  const unsigned nch = (q_sc ? 2u : 0u) + (q_m2 ? 2u : 0u);
  if (m <= 0 || nch == 0) return;
  AlignArgs A{q_sc, db_sc, sc_dt, q_m2, db_m2, m2_dt, m, n_local, db_row0, k, idx, variant, dist};
  hipLaunchKernelGGL(align_kernel, dim3((unsigned)m * (unsigned)k * nch), dim3(256), 0, st, A);
}

void launch_delight_align(hipStream_t st, const void* q, const void* db, int dt, int m, int n_local, int db_row0, int k, const int32_t* idx,
                          int32_t* variant, double* dist) {
  if (m <= 0) return;
  hipLaunchKernelGGL(delight_align_kernel, dim3((unsigned)m * (unsigned)k), dim3(256), 0, st, q, db, dt, n_local, db_row0, k, idx, variant, dist);
}

}  // namespace pr
