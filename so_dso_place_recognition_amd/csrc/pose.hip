// pose.hip — the two small kernels around the ICP refinement of a match (no reference counterpart; the normative
// arithmetic is tests/pose_np.py).  Compiled with -ffp-contract=off: pose_seed() (pose_seed.hpp) rounds like its host form.
//
// pose_seed_kernel     one lane per (pair, hypothesis): idx, the hypothesis' variant and the two PCA frames -> the seed T0 = [R | t] and
//                      the slot's (pair_src, pair_dst) for pr_icp_pairs_dev.  A slot without a pose - no candidate, a candidate of
//                      another shard, a variant outside the type's range, a frame of fewer than 3 points or with a non-finite entry, a
//                      second hypothesis that repeats the first - gets (-1, -1) and [I | 0]: PR_ICP_NO_PAIR downstream, no ICP work.
// verify_select_kernel one lane per pair: of the pair's H refined hypotheses the qualified one (status converged or max_iter) with the
//                      larger fitness, then the smaller rmse, then the smaller h; hypothesis 0 when none qualifies.  A NaN never wins.
// Both are latency-bound (a few hundred bytes per lane); fp64, plain C++, vector stores only.
#include "kernels.hpp"
#include "pose_seed.hpp"

namespace pr {
namespace {

constexpr int PS_THREADS = 256;

// mean, eigenvectors and the count: the entries the seed reads (slots 14 / 15 are optional intensity averages)
__device__ __forceinline__ bool frame_usable(const double* __restrict__ f) {
  bool ok = f[13] >= 3.0 && f[13] < INFINITY;
#pragma unroll
  for (int i = 0; i < 12; i++) ok = ok && (fabs(f[i]) < INFINITY);
  return ok;
}

__global__ __launch_bounds__(PS_THREADS) void pose_seed_kernel(int type, const double* __restrict__ frames_q, int m,
                                                                const double* __restrict__ frames_db, int n_local, int db_row0, int k,
                                                                const int* __restrict__ idx, const int* __restrict__ variant, int stride, int H,
                                                                const double* __restrict__ angles, double* __restrict__ T0,
                                                                int* __restrict__ pair_src, int* __restrict__ pair_dst) {
  const int slot = blockIdx.x * PS_THREADS + threadIdx.x;
  if (slot >= m * k * H) return;
  const int p = slot / H, h = slot - p * H, q = p / k;
  const int gi = idx[p];
  const long long local = (long long)gi - db_row0;
  const int v = variant[(size_t)p * stride + h];
  bool ok = gi >= 0 && local >= 0 && local < n_local && v >= 0 && v < pose_variants(type);
  if (ok && h > 0 && variant[(size_t)p * stride] == v) ok = false;
  const double* fq = frames_q + 16 * (size_t)q;
  const double* fd = frames_db + 16 * (size_t)(ok ? local : 0);
  ok = ok && frame_usable(fq) && frame_usable(fd);
  double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  if (ok) pose_seed(type, fq, fd, v, angles, angles + POSE_SC_ANGLES, T);
  double* o = T0 + 12 * (size_t)slot;
#pragma unroll
  for (int i = 0; i < 12; i++) o[i] = T[i];
  pair_src[slot] = ok ? q : -1;
  pair_dst[slot] = ok ? (int)local : -1;
}

__global__ __launch_bounds__(PS_THREADS) void verify_select_kernel(const double* __restrict__ T_h, const IcpStats* __restrict__ stats_h, int c, int H,
                                                                    double min_fitness, double max_rmse, double* __restrict__ T,
                                                                    IcpStats* __restrict__ stats, unsigned char* __restrict__ accepted,
                                                                    int* __restrict__ hyp) {
  const int p = blockIdx.x * PS_THREADS + threadIdx.x;
  if (p >= c) return;
  int best = pose_select(stats_h + (size_t)p * H, H, ICP_CONVERGED, ICP_MAX_ITER);
  const bool q = best >= 0;
  if (!q) best = 0;
  const IcpStats sb = stats_h[(size_t)p * H + best];
  const double* src = T_h + 12 * ((size_t)p * H + best);
  double* o = T + 12 * (size_t)p;
#pragma unroll
  for (int i = 0; i < 12; i++) o[i] = src[i];
  stats[p] = sb;
  hyp[p] = best;
  accepted[p] = (q && sb.fitness >= min_fitness && sb.rmse <= max_rmse) ? 1 : 0;
}

}  // namespace

void launch_pose_seed(hipStream_t st, int type, const double* frames_q, int m, const double* frames_db, int n_local, int db_row0, int k,
                      const int* idx, const int* variant, int stride, int H, const double* angles, double* T0, int* pair_src, int* pair_dst) {
  const int slots = m * k * H;
  if (slots > 0)
    hipLaunchKernelGGL(pose_seed_kernel, dim3((slots + PS_THREADS - 1) / PS_THREADS), dim3(PS_THREADS), 0, st, type, frames_q, m, frames_db, n_local,
                       db_row0, k, idx, variant, stride, H, angles, T0, pair_src, pair_dst);
}

void launch_verify_select(hipStream_t st, const double* T_h, const IcpStats* stats_h, int c, int H, double min_fitness, double max_rmse, double* T,
                          IcpStats* stats, unsigned char* accepted, int* hyp) {
  if (c > 0)
    hipLaunchKernelGGL(verify_select_kernel, dim3((c + PS_THREADS - 1) / PS_THREADS), dim3(PS_THREADS), 0, st, T_h, stats_h, c, H, min_fitness, max_rmse,
                       T, stats, accepted, hyp);
}

}  // namespace pr
