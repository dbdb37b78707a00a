// icp_common.hpp — what the brute-force correspondence kernels (icp.hip) and the uniform-grid ones (icp_grid.hip) share on the device: a
// pair's clouds, the transform, one inlier's terms, the fixed tree of a chunk and the chunk's 17 inlier sums as the launch that knows the
// final correspondences forms them.  One definition: both searches produce the same bits because they run the same code.  Compiled with
// -ffp-contract=off like its includers.
#pragma once
#include "kernels.hpp"

namespace pr {
namespace icp_dev {

constexpr int IC_THREADS = 256;

struct PairShape { long long q0, d0; int ns, nd; };

// the pair's clouds: first rows and sizes (clamped to the call's bounds); false: no pair
__device__ __forceinline__ bool pair_shape(const IcpClouds& A, int pair, PairShape& s) {
  const int src = A.pair_src[pair], dst = A.pair_dst[pair];
  if (src < 0 || dst < 0 || src >= A.Nq || dst >= A.Nd) return false;
  s.q0 = A.offs_q[src];
  s.d0 = A.offs_d[dst];
  const long long ns = A.offs_q[src + 1] - s.q0, nd = A.offs_d[dst + 1] - s.d0;
  s.ns = (int)(ns < 0 ? 0 : (ns > A.max_src ? A.max_src : ns));
  s.nd = (int)(nd < 0 ? 0 : (nd > A.max_dst ? A.max_dst : nd));
  return true;
}

__device__ __forceinline__ void transform(const double* __restrict__ T, double x, double y, double z, double (&p)[3]) {
#pragma unroll
  for (int a = 0; a < 3; a++) p[a] = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
}

// one inlier's terms, added to the lane's 17 sums
__device__ __forceinline__ void add_inlier(double (&a)[ICP_PARTIAL], const double (&p)[3], const double* __restrict__ q, double d2) {
  const double qx = q[0], qy = q[1], qz = q[2];
  a[0] += 1.0; a[1] += d2;
  a[2] += p[0]; a[3] += p[1]; a[4] += p[2];
  a[5] += qx; a[6] += qy; a[7] += qz;
#pragma unroll
  for (int r = 0; r < 3; r++) { a[8 + 3 * r] += p[r] * qx; a[9 + 3 * r] += p[r] * qy; a[10 + 3 * r] += p[r] * qz; }
}

// the fixed tree of a chunk: 64-lane shuffle tree per wave, then the four waves in order
__device__ __forceinline__ void reduce_partial(const double (&a)[ICP_PARTIAL], double (*red)[ICP_PARTIAL], double* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < ICP_PARTIAL; k++) {
    double v = a[k];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < ICP_PARTIAL) out[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// a chunk of 256 source points, one per lane, whose final correspondences (bd, bj) are known: lane's point i (has: i is a point of the
// cloud) is transformed again - the same operations, the same bits -, enters the sums when bd < mc2, and the tree writes the chunk's 17
// sums to out.  Every lane of the workgroup calls it.
__device__ __forceinline__ void chunk_sums(const IcpClouds& A, const PairShape& S, const double* __restrict__ T, int pair, int i, bool has, double bd,
                                           int bj, double mc2, double (*red)[ICP_PARTIAL], double* __restrict__ out) {
  double a[ICP_PARTIAL];
#pragma unroll
  for (int k = 0; k < ICP_PARTIAL; k++) a[k] = 0.0;
  if (has && bd < mc2) {
    const double* s = A.xyz_q + 3 * (size_t)(S.q0 + i);
    double p[3];
    transform(T + 12 * (size_t)pair, s[0], s[1], s[2], p);
    add_inlier(a, p, A.xyz_d + 3 * (size_t)(S.d0 + bj), bd);
  }
  reduce_partial(a, red, out);
}

}  // namespace icp_dev
}  // namespace pr
