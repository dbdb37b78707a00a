// icp_common.hpp — what the brute-force correspondence kernels (icp.hip) and the uniform-grid ones (icp_grid.hip) share on the device: a
// pair's clouds, the transform, a chunk's pivot, one inlier's terms, the fixed tree of a chunk and the chunk's 17 inlier sums as the launch that knows the
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

// The PIVOT of a chunk's update sums: the correspondence q of the chunk's FIRST inlier (lowest point index), so it lies inside the inlier
// set whatever else the clouds hold (a NaN, a max-range sentinel or a far outlier in the target is nobody's inlier and nobody's pivot).
// p' and q enter the sums as p' - pivot and q - pivot: the sums have the size of the inlier set's extent and not of its distance from
// the coordinates' origin, and H = sum p' q^T - (sum p')(sum q)^T / n cancels extent^2 / spread^2 ulps, whatever the origin (world-frame
// or UTM clouds).  The chunk writes its pivot behind its 17 sums; icp_finish_kernel moves every chunk's sums to the first chunk's pivot.
// key: the chunk-local index of the lane's first inlier (0xFFFFFFFF: none), bj: its target row; xd: the pair's target rows; red: the
// workgroup's [IC_THREADS / 64][ICP_PARTIAL] LDS (slot ICP_SUMS of each row carries the wave's minimum).  Every lane of the workgroup
// calls it; c = 0 for a chunk without inliers.
__device__ __forceinline__ void chunk_pivot(unsigned key, int bj, const double* __restrict__ xd, double (*red)[ICP_PARTIAL], double (&c)[3]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long v = ((unsigned long long)key << 32) | (unsigned)bj;
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_down(v, d);
    v = o < v ? o : v;
  }
  if (lane == 0) *reinterpret_cast<unsigned long long*>(&red[w][ICP_SUMS]) = v;
  __syncthreads();
  unsigned long long m = *reinterpret_cast<const unsigned long long*>(&red[0][ICP_SUMS]);
#pragma unroll
  for (int k = 1; k < IC_THREADS / 64; k++) {
    const unsigned long long o = *reinterpret_cast<const unsigned long long*>(&red[k][ICP_SUMS]);
    m = o < m ? o : m;
  }
  c[0] = c[1] = c[2] = 0.0;
  if ((unsigned)(m >> 32) != 0xFFFFFFFFu) {
    const double* q = xd + 3 * (size_t)(unsigned)(m & 0xFFFFFFFFu);
    c[0] = q[0]; c[1] = q[1]; c[2] = q[2];
  }
}

// one inlier's terms about the pivot c, added to the lane's 17 sums
__device__ __forceinline__ void add_inlier(double (&a)[ICP_SUMS], const double (&p)[3], const double* __restrict__ q, double d2,
                                           const double (&c)[3]) {
  const double qx = q[0] - c[0], qy = q[1] - c[1], qz = q[2] - c[2];
  const double pc[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  a[0] += 1.0; a[1] += d2;
  a[2] += pc[0]; a[3] += pc[1]; a[4] += pc[2];
  a[5] += qx; a[6] += qy; a[7] += qz;
#pragma unroll
  for (int r = 0; r < 3; r++) { a[8 + 3 * r] += pc[r] * qx; a[9 + 3 * r] += pc[r] * qy; a[10 + 3 * r] += pc[r] * qz; }
}

// the fixed tree of a chunk: 64-lane shuffle tree per wave, then the four waves in order; the chunk's pivot c goes behind the 17 sums
__device__ __forceinline__ void reduce_partial(const double (&a)[ICP_SUMS], const double (&c)[3], double (*red)[ICP_PARTIAL],
                                               double* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < ICP_SUMS; k++) {
    double v = a[k];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < ICP_SUMS) out[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  if (threadIdx.x == 0) { out[ICP_SUMS] = c[0]; out[ICP_SUMS + 1] = c[1]; out[ICP_SUMS + 2] = c[2]; }
}

// a chunk of 256 source points, one per lane, whose final correspondences (bd, bj) are known: lane's point i (has: i is a point of the
// cloud) is transformed again - the same operations, the same bits -, enters the sums when bd < mc2, and the tree writes the chunk's 17
// sums and its pivot to out.  Every lane of the workgroup calls it.
__device__ __forceinline__ void chunk_sums(const IcpClouds& A, const PairShape& S, const double* __restrict__ T, int pair, int i, bool has, double bd,
                                           int bj, double mc2, double (*red)[ICP_PARTIAL], double* __restrict__ out) {
  double a[ICP_SUMS], c[3];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; k++) a[k] = 0.0;
  const bool inl = has && bd < mc2;
  chunk_pivot(inl ? threadIdx.x : 0xFFFFFFFFu, bj, A.xyz_d + 3 * (size_t)S.d0, red, c);
  if (inl) {
    const double* s = A.xyz_q + 3 * (size_t)(S.q0 + i);
    double p[3];
    transform(T + 12 * (size_t)pair, s[0], s[1], s[2], p);
    add_inlier(a, p, A.xyz_d + 3 * (size_t)(S.d0 + bj), bd, c);
  }
  reduce_partial(a, c, red, out);
}

}  // namespace icp_dev
}  // namespace pr
