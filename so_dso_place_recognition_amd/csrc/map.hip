// map.hip — the resident keyframe map (no reference counterpart): a CSR set of keyframe clouds with their PCA frames, poses
// and ids over caller-owned buffers, grown on the stream.  One append is three launches whose grids depend on N, max_points and the create
// capacities only; everything that varies (how many keyframes the map holds, the clouds' sizes, whether the push in front emitted at all)
// is read from device memory, so one captured append serves every keyframe:
//   plan    ONE lane: reads state and offs[keyframes], walks the N sizes and decides per cloud - no free row: not appended; a row but
//           too many points (max_cloud_points, the room left in xyz, the call's max_points): the row gets an empty cloud and a zero
//           frame; else the cloud's first point in the map.  Writes the plan scratch only, nothing of the map.
//   copy    one lane per point of the call: finds its cloud in the plan's prefix (binary search over N + 1 words) and moves three
//           doubles and one float.  Lanes of a cloud that is not stored, and lanes past the total, leave.
//   commit  one workgroup: the rows of offs, frames, poses and ids, then state and info.
// No kernel waits for another workgroup.  A few hundred KB per keyframe: launch- and latency-bound, plain coalesced 8- and 4-byte
// accesses.  Plain C++, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace pr {
namespace {

enum { PH_NAPP = 0, PH_FIRST, PH_TOTAL, PH_FLAGS, PH_KEYS, PH_EMIT };
static_assert(PH_EMIT < MAP_PLAN_HEAD, "plan head");

__device__ __forceinline__ int64_t* plan_cum(const MapView& v) { return v.plan + MAP_PLAN_HEAD; }
__device__ __forceinline__ int64_t* plan_dst(const MapView& v) { return v.plan + MAP_PLAN_HEAD + v.max_append + 1; }
__device__ __forceinline__ int64_t* plan_end(const MapView& v) { return v.plan + MAP_PLAN_HEAD + 2 * (size_t)v.max_append + 1; }

__global__ __launch_bounds__(64) void map_plan_kernel(MapView v, const int64_t* __restrict__ offs, const int* __restrict__ emitted, int N,
                                                      int64_t max_points) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t *head = v.plan, *cum = plan_cum(v), *dst = plan_dst(v), *end = plan_end(v);
  int keys = v.state[0];
  keys = keys < 0 ? 0 : (keys > v.kcap ? v.kcap : keys);         // a scribbled state word must not turn into a row outside the buffers
  int flags = v.state[1] & MAP_OVERFLOW;
  const bool emit = !emitted || emitted[0] != 0;
  int64_t fill = v.offs[keys];
  fill = fill < 0 ? 0 : (fill > v.pcap ? v.pcap : fill);
  int64_t at = 0;                                                 // the cloud's first point, counted from the call's first; saturates
  int napp = 0;
  if (emit) {
    for (int i = 0; i < N; i++) {
      int64_t size = offs[i + 1] - offs[i];
      if (size < 0) size = 0;
      cum[i] = at;
      dst[i] = -1;
      if (keys + napp >= v.kcap) {
        flags |= MAP_OVERFLOW;
      } else {
        const bool drop = size > v.max_cloud || size > v.pcap - fill || (size > 0 && at + size > max_points);
        if (drop) flags |= MAP_OVERFLOW | MAP_DROPPED;
        else { dst[i] = fill; fill += size; }
        end[i] = fill;
        napp++;
      }
      at = (size > max_points - at) ? max_points + 1 : at + size;
    }
    cum[N] = at;
  }
  head[PH_NAPP] = napp;
  head[PH_FIRST] = napp > 0 ? keys : -1;
  head[PH_TOTAL] = emit ? (at > max_points ? max_points : at) : 0;
  head[PH_FLAGS] = flags;
  head[PH_KEYS] = keys;
  head[PH_EMIT] = emit ? 1 : 0;
}

__global__ __launch_bounds__(256) void map_copy_kernel(MapView v, const double* __restrict__ xyz, const float* __restrict__ inten,
                                                       const int64_t* __restrict__ offs, int N) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= v.plan[PH_TOTAL]) return;
  const int64_t* cum = plan_cum(v);
  int lo = 0, hi = N;                                             // the last cloud with cum[i] <= t: cum[0] = 0 <= t < cum[N]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= t) lo = mid; else hi = mid;
  }
  const int64_t d0 = plan_dst(v)[lo];
  if (d0 < 0) return;
  const int64_t r = t - cum[lo];
  const size_t s = (size_t)(offs[lo] + r), d = (size_t)(d0 + r);  // d < point_capacity: the plan kept d0 + size inside it
  v.xyz[3 * d] = xyz[3 * s]; v.xyz[3 * d + 1] = xyz[3 * s + 1]; v.xyz[3 * d + 2] = xyz[3 * s + 2];
  v.inten[d] = inten[s];
}

__global__ __launch_bounds__(256) void map_commit_kernel(MapView v, const double* __restrict__ frames, const double* __restrict__ poses,
                                                         const int* __restrict__ ids, int* __restrict__ info) {
  if (blockIdx.x != 0) return;
  const int64_t* head = v.plan;
  const int napp = (int)head[PH_NAPP], keys = (int)head[PH_KEYS], tid = threadIdx.x;
  const int64_t *dst = plan_dst(v), *end = plan_end(v);
  const size_t row0 = (size_t)keys;                              // rows keys .. keys + napp - 1 < keyframe_capacity (the plan's test)
  for (int64_t j = tid; j < (int64_t)napp * 16; j += 256) v.frames[16 * row0 + j] = dst[j >> 4] >= 0 ? frames[j] : 0.0;
  for (int64_t j = tid; j < (int64_t)napp * 12; j += 256) v.poses[12 * row0 + j] = poses ? poses[j] : 0.0;
  for (int j = tid; j < napp; j += 256) {
    v.ids[row0 + j] = ids ? ids[j] : -1;
    v.offs[row0 + j + 1] = end[j];
  }
  if (tid == 0) {
    const int flags = (int)head[PH_FLAGS];
    if (head[PH_EMIT]) { v.state[0] = keys + napp; v.state[1] = flags & MAP_OVERFLOW; }
    info[0] = napp; info[1] = (int)head[PH_FIRST]; info[2] = keys + napp; info[3] = flags;
  }
}

}  // namespace

void launch_map_append(hipStream_t st, const MapView& v, const double* xyz, const float* inten, const int64_t* offs, const double* frames,
                       const double* poses, const int* ids, const int* emitted, int N, int64_t max_points, int* info) {
  hipLaunchKernelGGL(map_plan_kernel, dim3(1), dim3(64), 0, st, v, offs, emitted, N, max_points);
  const unsigned nblk = (unsigned)((max_points + 255) / 256);
  if (N > 0 && nblk > 0) hipLaunchKernelGGL(map_copy_kernel, dim3(nblk), dim3(256), 0, st, v, xyz, inten, offs, N);
  hipLaunchKernelGGL(map_commit_kernel, dim3(1), dim3(256), 0, st, v, frames, poses, ids, info);
}

}  // namespace pr
