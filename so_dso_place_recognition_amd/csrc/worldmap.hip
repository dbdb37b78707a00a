// worldmap.hip — the world map (no reference counterpart): a deterministic voxel fusion of all clouds of a resident
// keyframe map (map.hip) into one world-frame point set under ANY [keyframe_capacity][12] pose array - the map's own or the relaxed ones
// (posegraph.hip).  One fuse is two memset nodes and four launches whose grids depend on the create capacities only; the keyframe count,
// the point count and every decision are read and made on the device, so one captured fuse serves every count.
//
// The rule (normative; restated in fp64 in tests/worldmap_np.py).  n = d_n[0] clamped into 0 .. keyframe_capacity, P = offs[n] clamped
// into 0 .. point_capacity (0 when n = 0).  Point g, 0 <= g < P, belongs to row r with offs[r] <= g < offs[r + 1].
//   1. world position: a pose row is world-to-camera [R | t]; d = p - t, w_a = (R[0][a] d0 + R[1][a] d1) + R[2][a] d2 in exactly this
//      association, fp64, no contraction (this file is built with -ffp-contract=off).
//   2. validity: the point is skipped (WORLDMAP_SKIPPED) if one of its pose's 12 entries or one w_a is not finite.  c_a = floor(w_a / cell)
//      with IEEE division; a c_a outside [-2^20, 2^20) - compared as a double, before any conversion - skips the point with
//      WORLDMAP_RANGE.  key = the three indices biased by 2^20, 21 bits each, packed into 63 bits (c_0 highest).
//   3. voxels: the valid points of one key; count = how many; representative = the smallest g (keep = 0) or the largest (keep = 1); the
//      voxel qualifies iff count >= min_count.
//   4. output: the qualifying voxels in ascending order of their representative's g; row j = (w of the representative with the bits of
//      step 1, its intensity, src = g, row = r, count); only j < out_capacity is stored, more set WORLDMAP_OVERFLOW; rows >=
//      min(qualifying, out_capacity) are not written.
//   5. state = {rows written, flags, 0, 0}, info = {rows written, qualifying voxels, valid points, flags}; the flags are the call's.
//
//   clear   two memsets: the table's (key, representative) pairs to all ones - no key has bit 63, and ~0 is the identity of the unsigned
//           minimum - and the counts and the flag word to zero.
//   insert  one lane per point slot of point_capacity: the row by the binary search of map_copy_kernel, the transform, the key, the home
//           slot (key * 0x9E3779B97F4A7C15) >> (64 - log2 T), a linear probe with a 64-bit compare-and-swap on the key, then an unsigned
//           minimum on the representative (g for keep = 0, ~g for keep = 1: the largest g is the smallest ~g) and an add on the count; the
//           slot goes to slot_of[g].  The probe runs at most T steps, then sets WORLDMAP_TABLE and drops the point: no input makes a lane
//           spin, and with T >= 2 point_capacity the table is never more than half full, so that cannot happen.
//   count   per 256 points: how many lanes are the representative of a qualifying voxel, how many are valid.
//   scan    ONE workgroup: the exclusive prefix of the block counts in chunks of 1024, in order; state and info.
//   emit    the lane's place inside its block by ballots, the row and w recomputed by the same inlined code as in insert (the same
//           instructions on the same inputs: the same bits), five stores per output row below out_capacity.
// Every reduction is an integer atomic or an integer scan and a position is computed per point in a fixed association, so the output
// bytes are a function of the inputs alone: equal between runs, between eager and replayed calls, and to the restatement.  No kernel
// waits for another workgroup.  Plain C++, vector stores only, no floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "worldmap_common.hpp"

namespace pr {
namespace {

// world_of, key_of, home_slot: shared with mapgrow.hip.  world_of is step 1, w[a] = (q[a] * d0 + q[4 + a] * d1) + q[8 + a] * d2 with
// d = p - t, and the finiteness half of step 2; key_of is the range half and the packing.
using namespace worldmap_dev;

struct Head { int n; int64_t P; };

__device__ __forceinline__ Head head_of(const WorldMapView& v, const int* __restrict__ nptr) {
  int n = nptr[0];
  n = n < 0 ? 0 : (n > v.kcap ? v.kcap : n);                      // a scribbled count must not turn into a row outside the buffers
  int64_t P = n > 0 ? v.m_offs[n] : 0;
  P = P < 0 ? 0 : (P > v.pcap ? v.pcap : P);
  return {n, P};
}

// the last row r in 0 .. n - 1 with offs[r] <= g (n >= 1; offs[0] = 0 <= g < offs[n]): an empty row owns nothing
__device__ __forceinline__ int row_of(const int64_t* __restrict__ offs, int n, int64_t g) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t rep_of(u64 word, int keep) { return (int64_t)(keep ? ~word : word); }

// is lane g the representative of a voxel that qualifies; *valid: does the point sit in the table at all
__device__ __forceinline__ bool is_row(const WorldMapView& v, int64_t g, int64_t P, int min_count, int keep, bool* valid, int* slot) {
  const int s = g < P ? v.slot_of[g] : -1;
  *valid = s >= 0;
  *slot = s;
  return s >= 0 && rep_of(v.slots[2 * (size_t)s + 1], keep) == g && v.cnt[s] >= min_count;
}

__global__ __launch_bounds__(256) void worldmap_insert_kernel(WorldMapView v, const double* __restrict__ poses, const int* __restrict__ nptr,
                                                              double cell, int keep) {
  __shared__ int sflags;
  if (threadIdx.x == 0) sflags = 0;
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const Head h = head_of(v, nptr);
  int flags = 0;
  if (g < h.P) {                                                  // g < P <= point_capacity
    int slot = -1;
    const int r = row_of(v.m_offs, h.n, g);                       // 0 <= r < n <= keyframe_capacity
    double w[3];
    if (!world_of(poses + 12 * (size_t)r, v.m_xyz + 3 * (size_t)g, w)) {
      flags = WORLDMAP_SKIPPED;
    } else {
      u64 key = 0;
      if (!key_of(w, cell, &key)) {
        flags = WORLDMAP_RANGE;
      } else {
        const u64 T = (u64)1 << v.log2T;
        u64 at = home_slot(key, v.log2T);
        for (u64 step = 0; step < T; step++, at = (at + 1) & (T - 1)) {          // at most T steps: no input makes a lane spin
          const u64 prev = atomicCAS(&v.slots[2 * at], EMPTY, key);
          if (prev == EMPTY || prev == key) { slot = (int)at; break; }
        }
        if (slot < 0) {
          flags = WORLDMAP_TABLE;
        } else {
          atomicMin(&v.slots[2 * (size_t)slot + 1], keep ? ~(u64)g : (u64)g);
          atomicAdd(&v.cnt[slot], 1);
        }
      }
    }
    v.slot_of[g] = slot;
  }
  if (flags) atomicOr(&sflags, flags);
  __syncthreads();
  if (threadIdx.x == 0 && sflags) atomicOr(&v.ctl[0], sflags);
}

__global__ __launch_bounds__(256) void worldmap_count_kernel(WorldMapView v, const int* __restrict__ nptr, int min_count, int keep) {
  __shared__ int srow[4], sval[4];
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const Head h = head_of(v, nptr);
  bool valid;
  int slot;
  const bool row = is_row(v, g, h.P, min_count, keep, &valid, &slot);
  const int nrow = __popcll(__ballot(row)), nval = __popcll(__ballot(valid));
  if ((threadIdx.x & 63) == 0) { srow[threadIdx.x >> 6] = nrow; sval[threadIdx.x >> 6] = nval; }
  __syncthreads();
  if (threadIdx.x == 0) {
    v.blk[blockIdx.x] = srow[0] + srow[1] + srow[2] + srow[3];
    v.blk[(size_t)((v.nblk + 3) & ~3) + blockIdx.x] = sval[0] + sval[1] + sval[2] + sval[3];
  }
}

__global__ __launch_bounds__(256) void worldmap_scan_kernel(WorldMapView v, const int* __restrict__ nptr, int64_t* __restrict__ info) {
  if (blockIdx.x != 0) return;
  __shared__ int wsum[4];
  __shared__ int64_t vsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Head h = head_of(v, nptr);
  const int nb = (int)((h.P + 255) >> 8);                        // <= nblk
  const int* bval = v.blk + ((v.nblk + 3) & ~3);
  int carry = 0;                                                  // rows in front of this chunk (<= point_capacity <= 2^29)
  int64_t nvalid = 0;
  for (int base = 0; base < nb; base += 1024) {
    const int i0 = base + 4 * tid;
    int a[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      a[j] = i0 + j < nb ? v.blk[i0 + j] : 0;
      nvalid += i0 + j < nb ? bval[i0 + j] : 0;
    }
    const int mine = a[0] + a[1] + a[2] + a[3];
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int off = carry;
    for (int w = 0; w < wave; w++) off += wsum[w];
    const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    int at = off + incl - mine;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (i0 + j < nb) v.blk[i0 + j] = at;
      at += a[j];
    }
    carry += total;
    __syncthreads();                                              // wsum is rewritten by the next chunk
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) nvalid += __shfl_down(nvalid, d);
  if (lane == 0) vsum[wave] = nvalid;
  __syncthreads();
  if (tid == 0) {
    const int64_t qualifying = carry, rows = qualifying < v.ocap ? qualifying : v.ocap;
    const int flags = v.ctl[0] | (qualifying > v.ocap ? WORLDMAP_OVERFLOW : 0);
    v.state[0] = (int)rows; v.state[1] = flags; v.state[2] = 0; v.state[3] = 0;
    info[0] = rows; info[1] = qualifying; info[2] = vsum[0] + vsum[1] + vsum[2] + vsum[3]; info[3] = flags;
  }
}

__global__ __launch_bounds__(256) void worldmap_emit_kernel(WorldMapView v, const double* __restrict__ poses, const int* __restrict__ nptr,
                                                            int min_count, int keep) {
  __shared__ int srow[4];
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const Head h = head_of(v, nptr);
  if ((int64_t)blockIdx.x * 256 >= h.P) return;                   // the whole block: its prefix was not scanned
  bool valid;
  int slot;
  const bool row = is_row(v, g, h.P, min_count, keep, &valid, &slot);
  const u64 mask = __ballot(row);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) srow[wave] = __popcll(mask);
  __syncthreads();
  if (!row) return;
  int64_t j = v.blk[blockIdx.x] + __popcll(mask & (((u64)1 << lane) - 1));
  for (int w = 0; w < wave; w++) j += srow[w];
  if (j >= v.ocap) return;                                        // j < out_capacity: inside the five output arrays
  const int r = row_of(v.m_offs, h.n, g);
  double w[3];
  (void)world_of(poses + 12 * (size_t)r, v.m_xyz + 3 * (size_t)g, w);
  v.xyz[3 * j] = w[0]; v.xyz[3 * j + 1] = w[1]; v.xyz[3 * j + 2] = w[2];
  v.inten[j] = v.m_inten[g];
  v.src[j] = g;
  v.row[j] = r;
  v.count[j] = v.cnt[slot];
}

}  // namespace

hipError_t launch_worldmap_fuse(hipStream_t st, const WorldMapView& v, const double* poses, const int* n, double cell, int min_count,
                                int keep, int64_t* info) {
  const size_t T = (size_t)1 << v.log2T;
  hipError_t e = hipMemsetAsync(v.slots, 0xFF, T * 16, st);
  if (e == hipSuccess) e = hipMemsetAsync(v.cnt, 0, T * 4 + 16, st);           // cnt and ctl are adjacent
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)v.nblk), block(256);
  hipLaunchKernelGGL(worldmap_insert_kernel, grid, block, 0, st, v, poses, n, cell, keep);
  hipLaunchKernelGGL(worldmap_count_kernel, grid, block, 0, st, v, n, min_count, keep);
  hipLaunchKernelGGL(worldmap_scan_kernel, dim3(1), block, 0, st, v, n, info);
  hipLaunchKernelGGL(worldmap_emit_kernel, grid, block, 0, st, v, poses, n, min_count, keep);
  return hipGetLastError();
}

}  // namespace pr
