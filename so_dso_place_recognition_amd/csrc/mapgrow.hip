// mapgrow.hip — the world map, the localiser's voxel index and the world-map normals grown by ONE keyframe a call (no
// reference counterpart).  A fuse with keep = 0 and min_count = 1 leaves the world rows as a subsequence of the map's points in map order,
// so a new keyframe's new voxels are new rows at the end, its points in known voxels only raise a count, the index only gains keys, and a
// normal changes only for the rows the index holds in the 27 voxels around a new row.  The contract is the rebuild's bytes (the rule:
// include/place_recognition.h; restated with a dict, without hashing, in tests/mapgrow_np.py).  Every launch's grid depends on the map's
// max_cloud_points only; the row, the counts and every decision - the refusals included - are read and made on the device, by every
// kernel from the same words, which only the last launch of a call (finish) changes.  Compiled with -ffp-contract=off.
//
//   sync     one lane: fused, rows_seen and the empty range.
//   insert   one lane per point slot of max_cloud_points: world_of and key_of of worldmap_common.hpp (the rebuild's own code), the home
//            slot in the LOCALISER's table, a linear probe with a 64-bit compare-and-swap on the key - at most T steps, then WORLDMAP_TABLE
//            -, and an unsigned minimum of TAG | i on the row word.  An old row (< out_capacity < TAG) survives the minimum: the voxel is
//            known.  Otherwise the word ends as TAG | the smallest point of the voxel: its representative.  The slot goes to slot_of[i].
//   blocks   per 256 points: how many lanes are the representative of a new voxel, how many are valid.
//   scan     ONE workgroup: the exclusive prefix of the block counts in chunks of 1024, in order; the totals for finish.
//   emit     a representative's place by ballots, row R + place: below out_capacity the five world stores (w recomputed by the same
//            inlined code: the same bits), count = 0 and the row into the table; past it the row word becomes all ones, which every lookup
//            of maploc.hip and mapplane_normal.hpp reads as "no row".
//   count    every valid point adds one to the count of the row its slot holds - an old row or the one emit stored.
//   finish   one lane: world.state, the localiser's rows indexed and one-cloud target, the handle's words, info.
//   A key that finds no slot (WORLDMAP_TABLE; only a call with more than T - R >= out_capacity new voxels can fill the table) makes the
//   call a refusal: emit and count store nothing, the call's keys stay in the table without a row.
//   normals  one lane per (row of the last range, one of the 27 keys around it): mapplane_normal.hpp's row_normal of the row the table
//            holds for that key.  Several lanes may recompute one row; they store equal bytes.
// Integer atomics and integer scans only; no kernel waits for another workgroup; every probe is a bounded for loop; a row word is compared
// with out_capacity before an address is formed.  Plain C++, vector stores only, no floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "mapplane_normal.hpp"
#include "worldmap_common.hpp"

namespace pr {
namespace {

using namespace worldmap_dev;

constexpr u64 TAG = (u64)1 << 62;                                 // a row word >= TAG: a voxel of this call (all ones included)

__device__ __forceinline__ int64_t clampi(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// what a call does, from words that no launch before finish changes.  go: 0 off, 1 extend, 2 refused
struct Plan { int go, r, flags; int64_t R, g0, g1; };

__device__ __forceinline__ Plan plan_of(const MapGrowView& v, const int* __restrict__ rowp) {
  Plan p;
  p.r = rowp[0];
  p.R = clampi(v.w.state[0], 0, v.w.ocap);                        // a scribbled count must not turn into a row outside the buffers
  p.flags = 0; p.g0 = 0; p.g1 = 0;
  if (p.r < 0) { p.go = 0; return p; }
  const int n = (int)clampi(v.w.m_state[0], 0, v.w.kcap);
  if (p.r != v.ctl[MG_FUSED] || p.r >= n) p.flags |= MAPGROW_ORDER;
  if (p.R != (int64_t)v.ctl[MG_SEEN]) p.flags |= MAPGROW_STALE;
  if (v.w.state[1] & WORLDMAP_OVERFLOW) p.flags |= MAPGROW_FULL;
  if (p.flags) { p.go = 2; return p; }
  p.go = 1;                                                       // 0 <= r < n <= keyframe_capacity: offs[r + 1] exists
  const int64_t P = clampi(v.w.m_offs[p.r + 1], 0, v.w.pcap);     // the fuse's P at n = r + 1
  p.g0 = clampi(v.w.m_offs[p.r], 0, P);
  p.g1 = P - p.g0 > (int64_t)v.mcp ? p.g0 + v.mcp : P;            // (a stored cloud has at most max_cloud_points points)
  return p;
}

// the call's pose row (go == 1: 0 <= r < keyframe_capacity); the host form stages that row alone
__device__ __forceinline__ const double* pose_of(const double* __restrict__ poses, int pose_is_row, int r) {
  return pose_is_row ? poses : poses + 12 * (size_t)r;
}

__global__ __launch_bounds__(64) void mapgrow_sync_kernel(MapGrowView v, const int* __restrict__ nptr) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int R = (int)clampi(v.w.state[0], 0, v.w.ocap);
  v.ctl[MG_FUSED] = (int)clampi(nptr[0], 0, v.w.kcap);
  v.ctl[MG_SEEN] = R; v.ctl[MG_A] = R; v.ctl[MG_B] = R;
  v.ctl[MG_FLAGS] = 0; v.ctl[MG_NEW] = 0; v.ctl[MG_VALID] = 0;
}

__global__ __launch_bounds__(256) void mapgrow_insert_kernel(MapGrowView v, const double* __restrict__ poses, int pose_is_row,
                                                             const int* __restrict__ rowp) {
  __shared__ int sflags;
  if (threadIdx.x == 0) sflags = 0;
  __syncthreads();
  const Plan p = plan_of(v, rowp);
  const int i = blockIdx.x * 256 + threadIdx.x;                   // < nblk * 256
  const int64_t g = p.g0 + i;
  int flags = 0;
  if (p.go == 1 && i < v.mcp && g < p.g1) {                       // g < g1 <= point_capacity; i < max_cloud_points
    int slot = -1;
    double w[3];
    u64 key = 0;
    const double* pose = pose_of(poses, pose_is_row, p.r);
    if (!world_of(pose, v.w.m_xyz + 3 * (size_t)g, w)) {
      flags = WORLDMAP_SKIPPED;
    } else if (!key_of(w, v.cell, &key)) {
      flags = WORLDMAP_RANGE;
    } else {
      const u64 T = (u64)1 << v.log2T;
      u64 at = home_slot(key, v.log2T);
      for (u64 step = 0; step < T; step++, at = (at + 1) & (T - 1)) {            // at most T steps: no input makes a lane spin
        const u64 prev = atomicCAS(&v.table[2 * at], EMPTY, key);
        if (prev == EMPTY || prev == key) { slot = (int)at; break; }
      }
      if (slot < 0) flags = WORLDMAP_TABLE;
      else atomicMin(&v.table[2 * (size_t)slot + 1], TAG | (u64)i);              // an old row word is below TAG and stays
    }
    v.slot_of[i] = slot;
  }
  if (flags) atomicOr(&sflags, flags);
  __syncthreads();
  if (threadIdx.x == 0 && sflags) atomicOr(&v.ctl[MG_FLAGS], sflags);
}

// is lane i the representative of a voxel this call found new; *slot: the point's slot or -1
__device__ __forceinline__ bool is_rep(const MapGrowView& v, const Plan& p, int i, int* slot) {
  const bool in = p.go == 1 && i < v.mcp && p.g0 + i < p.g1;
  const int s = in ? v.slot_of[i] : -1;
  *slot = s;
  return s >= 0 && v.table[2 * (size_t)s + 1] == (TAG | (u64)i);
}

__global__ __launch_bounds__(256) void mapgrow_blocks_kernel(MapGrowView v, const int* __restrict__ rowp) {
  __shared__ int srow[4], sval[4];
  const Plan p = plan_of(v, rowp);
  const int i = blockIdx.x * 256 + threadIdx.x;
  int slot;
  const bool rep = is_rep(v, p, i, &slot);
  const int nrow = __popcll(__ballot(rep)), nval = __popcll(__ballot(slot >= 0));
  if ((threadIdx.x & 63) == 0) { srow[threadIdx.x >> 6] = nrow; sval[threadIdx.x >> 6] = nval; }
  __syncthreads();
  if (threadIdx.x == 0) {
    v.blk[blockIdx.x] = srow[0] + srow[1] + srow[2] + srow[3];
    v.blk[(size_t)v.nblk + blockIdx.x] = sval[0] + sval[1] + sval[2] + sval[3];
  }
}

__global__ __launch_bounds__(256) void mapgrow_scan_kernel(MapGrowView v) {
  if (blockIdx.x != 0) return;
  __shared__ int wsum[4], vsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = v.nblk;
  const int* bval = v.blk + v.nblk;
  int carry = 0, nvalid = 0;                                      // both <= max_cloud_points <= 2^26
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
  if (tid == 0) { v.ctl[MG_NEW] = carry; v.ctl[MG_VALID] = vsum[0] + vsum[1] + vsum[2] + vsum[3]; }
}

__global__ __launch_bounds__(256) void mapgrow_emit_kernel(MapGrowView v, const double* __restrict__ poses, int pose_is_row,
                                                           const int* __restrict__ rowp) {
  __shared__ int srow[4];
  const Plan p = plan_of(v, rowp);
  const int i = blockIdx.x * 256 + threadIdx.x;
  int slot;
  const bool rep = is_rep(v, p, i, &slot);
  const u64 mask = __ballot(rep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) srow[wave] = __popcll(mask);
  __syncthreads();
  if (!rep) return;
  int64_t j = p.R + v.blk[blockIdx.x] + __popcll(mask & (((u64)1 << lane) - 1));
  for (int w = 0; w < wave; w++) j += srow[w];
  if (j >= v.w.ocap || (v.ctl[MG_FLAGS] & WORLDMAP_TABLE)) {      // not stored: the key stays in the table without a row
    v.table[2 * (size_t)slot + 1] = EMPTY;
    return;
  }
  const int64_t g = p.g0 + i;                                     // j < out_capacity: inside the five output arrays
  double w[3];
  (void)world_of(pose_of(poses, pose_is_row, p.r), v.w.m_xyz + 3 * (size_t)g, w);
  v.w.xyz[3 * j] = w[0]; v.w.xyz[3 * j + 1] = w[1]; v.w.xyz[3 * j + 2] = w[2];
  v.w.inten[j] = v.w.m_inten[g];
  v.w.src[j] = g;
  v.w.row[j] = p.r;
  v.w.count[j] = 0;                                               // the count launch adds the voxel's points
  v.table[2 * (size_t)slot + 1] = (u64)j;
}

__global__ __launch_bounds__(256) void mapgrow_count_kernel(MapGrowView v, const int* __restrict__ rowp) {
  const Plan p = plan_of(v, rowp);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (!(p.go == 1 && i < v.mcp && p.g0 + i < p.g1) || (v.ctl[MG_FLAGS] & WORLDMAP_TABLE)) return;
  const int s = v.slot_of[i];
  if (s < 0) return;
  const u64 j = v.table[2 * (size_t)s + 1];
  if (j < (u64)v.w.ocap) atomicAdd(&v.w.count[j], 1);             // (a voxel past out_capacity holds all ones) j < out_capacity
}

__global__ __launch_bounds__(64) void mapgrow_finish_kernel(MapGrowView v, const int* __restrict__ rowp, int64_t* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const Plan p = plan_of(v, rowp);
  if (p.go != 1) {
    info[0] = 0; info[1] = p.R; info[2] = 0; info[3] = p.flags;
    if (p.go == 2) v.ctl[MG_LAST] = p.flags;
    return;
  }
  if (v.ctl[MG_FLAGS] & WORLDMAP_TABLE) {                         // a key found no slot: the rows could not be the rebuild's, so none was stored
    info[0] = 0; info[1] = p.R; info[2] = 0; info[3] = v.ctl[MG_FLAGS];
    v.ctl[MG_LAST] = v.ctl[MG_FLAGS]; v.ctl[MG_FLAGS] = 0;
    return;
  }
  const int64_t fresh = v.ctl[MG_NEW], want = p.R + fresh;
  const int64_t R2 = want < v.w.ocap ? want : v.w.ocap, stored = R2 - p.R;
  const int flags = v.ctl[MG_FLAGS] | (want > v.w.ocap ? WORLDMAP_OVERFLOW : 0);
  v.w.state[0] = (int)R2; v.w.state[1] = v.w.state[1] | flags; v.w.state[2] = 0; v.w.state[3] = 0;
  v.ml_ctl[1] = v.ml_ctl[1] + (int)stored;
  v.offs2[0] = 0; v.offs2[1] = R2;
  v.ctl[MG_FUSED] = p.r + 1; v.ctl[MG_SEEN] = (int)R2; v.ctl[MG_A] = (int)p.R; v.ctl[MG_B] = (int)R2;
  info[0] = stored; info[1] = R2; info[2] = v.ctl[MG_VALID]; info[3] = flags;
  v.ctl[MG_FLAGS] = 0; v.ctl[MG_LAST] = flags;
}

__global__ __launch_bounds__(256) void mapgrow_normals_kernel(MapGrowView v, mapplane_dev::TableView tv, double r2, int min_nbrs,
                                                               double max_ratio, double* __restrict__ normals, int* __restrict__ ninfo,
                                                               int* __restrict__ out_rows) {
  const int64_t L = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (L >= 27 * (int64_t)v.mcp) return;
  const int64_t R = clampi(v.w.state[0], 0, v.w.ocap);
  const int64_t a = clampi(v.ctl[MG_A], 0, R), b = clampi(v.ctl[MG_B], a, R);
  const int64_t src = a + L / 27;
  if (src >= b) return;                                           // src < b <= R <= out_capacity
  const int k = (int)(L % 27), d0 = k / 9 - 1, kk = k % 9;
  const double* q = v.w.xyz + 3 * (size_t)src;
  const double x[3] = {q[0], q[1], q[2]};
  int f[3];
  u64 row = EMPTY;
  if (mapplane_dev::finite3(x[0], x[1], x[2]) && mapplane_dev::voxel_of(x, tv.cell, f))
    row = mapplane_dev::held_row(tv, (unsigned)(f[0] + d0), (unsigned)(f[1] + (kk / 3 - 1)), (unsigned)(f[2] + (kk % 3 - 1)));
  const bool on = row < (u64)v.w.ocap;                            // (EMPTY included) row < out_capacity before an address is formed
  if (out_rows) out_rows[L] = on ? (int)row : -1;
  if (!on) return;
  double n[3];
  int info;
  mapplane_dev::row_normal(tv, (int64_t)row, R, r2, min_nbrs, max_ratio, n, &info);
  const size_t o = out_rows ? (size_t)L : (size_t)row;
  normals[3 * o] = n[0]; normals[3 * o + 1] = n[1]; normals[3 * o + 2] = n[2];
  ninfo[o] = info;
}

}  // namespace

void launch_mapgrow_sync(hipStream_t st, const MapGrowView& v, const int* n) {
  hipLaunchKernelGGL(mapgrow_sync_kernel, dim3(1), dim3(64), 0, st, v, n);
}

void launch_mapgrow_extend(hipStream_t st, const MapGrowView& v, const double* poses, int pose_is_row, const int* row, int64_t* info) {
  const dim3 grid((unsigned)v.nblk), block(256);
  hipLaunchKernelGGL(mapgrow_insert_kernel, grid, block, 0, st, v, poses, pose_is_row, row);
  hipLaunchKernelGGL(mapgrow_blocks_kernel, grid, block, 0, st, v, row);
  hipLaunchKernelGGL(mapgrow_scan_kernel, dim3(1), block, 0, st, v);
  hipLaunchKernelGGL(mapgrow_emit_kernel, grid, block, 0, st, v, poses, pose_is_row, row);
  hipLaunchKernelGGL(mapgrow_count_kernel, grid, block, 0, st, v, row);
  hipLaunchKernelGGL(mapgrow_finish_kernel, dim3(1), dim3(64), 0, st, v, row, info);
}

void launch_mapgrow_normals(hipStream_t st, const MapGrowView& v, double r2, int min_nbrs, double max_ratio, double* normals, int* ninfo,
                            int* out_rows) {
  const mapplane_dev::TableView tv{reinterpret_cast<const ulonglong2*>(v.table), v.w.xyz, v.w.state, v.w.ocap, v.cell, v.log2T};
  const int64_t lanes = 27 * (int64_t)v.mcp;
  hipLaunchKernelGGL(mapgrow_normals_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, v, tv, r2, min_nbrs, max_ratio, normals,
                     ninfo, out_rows);
}

}  // namespace pr
