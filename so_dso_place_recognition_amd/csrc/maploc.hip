// maploc.hip — scan-to-map registration against the world map (no reference counterpart): ONE voxel hash index over the
// rows a pr_worldmap fuse left in the caller's buffers, shared by every pair of a call, an exact correspondence search through it and the
// ICP update of icp.hip on the same code.  Every launch's grid depends on the create sizes and c only; the row count and every decision
// are read and made on the device, so one captured index / refine serves every count.  Compiled with -ffp-contract=off.
//
// The rule (normative: include/place_recognition.h; restated in fp64, without hashing, in tests/maploc_np.py).
//   index   R = state[0] clamped into 0 .. out_capacity.  Row j < R is indexed iff its coordinates are finite (else MAPLOC_SKIPPED), every
//           c_a = floor(x_a / cell) - IEEE division, compared as a double before any conversion - lies in [-2^20, 2^20) (else
//           MAPLOC_RANGE) and it is the smallest j of its key; key = worldmap.hip's packing.  A key held by more than one row sets
//           MAPLOC_DUPLICATE.  offs2 = {0, R}, info = {rows indexed, R, flags, 0}.
//   probe   p' = icp_common.hpp's transform(T, s); no correspondent when p' is not finite or a t_a = p'_a / cell lies outside
//           [-2^20 - 1, 2^20 + 1) (tested in floating point).  Candidates: the indexed rows whose voxel differs from floor(t) by at most
//           1 per axis (27 keys, those outside the 21-bit range dropped) and whose world.row is not inside the pair's exclusion window;
//           d2 = ((dx dx) + dy dy) + dz dz, "smaller d2, then smaller j", masked to d2 < mc2: (j, d2) or (-1, +Inf).
//   seed    T0 = inv(P_idx) o T_rel in the association the header states.
//
//   clear   two memsets: the table's (key, row) pairs to all ones - no key has bit 63, and ~0 is the identity of the unsigned minimum -
//           and the control block to zero.
//   index   one lane per row of out_capacity: the key, the home slot (key * 0x9E3779B97F4A7C15) >> (64 - log2 T), a linear probe with a
//           64-bit compare-and-swap on the key - at most T steps, then MAPLOC_TABLE: no input makes a lane spin, and with T >= 2
//           out_capacity the table is never more than half full -, an unsigned minimum on the row word.  A lane that claimed an empty slot
//           counts one indexed row; flags and counts are summed per workgroup in LDS, then one integer atomic each.
//   finish  one lane: offs2 and info (a launch of its own behind index: no workgroup waits for another).
//   probe   grid (chunks of 256 source points, c): the 27 lookups in three batches of 9 whose home-slot (key, row) pairs - ONE 16-byte
//           load each - are all issued before the first compare; a lookup ends at its key, at an empty slot or after T steps.  Then
//           icp_common.hpp's chunk_sums: the code the grid probe and the brute-force combining launch run.
//   seed    one lane per pair.
// A row word comes from this file's own index, which stores only j < R <= out_capacity, and is compared with out_capacity again before an
// address is formed: a stale index can return stale rows, never an address outside xyz[0 .. out_capacity).  Integer atomics only, plain
// C++, vector stores.
#include "icp_common.hpp"
#include "kernels.hpp"

namespace pr {
namespace {

using namespace icp_dev;

typedef unsigned long long u64;

constexpr u64 EMPTY = ~(u64)0;
constexpr double CELL_LIM = 1048576.0;                           // 2^20
constexpr long long CELL_BIAS = 1048576;

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// a coordinate's voxel along one axis: the formula of the containment argument, the one the index and the probe share
__device__ __forceinline__ double voxel_quot(double x, double cell) { return x / cell; }
__device__ __forceinline__ double voxel_coord(double x, double cell) { return floor(voxel_quot(x, cell)); }

// three voxel indices in [-2^20, 2^20) -> the key, packed as worldmap.hip packs it (c_0 highest)
__device__ __forceinline__ u64 pack_key(long long c0, long long c1, long long c2) {
  return ((u64)(c0 + CELL_BIAS) << 42) | ((u64)(c1 + CELL_BIAS) << 21) | (u64)(c2 + CELL_BIAS);
}
__device__ __forceinline__ u64 home_slot(u64 key, int log2T) { return (key * 0x9E3779B97F4A7C15ull) >> (64 - log2T); }

__device__ __forceinline__ int64_t rows_of(const MapLocView& v) {
  const int64_t r = v.state[0];
  return r < 0 ? 0 : (r > v.ocap ? v.ocap : r);                  // a scribbled count must not turn into a row outside the buffers
}

__global__ __launch_bounds__(256) void maploc_index_kernel(MapLocView v) {
  __shared__ int sflags, scount;
  if (threadIdx.x == 0) { sflags = 0; scount = 0; }
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t R = rows_of(v);
  int flags = 0, mine = 0;
  if (j < R) {                                                    // j < R <= out_capacity
    const double* q = v.xyz + 3 * (size_t)j;
    const double x = q[0], y = q[1], z = q[2];
    if (!finite3(x, y, z)) {
      flags = MAPLOC_SKIPPED;
    } else {
      const double c0 = voxel_coord(x, v.cell), c1 = voxel_coord(y, v.cell), c2 = voxel_coord(z, v.cell);
      const bool in = c0 >= -CELL_LIM && c0 < CELL_LIM && c1 >= -CELL_LIM && c1 < CELL_LIM && c2 >= -CELL_LIM && c2 < CELL_LIM;
      if (!in) {
        flags = MAPLOC_RANGE;
      } else {
        const u64 key = pack_key((long long)c0, (long long)c1, (long long)c2);
        const u64 T = (u64)1 << v.log2T;
        u64 at = home_slot(key, v.log2T);
        bool placed = false;
        for (u64 step = 0; step < T; step++, at = (at + 1) & (T - 1)) {          // at most T steps: no input makes a lane spin
          const u64 prev = atomicCAS(&v.table[2 * at], EMPTY, key);
          if (prev == EMPTY) { mine = 1; placed = true; break; }
          if (prev == key) { flags = MAPLOC_DUPLICATE; placed = true; break; }
        }
        if (placed) atomicMin(&v.table[2 * at + 1], (u64)j);
        else flags = MAPLOC_TABLE;
      }
    }
  }
  if (flags) atomicOr(&sflags, flags);
  if (mine) atomicAdd(&scount, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sflags) atomicOr(&v.ctl[0], sflags);
    if (scount) atomicAdd(&v.ctl[1], scount);                     // <= out_capacity <= 2^29
  }
}

__global__ __launch_bounds__(64) void maploc_index_finish_kernel(MapLocView v, int64_t* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t R = rows_of(v);
  v.offs2[0] = 0; v.offs2[1] = R;
  info[0] = v.ctl[1]; info[1] = R; info[2] = v.ctl[0]; info[3] = 0;
}

// what a pass needs of the handle, by value in the kernel arguments
struct ProbeView { const ulonglong2* tab; const double* xyz; const int* row; int64_t ocap; double cell; int log2T, ld, nchunks; };

// grid (chunks of 256 source points, pairs)
__global__ __launch_bounds__(IC_THREADS) void maploc_probe_kernel(ProbeView v, IcpClouds A, const double* __restrict__ T,
                                                                   const int32_t* __restrict__ excl, const int* __restrict__ done,
                                                                   const long long* __restrict__ base, double* __restrict__ nn_d,
                                                                   int* __restrict__ nn_j, double mc2, double* __restrict__ part) {
  __shared__ double red[IC_THREADS / 64][ICP_PARTIAL];
  const int pair = blockIdx.y;
  if (done && done[pair]) return;
  PairShape S;
  if (!pair_shape(A, pair, S)) return;
  const int i0 = blockIdx.x * IC_THREADS, i = i0 + threadIdx.x;
  if (i0 >= S.ns) return;
  double bd = INFINITY;
  int bj = -1;
  if (i < S.ns) {
    const double* s = A.xyz_q + 3 * (size_t)(S.q0 + i);
    double p[3];
    transform(T + 12 * (size_t)pair, s[0], s[1], s[2], p);
    bool ok = finite3(p[0], p[1], p[2]);
    int f[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double t = voxel_quot(p[a], v.cell);                   // the range test in floating point: 1e300 never reaches an integer
      const bool in = t >= -(CELL_LIM + 1.0) && t < CELL_LIM + 1.0;     // (a NaN fails)
      ok = ok && in;
      f[a] = in ? (int)floor(t) + (int)CELL_BIAS : 0;              // biased: 2^20 is voxel 0, the indexed range is [0, 2^21)
    }
    if (ok) {
      int elo = 0, ehi = -1;                                       // lo > hi: excludes nothing
      if (excl) { elo = excl[2 * (size_t)pair]; ehi = excl[2 * (size_t)pair + 1]; }
      const ulonglong2* __restrict__ tab = v.tab;
      const u64 Tn = (u64)1 << v.log2T, mask = Tn - 1;
      const int sh = 64 - v.log2T;
      for (int d0 = -1; d0 <= 1; d0++) {
        const unsigned c0 = (unsigned)(f[0] + d0);                   // (a voxel below the range wraps to a large unsigned)
        u64 key[9], at[9];
        u64 ex[9], ey[9];                                           // (two scalar arrays: a ulonglong2 array is not promoted to registers)
#pragma unroll
        for (int k = 0; k < 9; k++) {                               // the nine home-slot loads are issued before the first compare
          const unsigned c1 = (unsigned)(f[1] + (k / 3 - 1)), c2 = (unsigned)(f[2] + (k % 3 - 1));
          const bool val = c0 < 2097152u && c1 < 2097152u && c2 < 2097152u;
          key[k] = val ? ((u64)c0 << 42) | ((u64)c1 << 21) | (u64)c2 : EMPTY;
          at[k] = (key[k] * 0x9E3779B97F4A7C15ull) >> sh;
          const ulonglong2 e = tab[at[k]];                            // (key, row): one 16-byte load
          ex[k] = e.x; ey[k] = e.y;
        }
#pragma unroll
        for (int k = 0; k < 9; k++) {
          u64 j = EMPTY;
          u64 cx = ex[k], cy = ey[k], a = at[k];
          for (u64 step = 0; step < Tn; step++) {                   // ends at an empty slot, at the key or after T steps
            if (cx == EMPTY) break;                                 // (a key outside the range is EMPTY itself: no row)
            if (cx == key[k]) { j = cy; break; }
            a = (a + 1) & mask;
            const ulonglong2 e = tab[a];
            cx = e.x; cy = e.y;
          }
          if (j >= (u64)v.ocap) continue;                           // (EMPTY included) j < out_capacity before an address is formed
          if (excl) {
            const int r = v.row[j];
            if (elo <= r && r <= ehi) continue;
          }
          const double* q = v.xyz + 3 * (size_t)j;
          const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
          const double d = ((dx * dx) + dy * dy) + dz * dz;
          if (d < bd || (d == bd && (int)j < bj)) { bd = d; bj = (int)j; }
        }
      }
    }
    if (!(bd < mc2)) { bd = INFINITY; bj = -1; }
    const size_t row = base ? (size_t)base[pair] : (size_t)pair * v.ld;
    nn_d[row + i] = bd;
    nn_j[row + i] = bj;
  }
  if (part) chunk_sums(A, S, T, pair, i, i < S.ns, bd, bj, mc2, red, part + ((size_t)pair * v.nchunks + blockIdx.x) * ICP_PARTIAL);
}

__global__ __launch_bounds__(64) void maploc_seed_kernel(const double* __restrict__ poses, const int* __restrict__ nptr, int kcap,
                                                          const int32_t* __restrict__ idx, const unsigned char* __restrict__ accepted,
                                                          const double* __restrict__ T_rel, const int32_t* __restrict__ src, int c,
                                                          double* __restrict__ T0, int32_t* __restrict__ pair_src) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= c) return;
  int n = nptr[0];
  n = n < 0 ? 0 : (n > kcap ? kcap : n);                          // a scribbled count must not turn into a row outside the poses
  const int r = idx[p];
  bool on = r >= 0 && r < n && (!accepted || accepted[p] != 0);
  double P[12], Tr[12];
#pragma unroll
  for (int k = 0; k < 12; k++) { P[k] = 0.0; Tr[k] = 0.0; }
  if (on) {
#pragma unroll
    for (int k = 0; k < 12; k++) { P[k] = poses[12 * (size_t)r + k]; on = on && isfinite(P[k]); }
  }
  if (on && T_rel) {
#pragma unroll
    for (int k = 0; k < 12; k++) { Tr[k] = T_rel[12 * (size_t)p + k]; on = on && isfinite(Tr[k]); }
  }
  double out[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  if (on) {
    double Ri[3][3], ti[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
      for (int b = 0; b < 3; b++) Ri[a][b] = P[4 * b + a];
      ti[a] = -((P[a] * P[3] + P[4 + a] * P[7]) + P[8 + a] * P[11]);
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (!T_rel) {
#pragma unroll
        for (int b = 0; b < 3; b++) out[4 * a + b] = Ri[a][b];
        out[4 * a + 3] = ti[a];
      } else {
#pragma unroll
        for (int b = 0; b < 3; b++) out[4 * a + b] = (Ri[a][0] * Tr[b] + Ri[a][1] * Tr[4 + b]) + Ri[a][2] * Tr[8 + b];
        out[4 * a + 3] = ((Ri[a][0] * Tr[3] + Ri[a][1] * Tr[7]) + Ri[a][2] * Tr[11]) + ti[a];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 12; k++) T0[12 * (size_t)p + k] = out[k];
  pair_src[p] = on ? (src ? src[p] : p) : -1;
}

}  // namespace

hipError_t launch_maploc_index(hipStream_t st, const MapLocView& v, int64_t* info) {
  const size_t T = (size_t)1 << v.log2T;
  hipError_t e = hipMemsetAsync(v.table, 0xFF, T * 16, st);
  if (e == hipSuccess) e = hipMemsetAsync(v.ctl, 0, 16, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(maploc_index_kernel, dim3((unsigned)((v.ocap + 255) / 256)), dim3(256), 0, st, v);
  hipLaunchKernelGGL(maploc_index_finish_kernel, dim3(1), dim3(64), 0, st, v, info);
  return hipGetLastError();
}

void launch_maploc_probe(hipStream_t st, const MapLocView& v, const IcpClouds& A, const double* T, const int32_t* excl, const int* done,
                         const long long* base, double* nn_d, int* nn_j, double mc2, double* part) {
  if (A.c <= 0 || A.max_src <= 0) return;
  const ProbeView pv{reinterpret_cast<const ulonglong2*>(v.table), v.xyz, v.row, v.ocap, v.cell, v.log2T, v.ld, v.nchunks};
  hipLaunchKernelGGL(maploc_probe_kernel, dim3((A.max_src + IC_THREADS - 1) / IC_THREADS, A.c), dim3(IC_THREADS), 0, st, pv, A, T, excl, done, base,
                     nn_d, nn_j, mc2, part);
}

void launch_maploc_seed(hipStream_t st, const double* poses, const int* n, int kcap, const int32_t* idx, const unsigned char* accepted,
                        const double* T_rel, const int32_t* src, int c, double* T0, int32_t* pair_src) {
  if (c <= 0) return;
  hipLaunchKernelGGL(maploc_seed_kernel, dim3((c + 63) / 64), dim3(64), 0, st, poses, n, kcap, idx, accepted, T_rel, src, c, T0, pair_src);
}

}  // namespace pr
