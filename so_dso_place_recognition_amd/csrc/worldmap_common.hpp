// worldmap_common.hpp — steps 1 and 2 of the world map's rule (include/place_recognition.h) as inlined device code: the
// world position of a map point under its pose row, its voxel key and the key's home slot.  worldmap.hip (the rebuild) and mapgrow.hip
// (one keyframe at a time) include it, so both run the same instructions on the same inputs and leave the same bits.  Both files are built
// with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pr {
namespace worldmap_dev {

typedef unsigned long long u64;

constexpr u64 EMPTY = ~(u64)0;
constexpr double CELL_LIM = 1048576.0;                           // 2^20

// step 1 and the finiteness half of step 2
__device__ __forceinline__ bool world_of(const double* __restrict__ pose, const double* __restrict__ p, double w[3]) {
  double q[12];
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 12; i++) { q[i] = pose[i]; fin = fin && __builtin_isfinite(q[i]); }
  const double d0 = p[0] - q[3], d1 = p[1] - q[7], d2 = p[2] - q[11];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    w[a] = (q[a] * d0 + q[4 + a] * d1) + q[8 + a] * d2;
    fin = fin && __builtin_isfinite(w[a]);
  }
  return fin;
}

// the range half of step 2 and the key: false when a c_a = floor(w_a / cell) lies outside [-2^20, 2^20), compared as a double
__device__ __forceinline__ bool key_of(const double w[3], double cell, u64* key) {
  const double c0 = floor(w[0] / cell), c1 = floor(w[1] / cell), c2 = floor(w[2] / cell);
  const bool in = c0 >= -CELL_LIM && c0 < CELL_LIM && c1 >= -CELL_LIM && c1 < CELL_LIM && c2 >= -CELL_LIM && c2 < CELL_LIM;
  if (in) *key = ((u64)((int64_t)c0 + 1048576) << 42) | ((u64)((int64_t)c1 + 1048576) << 21) | (u64)((int64_t)c2 + 1048576);
  return in;
}

__device__ __forceinline__ u64 home_slot(u64 key, int log2T) { return (key * 0x9E3779B97F4A7C15ull) >> (64 - log2T); }

}  // namespace worldmap_dev
}  // namespace pr
