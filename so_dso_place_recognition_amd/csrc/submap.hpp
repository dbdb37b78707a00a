// submap.hpp — what submap.hip (the kernels) and submap.cpp (the C ABI) of the local submaps share.  The finiteness test,
// the clamp and the pose load are trajeval.hpp's (namespace traj), which holds their only copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int SUBMAP_TRUNCATED = 1, SUBMAP_NO_CENTER = 2, SUBMAP_OVERFLOW = 4;      // = PR_SUBMAP_*
constexpr int SUBMAP_T = 256;                // threads of every workgroup
constexpr int SUBMAP_MAX_W = 31;             // 2 w + 1 <= 63: a lane of the plan's wave per walked row
constexpr int SUBMAP_MAX_CHUNKS = 4;         // most workgroups that share the points of one (slot, entry)

// The create sizes and the scratch of a pr_submap (all allocated by pr_submap_create); L = 2 w_max + 1 entries per slot, in walk order.
//   row   [slot_capacity][L] i32   the map row of the entry
//   dst   [slot_capacity][L] i32   where the entry's points start inside the slot; -1: the entry is not taken
//   len   [slot_capacity][L] i32   its points
//   src   [slot_capacity][L] i64   where they start in the map's xyz
//   total, flags, taken [slot_capacity] i32   the slot's points, flags and rows taken, before placement
//   base  [slot_capacity] i64      where the slot starts in out_xyz; -1: not placed (overflow, or p >= c)
struct SubmapView {
  int slot_capacity, w_max, L, max_cloud_points, keyframe_capacity, chunks;
  long long point_capacity;
  int* row; int* dst; int* len; long long* src; int* total; int* flags; int* taken; long long* base;
};

struct SubmapParams { int w, past_only, avoid_gap, max_pts; };

struct SubmapIn {
  const double* xyz; const long long* offs; const double* poses; const int* n; const int* center; const int* avoid;   // avoid may be NULL
  int c;
};

struct SubmapOut { double* xyz; long long* offs; int* rows; int* info; };

inline int submap_chunks(int max_cloud_points) {
  const int ch = (max_cloud_points + SUBMAP_T - 1) / SUBMAP_T;
  return ch < 1 ? 1 : (ch > SUBMAP_MAX_CHUNKS ? SUBMAP_MAX_CHUNKS : ch);
}

void launch_submap(hipStream_t st, const SubmapView& v, const SubmapIn& in, const SubmapParams& prm, const SubmapOut& out);

}  // namespace pr
