// proximity.hpp — what proximity.hip (the kernels) and proximity.cpp (the C ABI) of the pose-proximity candidate search share
// (DESIGN.md 4.27).  The rigid products and the finiteness test are trajeval.hpp's (namespace traj), which holds their only copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int PROX_QRANGE_CLAMPED = 1;       // = PR_PROXIMITY_QRANGE_CLAMPED
constexpr int PROX_T = 256;                  // threads of every workgroup = blocks of the path-length prefix
constexpr int PROX_ROWS = 16;                // query rows of a search workgroup: 4 waves of PROX_RPW rows
constexpr int PROX_RPW = 4;                  // rows whose lists one wave keeps in its registers
constexpr int PROX_COLS = 256;               // DB rows of a slab (staged through LDS once per tile)
constexpr int PROX_MAX_K = 32;
constexpr int PROX_MAX_RUNS = 16;            // most runs the DB range of a tile is cut into
constexpr int PROX_FEW_TILES = 128;          // from this many tiles on a tile walks its DB range in one run

// The create sizes and the scratch of a pr_proximity (all allocated by pr_proximity_create).
//   cen    [node_capacity][3] f64   camera centres (zeros for a row that is not valid)
//   axis   [node_capacity][3] f64   viewing axes (row 2 of R)
//   s      [node_capacity] f64      path length over the valid rows, blocked order
//   valid  [node_capacity] i32      1: the row is < n and its 12 entries are finite
//   part_d2 / part_idx [query_capacity][runs][k_max]   every run's list of a searched row, ascending, empty = +Inf / INT_MAX
struct ProxView {
  int node_capacity, query_capacity, k_max, runs;
  double* cen; double* axis; double* s; int* valid; double* part_d2; int* part_idx;
};

struct ProxParams {
  double radius, growth, radius_max, cos_min;
  int min_gap, stride, k, known_window;
};

struct ProxIn {
  const double* poses; const int* n; const int* qrange;
  const int* e_ij; const int* e_state; int log_edge_capacity;    // the closure log, or two NULLs and 0
};

struct ProxOut {
  int* idx; double* d2; double* T0; int* pair_src; int* pair_dst; unsigned char* known; int* info;
};

inline int prox_tiles(int query_capacity) { return (query_capacity + PROX_ROWS - 1) / PROX_ROWS; }
// the runs of a handle: a create size, so that every grid depends on the create sizes only
inline int prox_runs(int node_capacity, int query_capacity) {
  if (prox_tiles(query_capacity) >= PROX_FEW_TILES) return 1;
  const int slabs = (node_capacity + PROX_COLS - 1) / PROX_COLS;
  return slabs < PROX_MAX_RUNS ? slabs : PROX_MAX_RUNS;
}

void launch_proximity(hipStream_t st, const ProxView& v, const ProxIn& in, const ProxParams& prm, const ProxOut& out);

}  // namespace pr
