// gate.hpp — what gate.hip (the kernels) and gate.cpp (the C ABI) of the closure consistency gate share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int GATE_SRC_OVERFLOW = 1;         // = PR_GATE_SRC_OVERFLOW
constexpr int GATE_UNSETTLED = 2;            // = PR_GATE_UNSETTLED
constexpr int GATE_LOG_OVERFLOW = 1;         // = PR_POSEGRAPH_OVERFLOW, the bit of the source log's state[1]
constexpr int GATE_TILE = 64;                // edges b of one LDS tile of a round
constexpr int GATE_LMN = 36;                 // doubles of one edge's L, M, N (12 each, [R | t] row-major)

// The two logs' caller-owned buffers (src is only read), the create sizes and the scratch of a pr_gate (all allocated by pr_gate_create).
//   lmn    [edge_capacity][36]  L_a = Z_a^-1 P_ia, M_a = (P_ia^-1 Z_a) P_ja, N_a = P_ja^-1 of every valid edge
//   eij    [edge_capacity][2]   the edge's rows (0, 0 where the edge is not valid)
//   valid  [edge_capacity] i32  1: the edge is valid in this run
//   keep   2 x [edge_capacity] i32   keep_r in keep[r & 1]
//   sup    [edge_capacity] i32  s_r of the round in flight (integer adds of the b ranges), zero between rounds
//   map    [edge_capacity] i32  the rank of a kept edge among the kept, or -1
//   rot_tab, trans2_tab [max_gap + 1]  the two tables, uploaded by create
//   ctl    [4] i32              n, E, the source log's overflow bit, 0
struct GateView {
  const int* s_ij; const double* s_Z; const double* s_w; const int* s_state;
  int* d_ij; double* d_Z; double* d_w; int* d_state;
  int node_capacity, edge_capacity, max_gap, min_support, rounds;
  double* lmn; int* eij; int* valid; int* keep[2]; int* sup; int* map;
  const double* rot_tab; const double* trans2_tab; int* ctl;
};

// workgroups over the b range of a round: a function of edge_capacity only
inline int gate_split(int edge_capacity) {
  const int gx = (edge_capacity + 255) / 256, tiles = (edge_capacity + GATE_TILE - 1) / GATE_TILE, want = 1024 / gx > 1 ? 1024 / gx : 1;
  return tiles < want ? tiles : want;
}

void launch_gate(hipStream_t st, const GateView& v, const double* poses, const int* n, unsigned char* keep, int* support, int* map, int* info);

}  // namespace pr
