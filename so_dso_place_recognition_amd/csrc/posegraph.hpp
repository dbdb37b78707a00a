// posegraph.hpp — what posegraph.hip (the kernels) and posegraph.cpp (the C ABI) of the loop-closure log and the pose-graph relaxation
// share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int POSEGRAPH_OVERFLOW = 1;        // = PR_POSEGRAPH_OVERFLOW
constexpr int POSEGRAPH_MAX_K = 128;         // most slots of one add
constexpr int PG_BLOCKS = 45;                // doubles of one edge's Jacobian blocks: Arw, Atw, Atv, Brw, Btv (3 x 3 each, row-major)

// The caller's four buffers, the create sizes and the scratch of a pr_posegraph (all allocated by pr_posegraph_create).  An edge SLOT s
// is an odometry edge (s, s + 1) for s < node_capacity - 1 and the logged edge s - (node_capacity - 1) behind them: S slots in all.
//   X      [node_capacity][12]  the poses the relaxation works on (a copy of the input, so the output may be the input)
//   zodo   [node_capacity][12]  the odometry measurements Z = P_s (P_s+1)^-1 of the input poses
//   valid  [S] i32              1: the slot is an edge of this call
//   jac    [S][45], res [S][6], wgt [S][2], cost [S]   the linearisation of every valid slot at X
//   g, x, r, z, p, q [node_capacity][6]  the gradient and the vectors of the inner solve;  dinv [node_capacity][36]
//   u      [S][6]               W (A x_i + B x_j) of the matrix-vector product
//   finite [node_capacity] i32, deg / cursor [node_capacity] i32, inc_off [node_capacity + 1] i32, inc_raw / inc [2 edge_capacity] i32
//          the incidence list: node a's logged edges, 2 l + side (0: a is the edge's i, 1: its j), ascending = log order (inc_raw: as filled, before the ranking)
//   ctl    [4] i32              n, logged edges, edges used, logged edges used
struct PoseGraphView {
  int* edge_ij; double* edge_Z; double* edge_w; int* state;
  int node_capacity, edge_capacity, max_outer, max_inner, S;
  double* X; double* zodo; double* jac; double* res; double* wgt; double* cost; double* u;
  double* g; double* x; double* r; double* z; double* p; double* q; double* dinv;
  int* valid; int* finite; int* deg; int* cursor; int* inc_off; int* inc_raw; int* inc; int* ctl;
};

struct PoseGraphParams { int outer, inner; double lambda, w_odo_rot, w_odo_trans; };

void launch_posegraph_add(hipStream_t st, const PoseGraphView& v, const int* idx, const double* T, const unsigned char* accepted,
                          const int* query_row, int k, double w_rot, double w_trans, int* info);
// the add with per-slot weights w [k][2] in device memory
void launch_posegraph_add_weighted(hipStream_t st, const PoseGraphView& v, const int* idx, const double* T, const unsigned char* accepted,
                                   const int* query_row, int k, const double* w, int* info);
// the batch add: rows (i[p], j[p]) per slot, weights w [c][2] in device memory or, with w == NULL, the pair (w_rot, w_trans); c <= 65535
void launch_posegraph_add_batch(hipStream_t st, const PoseGraphView& v, const int* i, const int* j, const double* T, const unsigned char* accepted,
                                const double* w, double w_rot, double w_trans, int c, int* info);
// brk: NULL (every odometry slot of finite rows is an edge), or a per-row break array [node_capacity] i32 (session.hpp)
void launch_posegraph_relax(hipStream_t st, const PoseGraphView& v, const double* poses_in, const int* n, const PoseGraphParams& prm,
                            double* poses_out, double* report, const int* brk = nullptr);

}  // namespace pr

// what session.cpp needs of a pr_posegraph (defined in posegraph.cpp): the argument checks of a relax under the caller's name, which touch
// no device, and the launch with a break array
struct pr_ctx;
struct pr_posegraph;
struct pr_posegraph_params;
namespace pr {
int posegraph_relax_check(const char* who, pr_posegraph* g, const double* d_poses_in, const int32_t* d_n, const pr_posegraph_params* params,
                          double* d_poses_out, double* d_report);
int posegraph_relax_launch(pr_posegraph* g, const double* d_poses_in, const int32_t* d_n, const pr_posegraph_params* params,
                           double* d_poses_out, double* d_report, const int* d_brk);
pr_ctx* posegraph_ctx(pr_posegraph* g);
int posegraph_node_capacity(pr_posegraph* g);
}  // namespace pr
