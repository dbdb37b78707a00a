// trajeval.hpp — what trajeval.hip (the kernels) and trajeval.cpp (the C ABI) of the trajectory evaluation share.
// The rigid products are gate.hip's, copied here in the same operation order (gate.hip keeps its own text); the one-sided Jacobi follows
// icp.hip's kabsch with a FIXED sweep count, so that tests/trajeval_np.py can restate it rotation by rotation.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int TRAJ_ALIGN_NONE = 0, TRAJ_ALIGN_FIRST = 1, TRAJ_ALIGN_SE3 = 2, TRAJ_ALIGN_SIM3 = 3;      // = PR_TRAJ_ALIGN_*
constexpr int TRAJ_GT_W2C = 0, TRAJ_GT_C2W = 1, TRAJ_GT_POSITIONS = 2;                                 // = PR_TRAJ_GT_*
constexpr int TRAJ_FEW = 1, TRAJ_DEGENERATE = 2, TRAJ_NO_SCALE = 4;                                    // = PR_TRAJ_* flags
constexpr int TRAJ_T = 256;                  // threads of every workgroup = lanes of the fixed tree = blocks of the prefix
constexpr int TRAJ_SWEEPS = 10;              // Jacobi sweeps, always all of them
constexpr int TRAJ_MAX_B = 64, TRAJ_MAX_K = 8, TRAJ_MAX_L = 8;
constexpr int TRAJ_ATE = 24, TRAJ_RPE = 8, TRAJ_SEG = 4, TRAJ_CLO = 8;       // doubles of one statistics row (= PR_TRAJ_*_STATS)

// The create sizes, the tables and the scratch of a pr_trajeval (all allocated by pr_trajeval_create).
//   used    [B][cap] i32     1: row i of candidate b is used in this run
//   gtok    [cap] i32        1: i < n, valid[i] != 0 and the gt row is finite
//   cen     [B + 1][cap][3]  the camera centres of the est rows of every b, then of the gt rows; zeros for a row that is not used
//   prefix  [B][2][cap]      path length over the gt centres, then over the est centres, of the used rows of b
//   S       [B][16]          s, R (9, row-major), t (3), 3 unused
//   segsum  [B][L][4]        segments and the three tree sums of every length (what the row over all lengths is added from)
//   deltas  [8] i32, lengths [8] f64   the two tables, uploaded by create
struct TrajView {
  int cap, B, align, gt_kind, K, L, step, slots, edge_capacity;
  double rot_thr, trans_thr;
  int* used; int* gtok; double* cen; double* prefix; double* S; double* segsum;
  const int* deltas; const double* lengths;
};

struct TrajIn {
  const double* est; const int* n; const double* gt; const unsigned char* valid;
  const int* e_ij; const double* e_Z; const int* e_state;       // the closure log, or three NULLs
};

struct TrajOut {
  double* ate; double* rpe; double* seg; double* clo; double* err; int* seg_end; double* edge_err; double* centres; double* prefix;
};

inline int traj_slots(int cap, int step) { return (int)(((long long)cap + step - 1) / step); }

void launch_trajeval(hipStream_t st, const TrajView& v, const TrajIn& in, const TrajOut& out);

#if defined(__HIPCC__)
namespace traj {

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ bool fin(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }       // false for NaN and Inf

__device__ __forceinline__ void mul33(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void mv3(const double* A, const double* x, double* y) {            // A x
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
__device__ __forceinline__ void mtv3(const double* A, const double* x, double* y) {           // A^T x
#pragma unroll
  for (int r = 0; r < 3; r++) y[r] = A[r] * x[0] + A[3 + r] * x[1] + A[6 + r] * x[2];
}
// pose row p [12] = [R | t] row-major 3 x 4
__device__ __forceinline__ void load_pose(const double* p, double* R, double* t) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    R[3 * r] = p[4 * r]; R[3 * r + 1] = p[4 * r + 1]; R[3 * r + 2] = p[4 * r + 2]; t[r] = p[4 * r + 3];
  }
}
// C = A B = [R_A R_B | R_A t_B + t_A]
__device__ __forceinline__ void rigid_mul(const double* RA, const double* tA, const double* RB, const double* tB, double* RC, double* tC) {
  double y[3];
  mul33(RA, RB, RC);
  mv3(RA, tB, y);
  tC[0] = y[0] + tA[0]; tC[1] = y[1] + tA[1]; tC[2] = y[2] + tA[2];
}
// A^-1 = [R^T | -(R^T t)]
__device__ __forceinline__ void rigid_inv(const double* R, const double* t, double* Ri, double* ti) {
  double y[3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Ri[3 * r + c] = R[3 * c + r];
  mtv3(R, t, y);
  ti[0] = -y[0]; ti[1] = -y[1]; ti[2] = -y[2];
}
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace traj
#endif

}  // namespace pr
