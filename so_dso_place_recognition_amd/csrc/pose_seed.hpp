// pose_seed.hpp — the relative-pose seed of a matched pair from the two clouds' PCA frames and the pair's best-aligning variant
// (tests/pose_np.py is the normative restatement).  One function for the host form (pose.cpp) and the device kernel
// (pose.hip), both compiled with -ffp-contract=off: every product and every sum is rounded on its own, in the order written here, which
// for SC is the order of pr_sc_relative_pose (pr_api.cpp).
//   R = E_db S E_q^T, t = mu_db - R mu_q: [R | t] maps points of the query's camera frame into the DB entry's.
//   SC       v = 2 s + r   S = diag(sigma, B): r = 0 turns the y'z' plane by -s D, r = 1 reflects it by f = (s + 1) D, D = 2 pi / 60
//   M2DP     v = 4 a + b   S0 = D_b D_a, D_u = diag(dx, dy, dx dy), (dx, dy) = (-1,-1), (-1,+1), (+1,-1), (+1,+1) (test_m2dp.cpp:46-57)
//   DELIGHT  v = k         S0 = the sign flips of the octant XOR 0, 5, 6, 3 of Mut's row k (processDELIGHT.m:2-5, DELIGHT.cpp:21)
//   M2DP / DELIGHT: S = diag(sigma, 1, 1) S0, sigma = sign(det E_db) sign(det E_q): R is proper whatever the eigen-solver's handedness.
#pragma once

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace pr {

constexpr int POSE_SC = 0, POSE_M2DP = 1, POSE_DELIGHT = 2;   // PR_POSE_* of the header
constexpr int POSE_SC_ANGLES = 61;                            // cos / sin of k D, k = 0 .. 60 (f = (s + 1) D reaches 60 D)

__host__ __device__ inline int pose_variants(int type) { return type == POSE_SC ? 120 : type == POSE_M2DP ? 16 : type == POSE_DELIGHT ? 4 : 0; }

__host__ __device__ inline double pose_det3(const double (&M)[3][3]) {
  return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
         M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// fq / fd: the two [16]-double frames; 0 <= v < pose_variants(type); cs / sn: the SC angle tables (unused for the other types); T [3][4]
__host__ __device__ inline void pose_seed(int type, const double* fq, const double* fd, int v, const double* cs, const double* sn, double* T) {
  double Eq[3][3], Ed[3][3];                                   // [component][eigenvector]
  for (int j = 0; j < 3; j++)
    for (int e = 0; e < 3; e++) { Eq[j][e] = fq[3 + 3 * e + j]; Ed[j][e] = fd[3 + 3 * e + j]; }
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  if (type == POSE_SC) {
    const int s = v >> 1, r = v & 1;
    const double ca = cs[r ? s + 1 : s], sa = sn[r ? s + 1 : s];
    const double sigma = pose_det3(Ed) * pose_det3(Eq) * (r ? -1.0 : 1.0) < 0 ? -1.0 : 1.0;
    S[0][0] = sigma;
    S[1][1] = ca; S[1][2] = sa;
    S[2][1] = r ? sa : -sa; S[2][2] = r ? -ca : ca;
  } else {
    double sx, sy, sz;
    if (type == POSE_M2DP) {
      const int a = v >> 2, b = v & 3;
      const double ax = (a & 2) ? 1.0 : -1.0, ay = (a & 1) ? 1.0 : -1.0, bx = (b & 2) ? 1.0 : -1.0, by = (b & 1) ? 1.0 : -1.0;
      sx = bx * ax; sy = by * ay; sz = (bx * by) * (ax * ay);
    } else {
      const int x = v == 0 ? 0 : v == 1 ? 5 : v == 2 ? 6 : 3;   // octant = 4 (z > 0) + 2 (y > 0) + (x > 0)
      sx = (x & 1) ? -1.0 : 1.0; sy = (x & 2) ? -1.0 : 1.0; sz = (x & 4) ? -1.0 : 1.0;
    }
    const double sigma = (pose_det3(Ed) < 0 ? -1.0 : 1.0) * (pose_det3(Eq) < 0 ? -1.0 : 1.0);
    S[0][0] = sigma * sx; S[1][1] = sy; S[2][2] = sz;
  }
  double ES[3][3], R[3][3];
  for (int j = 0; j < 3; j++)
    for (int e = 0; e < 3; e++) ES[j][e] = Ed[j][0] * S[0][e] + Ed[j][1] * S[1][e] + Ed[j][2] * S[2][e];
  for (int j = 0; j < 3; j++)
    for (int e = 0; e < 3; e++) R[j][e] = ES[j][0] * Eq[e][0] + ES[j][1] * Eq[e][1] + ES[j][2] * Eq[e][2];   // E_db S E_q^T
  for (int j = 0; j < 3; j++) {
    for (int e = 0; e < 3; e++) T[4 * j + e] = R[j][e];
    T[4 * j + 3] = fd[j] - (R[j][0] * fq[0] + R[j][1] * fq[1] + R[j][2] * fq[2]);
  }
}

// The choice among a pair's H refined hypotheses (S: a statistics record with fitness, rmse, status; ok0 / ok1: the two qualifying status
// codes, converged and max_iter): the qualified one with the larger fitness, then the smaller rmse, then the smaller h.  IEEE comparisons:
// a NaN never replaces anything and a kept NaN loses to a number.  Returns the kept h, or -1 when none qualifies.
template <class S>
__host__ __device__ inline bool pose_better(const S& a, const S& b) {
  if (a.fitness > b.fitness) return true;
  if (b.fitness != b.fitness && a.fitness == a.fitness) return true;
  if (a.fitness == b.fitness) return a.rmse < b.rmse || (b.rmse != b.rmse && a.rmse == a.rmse);
  return false;
}
template <class S>
__host__ __device__ inline int pose_select(const S* s, int H, int ok0, int ok1) {
  int best = -1;
  for (int h = 0; h < H; h++) {
    if (s[h].status != ok0 && s[h].status != ok1) continue;
    if (best < 0 || pose_better(s[h], s[best])) best = h;
  }
  return best;
}

}  // namespace pr
