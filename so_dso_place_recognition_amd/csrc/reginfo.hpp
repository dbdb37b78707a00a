// reginfo.hpp — what reginfo.hip (the kernels) and reginfo.cpp (the C ABI) of the registration information share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int REGINFO_POINT_SUMS = 11;       // n, sum d2, sum u_a (3), sum u_a u_b (6: 00 01 02 11 12 22)
constexpr int REGINFO_PLANE_SUMS = 25;       // n_inl, sum d2, n_pl, sum r^2, sum J J^T (21: upper triangle, row-major)
constexpr int REGINFO_NS = 25;               // doubles of one chunk's record in the handle's partials (the point metric uses the first 11)

// the flag bits of stat[3] (= PR_REGINFO_*)
constexpr int REGINFO_OFF = 1, REGINFO_NONFINITE = 2, REGINFO_TOO_FEW = 4, REGINFO_SINGULAR = 8, REGINFO_WEAK_ROT = 16, REGINFO_WEAK_TRANS = 32;

// one call's inputs: the source clouds, the slots, the poses and the correspondences of the pass the caller ran at those poses; for the
// plane metric the world rows and their normals
struct RegInfoIn {
  const double* xyz_q; const int64_t* offs_q; int Nq;
  const int32_t* pair_src; int c;
  const double* T; const unsigned char* accepted;               // accepted may be NULL
  const int64_t* out_offs; const int32_t* nn_idx; const double* nn_d2;
  int max_src, nchunks;
  double mc2;                                                    // fl(max_corr^2)
  const double* world_xyz; int64_t ocap; const double* normals; const int* ninfo;        // plane metric only
};

struct RegInfoParams { int min_inliers; double min_ratio, sigma_min, w_max; };

struct RegInfoOut { double* H; double* cov; double* spec; double* w; int32_t* stat; unsigned char* ok; };

// grid (nchunks, c): part [c][nchunks][REGINFO_NS]
void launch_reginfo_sums(hipStream_t st, const RegInfoIn& in, int plane, double* part);
// grid (c): one wave per slot
void launch_reginfo_finish(hipStream_t st, const RegInfoIn& in, int plane, const double* part, const RegInfoParams& prm, const RegInfoOut& out);

}  // namespace pr
