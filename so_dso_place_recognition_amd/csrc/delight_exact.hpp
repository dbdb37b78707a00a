// delight_exact.hpp - the exact DELIGHT pair distance in fp64, 16 pairs at a time (processDELIGHT.m:7-37 in the reference's summation
// order), shared by delight_match.hip (rerank and exact rows) and online.hip (the rows of an online DELIGHT set): one text, so a
// duplicated row gives both the same bits.  256 threads compute the terms of 4 columns x 16 rows x 4 permutations of every pair in
// parallel, then 64 threads - one per (pair, permutation) - add them in the normative order.
#pragma once
#include <hip/hip_runtime.h>

namespace pr {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int XB = 16;            // pairs per batch
struct XShared {
  double term[64][65];            // [4 columns x 16 rows in the normative order][pair * 4 + permutation], padded
  double fin[XB][4];
};

// d[p] = the normative distance of (A[p], B[p]) for p < np (1 <= np <= 16); all 256 threads call it.  A skipped term is stored as -1:
// a term that is added is >= +0, +Inf or NaN, never negative.
__device__ __forceinline__ void exact_batch(XShared& sh, int tid, int np, const double* const* A, const double* const* B, double* d) {
#pragma clang fp contract(off)      // the generators' rounding (-ffp-contract=off) whatever the flags of the file that includes this
  const int p = tid >> 4, r = tid & 15, pl = p < np ? p : 0;
  const double* pa = A[pl] + r * 256;
  const double* pb = B[pl] + r * 256;
  double ts = 0.0;
  int tc = 0;
  for (int c0 = 0; c0 < 256; c0 += 4) {
    const f64x2 a0 = *reinterpret_cast<const f64x2*>(pa + c0), a1 = *reinterpret_cast<const f64x2*>(pa + c0 + 2);
    const f64x2 b0 = *reinterpret_cast<const f64x2*>(pb + c0), b1 = *reinterpret_cast<const f64x2*>(pb + c0 + 2);
    const double av[4] = {a0[0], a0[1], a1[0], a1[1]}, bv[4] = {b0[0], b0[1], b1[0], b1[1]};
#pragma unroll
    for (int cc = 0; cc < 4; cc++) {
      const double a = av[cc];
      const double b[4] = {bv[cc], __shfl_xor(bv[cc], 5), __shfl_xor(bv[cc], 6), __shfl_xor(bv[cc], 3)};   // row r ^ X of the same pair
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const double sum = a + b[k], df = a - b[k];
        const double t = ((2.0 * df) * df) / sum;
        sh.term[cc * 16 + r][p * 4 + k] = sum > 0.0 ? t : -1.0;
      }
    }
    __syncthreads();
    if (tid < 64) {
      for (int e = 0; e < 64; e++) {
        const double t = sh.term[e][tid];
        if (t != -1.0) { ts += t; tc++; }
      }
    }
    __syncthreads();
  }
  if (tid < 64) sh.fin[tid >> 2][tid & 3] = ts / (double)tc;
  __syncthreads();
  if (tid < np) {
    double best = __builtin_inf();
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (best > sh.fin[tid][k]) best = sh.fin[tid][k];
    d[tid] = best;
  }
  __syncthreads();
}

}  // namespace
}  // namespace pr
