// resident_common.hpp - device helper shared by the rerank kernels of gist_match.hip and delight_match.hip.
#pragma once

namespace pr {
namespace {

// ascending bitonic sort of (sk, si)[0, N) by (score, index); N a power of two, 256 threads
__device__ __forceinline__ void sort_pairs(double* sk, int* si, int N, int tid) {
  for (int k2 = 2; k2 <= N; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < N; i += 256) {
        const int x = i ^ j;
        if (x > i) {
          const double a = sk[i], b = sk[x];
          const int ia = si[i], ib = si[x];
          const bool gt = a > b || (a == b && ia > ib);
          if (gt == ((i & k2) == 0)) { sk[i] = b; sk[x] = a; si[i] = ib; si[x] = ia; }
        }
      }
    }
  __syncthreads();
}

}  // namespace
}  // namespace pr
