// online.hpp — what online.hip (the kernels) and online.cpp (the C ABI) of the online signature database share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int ONLINE_OVERFLOW = 1;           // = PR_ONLINE_OVERFLOW
constexpr int ONLINE_NB = 512;               // most workgroups of the rows kernel: NB = min(capacity, ONLINE_NB)
constexpr int ONLINE_MAX_K = 128;

// The caller's two buffers, the create sizes and the scratch of a pr_online (all allocated by pr_online_create):
//   rows    [2][capacity]  the distances of the last match (structure | intensity; count | intensity for M2DP)
//   partial [NB][2][2]     per workgroup and channel: (entries that are not NaN, sum of d - 0.5) - every slot written by every match
//   stats   [2][2]         per channel: mean, sd (N - 1)
struct OnlineView {
  double* sig; int* state;
  int type, capacity, max_k, NB;
  int sig_doubles;                           // of one entry: 2400 (SC: 1 x 2400) or 1536 (M2DP: 4 x 384)
  double* rows; double* partial; double* stats;
};

inline int online_blocks(int capacity) { return capacity < ONLINE_NB ? capacity : ONLINE_NB; }

// rows: where the distances go and are read from - the view's scratch, or the caller's [2][capacity]
void launch_online_match(hipStream_t st, const OnlineView& v, const double* sig, const int* emitted, int mask_width, double p_weight, int k,
                         int* idx, double* score, double* rows);
void launch_online_append(hipStream_t st, const OnlineView& v, const double* sig, const int* emitted, int* info);

}  // namespace pr
