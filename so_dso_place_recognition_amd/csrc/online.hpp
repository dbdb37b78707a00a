// online.hpp — what online.hip (the kernels) and online.cpp (the C ABI) of the online engine share: ONE engine of four kinds behind
// pr_online (SC, M2DP) and pr_onlineset (FUSED, DELIGHT).
#pragma once
#include <hip/hip_runtime.h>
#include "onlineset.hpp"

namespace pr {
constexpr int ONLINE_SC = 0, ONLINE_M2DP = 1, ONLINE_FUSED = 2, ONLINE_DELIGHT = 3;      // the engine's kinds (not an ABI value)
constexpr int ONLINE_OVERFLOW = 1;           // = PR_ONLINE_OVERFLOW
constexpr int ONLINE_NB = 512;               // most workgroups of the SC / M2DP rows kernel: NB = min(capacity, ONLINE_NB)
constexpr int ONLINE_MAX_K = 128, ONLINE_SC_LEN = 2400, ONLINE_M2DP_LEN = 4 * 384, ONLINE_DELIGHT_LEN = 16 * 256;      // ..._LEN: doubles of one entry's part

// The caller's buffers, the create sizes and the scratch (all allocated by the create call).  With C = online_channels(kind):
//   part, len  the one or two row buffers and their doubles per entry: SC {2400}, M2DP {1536}, FUSED {2400, 1536}, DELIGHT {4096}; len[1] = 0: one part
//   rows    [C][capacity]  the distances of the last match, channels in the order SC structure, SC intensity, M2DP count, M2DP intensity
//   partial [NB][C][2]     C > 1 - per workgroup and channel: (entries that are not NaN, sum of d - 0.5), every slot written by every match
//   stats   [C][2]         C > 1 - per channel: mean, sd (N - 1)
struct OnlineView {
  double* part[2]; int len[2];
  int* state;
  int kind, capacity, max_k, NB;
  double* rows; double* partial; double* stats;
};
struct OnlineParts { const double* p[2]; };  // the query's (or the new keyframe's) parts, in the view's order

inline int online_channels(int kind) { return kind == ONLINE_FUSED ? 4 : (kind == ONLINE_DELIGHT ? 1 : 2); }
inline int online_blocks(int kind, int capacity) {
  if (kind != ONLINE_DELIGHT) return capacity < ONLINE_NB ? capacity : ONLINE_NB;      // (ONLINESET_NB_FUSED is the same number: static_assert in online.hip)
  const int batches = (capacity + 15) / 16;
  return batches < ONLINESET_NB_DELIGHT ? batches : ONLINESET_NB_DELIGHT;
}

// rows: where the distances go and are read from - the view's scratch, or the caller's [C][capacity]
void launch_online_match(hipStream_t st, const OnlineView& v, const OnlineParts& q, const int* emitted, int mask_width, double p_weight, int k,
                         int* idx, double* score, double* rows);
void launch_online_append(hipStream_t st, const OnlineView& v, const OnlineParts& src, const int* emitted, int* info);

}  // namespace pr
