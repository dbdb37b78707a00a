// onlineset.hpp — what onlineset.hip (the kernels) and onlineset.cpp (the C ABI) of the online signature SETS share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int ONLINESET_FUSED = 0, ONLINESET_DELIGHT = 1;      // = PR_ONLINESET_FUSED / PR_ONLINESET_DELIGHT
constexpr int ONLINESET_OVERFLOW = 1;                           // = PR_ONLINE_OVERFLOW
constexpr int ONLINESET_NB_FUSED = 512;      // most workgroups of the fused rows kernel: NB = min(capacity, ONLINESET_NB_FUSED), one entry per stride
constexpr int ONLINESET_NB_DELIGHT = 64;     // most workgroups of the DELIGHT rows kernel: NB = min(ceil(capacity / 16), ONLINESET_NB_DELIGHT), 16 entries per stride
constexpr int ONLINESET_MAX_K = 128;
constexpr int ONLINESET_SC = 2400, ONLINESET_M2DP = 4 * 384, ONLINESET_DELIGHT_LEN = 16 * 256;      // doubles of one entry's part

// The caller's buffers, the create sizes and the scratch of a pr_onlineset (all allocated by pr_onlineset_create):
//   rows    [C][capacity]  the distances of the last match; C = 4 (FUSED: SC structure, SC intensity, M2DP count, M2DP intensity) or 1
//   partial [NB][4][2]     FUSED only - per workgroup and channel: (entries that are not NaN, sum of d - 0.5), every slot written by every match
//   stats   [4][2]         FUSED only - per channel: mean, sd (N - 1)
struct OnlineSetView {
  double* sc; double* m2dp; double* delight; int* state;
  int kind, capacity, max_k, NB;
  double* rows; double* partial; double* stats;
};

inline int onlineset_channels(int kind) { return kind == ONLINESET_FUSED ? 4 : 1; }
inline int onlineset_blocks(int kind, int capacity) {
  if (kind == ONLINESET_FUSED) return capacity < ONLINESET_NB_FUSED ? capacity : ONLINESET_NB_FUSED;
  const int batches = (capacity + 15) / 16;
  return batches < ONLINESET_NB_DELIGHT ? batches : ONLINESET_NB_DELIGHT;
}

// sc / m2dp / delight: the query's (or the new keyframe's) parts - the two of a FUSED set or the one of a DELIGHT set.
// rows: where the distances go and are read from - the view's scratch, or the caller's [C][capacity]
void launch_onlineset_match(hipStream_t st, const OnlineSetView& v, const double* sc, const double* m2dp, const double* delight,
                            const int* emitted, int mask_width, double p_weight, int k, int* idx, double* score, double* rows);
void launch_onlineset_append(hipStream_t st, const OnlineSetView& v, const double* sc, const double* m2dp, const double* delight,
                             const int* emitted, int* info);

}  // namespace pr
