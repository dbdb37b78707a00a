// seqmatch.hpp — what seqmatch.hip (the kernels), seqmatch.cpp (the C ABI) and pr_api.cpp (the host-buffer form) of the sequence
// matcher share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int SEQ_R = 8;              // query rows of a workgroup's tile (pr_seq_tile's rows)
constexpr int SEQ_W = 256;            // columns of a slab (pr_seq_tile's cols)
constexpr int SEQ_REACH = 64;         // largest |steps[v][l]|: the halo on either side of a slab
constexpr int SEQ_MAX_L = 32, SEQ_MAX_V = 16, SEQ_MAX_K = 32;
constexpr int SEQ_MAX_P = 64;         // most column parts of a row tile
constexpr size_t SEQ_LIST_ENTRIES = (size_t)1024 * SEQ_R * SEQ_MAX_K;   // capacity of the parts' lists: P m k entries

// 0 when the HOST table [V][L] is one a call accepts, else the number (1-based) of the first rule it breaks:
// 1: sizes, 2: steps[v][0] != 0, 3: |steps[v][l]| > 64
inline int seq_steps_bad(const int32_t* steps, int V, int L) {
  if (V < 1 || V > SEQ_MAX_V || L < 1 || L > SEQ_MAX_L) return 1;
  for (int v = 0; v < V; v++) {
    if (steps[(size_t)v * L] != 0) return 2;
    for (int l = 0; l < L; l++)
      if (steps[(size_t)v * L + l] > SEQ_REACH || steps[(size_t)v * L + l] < -SEQ_REACH) return 3;
  }
  return 0;
}

// column parts per row tile: a function of (m, n) only.  Row tiles alone fill the chip from 1024 of them on; below that every tile's
// slabs are cut into P consecutive runs, one workgroup each, and seq_merge_kernel reduces the P lists of a row by (S, j).
inline int seq_parts(int m, int n) {
  const long long tiles = ((long long)m + SEQ_R - 1) / SEQ_R, slabs = ((long long)n + SEQ_W - 1) / SEQ_W;
  if (tiles <= 0) return 1;
  long long P = 1024 / tiles;
  if (P > SEQ_MAX_P) P = SEQ_MAX_P;
  if (P > slabs) P = slabs;
  return P < 1 ? 1 : (int)P;
}

// scores f64 | indices i32 | velocities i32 of SEQ_LIST_ENTRIES list entries
inline size_t seq_scratch_bytes() { return SEQ_LIST_ENTRIES * 16; }

// ---- the online form (pr_seqmatch): everything SeqView names lies in the ONE allocation of pr_seqmatch_create
constexpr int SEQ_ONLINE_MAX_K = 128;
constexpr int SEQ_PUSH_COLS = 256;     // columns of a workgroup of the push's score kernel: its sorted list has min(k, 256) entries
//   ring   [L][capacity] f64  the fused rows of the last L pushes (slot = push number mod L; columns >= the row's n keep older bytes)
//   ids    [L] i32            the row id n of every slot
//   count  [1] i32            pushes so far
//   stats  [4][2] f64         (mean, sd) per channel of the push in flight
//   ctl    [4] i32            on, n, pushes before - written by the statistics kernel for the two kernels behind it
//   lists  [blocks][max_k]    the workgroups' best cells: score f64 | j i32 | v i32
struct SeqView {
  int capacity, channels, V, L, max_k, blocks;
  double* ring; int* ids; int* count; double* stats; int* ctl; const int* steps;
  double* lscore; int* lj; int* lv;
};
struct SeqWeights { double w[4]; };
void launch_seq_push(hipStream_t st, const SeqView& v, const double* rows, const int* count, const int* emitted, const SeqWeights& w,
                     int normalize, int mask_width, int k, int32_t* idx, double* score, int32_t* vel, int32_t* info);

void launch_seq_select(hipStream_t st, const float* d_p, const float* d_i, int m, int n, const double* mom, const int* d_steps, int V, int L,
                       int q_row0, int db_row0, int mask_width, double p_weight, int k, int32_t* idx, double* score, int32_t* vel, double* d_S,
                       void* scratch);

}  // namespace pr
