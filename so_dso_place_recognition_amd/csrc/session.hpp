// session.hpp — what session.hip (the kernels) and session.cpp (the C ABI) of the drive sessions share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr int SESSION_OVERFLOW = 1;          // = PR_SESSION_OVERFLOW
constexpr int SESSION_REUSED = 2;            // = PR_SESSION_REUSED
constexpr int SESSION_LOG_OVERFLOW = 4;      // = PR_SESSION_LOG_OVERFLOW
constexpr int SESSION_POSEGRAPH_OVERFLOW = 1;  // = PR_POSEGRAPH_OVERFLOW, the bit of the log's state[1]
constexpr int SESSION_ALIGNED = 0, SESSION_NO_TARGET = 1, SESSION_NO_CANDIDATE = 2, SESSION_WEAK = 3, SESSION_NONFINITE = 4;
constexpr int SESSION_TILE = 64;             // candidates b of one LDS tile of the pairs kernel
constexpr int SESSION_MAX = 1024;            // most sessions of a table: the starts of one table fit one LDS array

// The caller's two buffers, the create sizes and the scratch of a pr_session (one allocation made by pr_session_create).
//   sid    [node_capacity] i32   the session of every row
//   brk    [node_capacity] i32   1: the row is a break (what the relaxation's prepare step reads)
//   cand   [edge_capacity] i32   1: the edge slot is a candidate of this call
//   q      [edge_capacity] i32   the candidate's row in the target session
//   hyp    [edge_capacity][12]   G_a; c, p [edge_capacity][3]: c_a and G_a c_a
//   sup, inl [edge_capacity] i32 the support counts (integer adds of the b ranges) and the membership of I
//   gd     [24] f64              G and G^-1 of this call;  ctl [12] i32: n, E, S, t, status, a*, its support, candidates, |I|, flags, 0, 0
struct SessionView {
  int* start; int* state;
  int node_capacity, edge_capacity, session_capacity;
  int* sid; int* brk; int* cand; int* q; double* hyp; double* c; double* p; int* sup; int* inl; double* gd; int* ctl;
};

// the log of one align call (only read) and the call's numbers
struct SessionAlign {
  const int* e_ij; const double* e_Z; const double* e_w; const int* e_state;
  int log_edge_capacity, session, min_inliers;
  double rot_c_max, trans2_max;
};

// workgroups over the b range of the pairs kernel: a function of edge_capacity only
inline int session_split(int edge_capacity) {
  const int gx = (edge_capacity + 255) / 256, tiles = (edge_capacity + SESSION_TILE - 1) / SESSION_TILE, want = 1024 / gx > 1 ? 1024 / gx : 1;
  return tiles < want ? tiles : want;
}

void launch_session_reset(hipStream_t st, const SessionView& v);
void launch_session_begin(hipStream_t st, const SessionView& v, const int* n, int* info);
// sid and brk of every row from the table as it stands: the launch in front of a relaxation across breaks
void launch_session_rows(hipStream_t st, const SessionView& v);
void launch_session_align(hipStream_t st, const SessionView& v, const SessionAlign& a, const double* poses_in, const int* n, double* poses_out,
                          double* G, double* hyp, int* support, unsigned char* inlier, int* info);

}  // namespace pr
