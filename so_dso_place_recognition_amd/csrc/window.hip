// window.hip — the pre-stage one keyframe at a time (utils/pts_preprocess.h:135-216): the reference's "nearby" point set
// lives in HBM, one push appends a keyframe's new world points, prunes the set against that keyframe's pose and emits its down-sampled
// cloud with the PCA frame.  prestage.hip answers the same question point-major for a finished drive (a point's death is found by walking
// the later poses); here the set is carried from push to push instead, in the reference's own order: append-only, pruning keeps the
// relative order - so "member index" below is simply the position in the set.
//
// A push is a fixed chain of launches whose grids depend on the capacities given at create only; everything that varies (the pose, the
// count of new points, the reset test, the 30 warm-up frames, the alive count, which buffer of the ping-pong pair is current) is read from
// device memory, so one captured push serves every keyframe:
//   state     one lane: reset test, warm-up counter, emit decision, n_new clamped to max_new and to the free capacity
//   append    the new points go behind the alive set
//   count     (emitting push) range test per member, per-workgroup survivor counts
//   scan      exclusive scan of the workgroup totals -> alive count
//   scatter   survivors to the other buffer in order (stable compaction); cell id + ordering value per survivor, per-cell atomicMin of the
//             value and of the first member index
//   winners   earliest member among those that hold their cell's minimum; per-workgroup counts of the members that are first of their cell
//   scan      -> K, n_out
//   keys      ordered compaction of the first-of-cell members: the key insertion sequence, and each key's winner
//   order     ONE lane: libstdc++ node-list order of that sequence (hash_order.hpp), scratch in LDS when it fits; writes out_offs and info
//   gather    one workgroup: the emitted cloud, its frame and float intensity average (gather_frames_cloud, shared with prestage.hip)
//   clear     the touched cells of the dense table back to "empty" (a table of 450 241 voxel cells costs 7.2 MB to memset per push; the
//             members that touched it are at hand)
// No floating-point atomics, no matrix cores; all deciding arithmetic is prestage_common.hpp's, compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hash_order.hpp"
#include "kernels.hpp"
#include "prestage_common.hpp"

namespace pr {
namespace {

// device state words of a window (WinView::st)
enum { WS_ALIVE = 0, WS_SINCE, WS_FLAGS, WS_EMIT, WS_NNEW, WS_BASE, WS_NTOT, WS_CUR, WS_SRC, WS_DST, WS_K, WS_NOUT, WS_WORDS };
static_assert(WS_WORDS <= WIN_STATE_WORDS, "state words");

__global__ __launch_bounds__(64) void win_state_kernel(WinView v, const double* __restrict__ pose, const int* __restrict__ n_new_dev,
                                                       int max_new) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int* st = v.st;
  const double* w = pose;
  if (sqrt(w[3] * w[3] + w[7] * w[7] + w[11] * w[11]) < 1.0) {          // :189-193
    st[WS_ALIVE] = 0; st[WS_SINCE] = 0; st[WS_FLAGS] = 0;
  }
  int n = *n_new_dev, flags = st[WS_FLAGS];
  const int alive = st[WS_ALIVE];
  if (n < 0) n = 0;
  if (n > max_new) { n = max_new; flags |= WIN_OVERFLOW; }
  if (n > v.cap - alive) { n = v.cap - alive; flags |= WIN_OVERFLOW; }
  st[WS_FLAGS] = flags;
  st[WS_NNEW] = n; st[WS_BASE] = alive; st[WS_NTOT] = alive + n;
  st[WS_K] = 0; st[WS_NOUT] = 0;
  const int cur = st[WS_CUR] & 1;
  st[WS_SRC] = cur;
  if (st[WS_SINCE] < 30) {                                                // INIT_FRAME :203-206: the points are appended, nothing else
    st[WS_SINCE] = st[WS_SINCE] + 1;
    st[WS_EMIT] = 0; st[WS_DST] = cur; st[WS_ALIVE] = alive + n;
  } else {
    st[WS_EMIT] = 1; st[WS_DST] = cur ^ 1; st[WS_CUR] = cur ^ 1;          // WS_ALIVE: the scan of the survivor counts
  }
}

__global__ __launch_bounds__(64) void win_reset_kernel(WinView v) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  v.st[WS_ALIVE] = 0; v.st[WS_SINCE] = 0; v.st[WS_FLAGS] = 0;
}

__global__ __launch_bounds__(256) void win_append_kernel(WinView v, const double* __restrict__ xyz_new, const float* __restrict__ inten_new) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= v.st[WS_NNEW]) return;
  const size_t d = (size_t)v.st[WS_BASE] + i;                             // < cap: the state kernel clamped n_new
  double* x = v.xyz[v.st[WS_SRC]];
  x[3 * d] = xyz_new[3 * (size_t)i]; x[3 * d + 1] = xyz_new[3 * (size_t)i + 1]; x[3 * d + 2] = xyz_new[3 * (size_t)i + 2];
  v.inten[v.st[WS_SRC]][d] = inten_new[i];
}

__global__ __launch_bounds__(256) void win_count_kernel(WinView v, const double* __restrict__ pose) {
  const int ntot = v.st[WS_NTOT];
  if (!v.st[WS_EMIT] || (int)blockIdx.x * 256 >= ntot) return;            // uniform per workgroup
  const int s = blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  if (s < ntot) {
    const double* x = v.xyz[v.st[WS_SRC]] + 3 * (size_t)s;
    const double g[3] = {x[0], x[1], x[2]};
    double l[3];
    keep = to_camera(pose, g, v.grid.range, l);
  }
  int tot;
  (void)block_rank(keep, &tot);
  if (threadIdx.x == 0) v.bcnt[blockIdx.x] = tot;
}

// exclusive scan of cnt[0 .. ceil(st[n_word] / 256)) by one workgroup; total -> the alive count (which = 0) or K and n_out (which = 1)
__global__ __launch_bounds__(256) void win_scan_kernel(WinView v, int which) {
  __shared__ int wsum[4];
  __shared__ int carry;
  int* st = v.st;
  if (!st[WS_EMIT]) return;
  const int* cnt = which ? v.kcnt : v.bcnt;
  int* off = which ? v.koff : v.boff;
  const int nb = ((which ? st[WS_ALIVE] : st[WS_NTOT]) + 255) >> 8;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int c = 0; c < nb; c += 256) {
    const int x = (c + tid < nb) ? cnt[c + tid] : 0;
    int inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(inc, d); if (lane >= d) inc += y; }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int base = carry, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { if (i < w) base += wsum[i]; tot += wsum[i]; }
    if (c + tid < nb) off[c + tid] = base + inc - x;
    __syncthreads();
    if (tid == 0) carry += tot;
    __syncthreads();
  }
  if (tid == 0) {
    const int total = carry;
    if (which == 0) st[WS_ALIVE] = total;
    else {
      st[WS_K] = total;
      if (total > v.max_out) { st[WS_NOUT] = v.max_out; st[WS_FLAGS] = st[WS_FLAGS] | WIN_OVERFLOW; } else st[WS_NOUT] = total;
    }
  }
}

__global__ __launch_bounds__(256) void win_scatter_kernel(WinView v, const double* __restrict__ pose) {
  const int ntot = v.st[WS_NTOT];
  if (!v.st[WS_EMIT] || (int)blockIdx.x * 256 >= ntot) return;
  const int s = blockIdx.x * 256 + threadIdx.x;
  const double* sx = v.xyz[v.st[WS_SRC]];
  bool keep = false;
  double g[3] = {0, 0, 0}, l[3] = {0, 0, 0};
  if (s < ntot) {
    g[0] = sx[3 * (size_t)s]; g[1] = sx[3 * (size_t)s + 1]; g[2] = sx[3 * (size_t)s + 2];
    keep = to_camera(pose, g, v.grid.range, l);
  }
  int tot;
  const int r = block_rank(keep, &tot);
  if (!keep) return;
  const size_t d = (size_t)v.boff[blockIdx.x] + r;                        // <= s: the survivors in front of this one
  double* dx = v.xyz[v.st[WS_DST]];
  dx[3 * d] = g[0]; dx[3 * d + 1] = g[1]; dx[3 * d + 2] = g[2];
  v.inten[v.st[WS_DST]][d] = v.inten[v.st[WS_SRC]][s];
  int cell;
  unsigned long long val;
  cell_of(v.grid, l, &cell, &val);
  if (cell < 0 || cell >= v.C) cell = 0;          // cannot happen for |p| < range; keeps a corrupt input from writing out of bounds
  v.cell[d] = cell;
  v.val[d] = val;
  atomicMin(&v.tval[cell], val);
  atomicMin(&v.tfirst[cell], (unsigned)d);
}

__global__ __launch_bounds__(256) void win_winners_kernel(WinView v) {
  const int n = v.st[WS_ALIVE];
  if (!v.st[WS_EMIT] || (int)blockIdx.x * 256 >= n) return;
  const int s = blockIdx.x * 256 + threadIdx.x;
  bool first = false;
  if (s < n) {
    const int c = v.cell[s];
    if (v.val[s] == v.tval[c]) atomicMin(&v.tbest[c], (unsigned)s);       // ties -> the earlier point (:78-80 / :117-119 are strict)
    first = v.tfirst[c] == (unsigned)s;
  }
  int tot;
  (void)block_rank(first, &tot);
  if (threadIdx.x == 0) v.kcnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void win_keys_kernel(WinView v) {
  const int n = v.st[WS_ALIVE];
  if (!v.st[WS_EMIT] || (int)blockIdx.x * 256 >= n) return;
  const int s = blockIdx.x * 256 + threadIdx.x;
  bool first = false;
  int c = 0;
  if (s < n) { c = v.cell[s]; first = v.tfirst[c] == (unsigned)s; }
  int tot;
  const int r = block_rank(first, &tot);
  if (!first) return;
  const int d = v.koff[blockIdx.x] + r;
  v.keys[d] = c;
  v.win[d] = (int)v.tbest[c];
}

// bucket count of the container after K insertions (the last rehash of the schedule that K keys reach)
__device__ __forceinline__ int buckets_of(const int* __restrict__ sched_cnt, const int* __restrict__ sched_nb, int nsched, int K) {
  int nb = 1;
  for (int i = 0; i < nsched && sched_cnt[i] < (K > 1 ? K : 1); i++) nb = sched_nb[i];
  return nb;
}

__global__ __launch_bounds__(64) void win_order_kernel(WinView v, int64_t* __restrict__ out_offs, int* __restrict__ info) {
  __shared__ int lds[WIN_ORDER_LDS_INTS];
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int* st = v.st;
  const int K = st[WS_K];
  int path = 0;
  if (K > 0) {
    const int nb = buckets_of(v.sched_cnt, v.sched_nb, v.nsched, K);
    if ((long long)K + nb <= WIN_ORDER_LDS_INTS) hash_order(v.keys, K, v.sched_cnt, v.sched_nb, v.nsched, lds, lds + K, v.order);
    else { hash_order(v.keys, K, v.sched_cnt, v.sched_nb, v.nsched, v.next, v.bkt, v.order); path = WIN_ORDER_GLOBAL; }
  }
  out_offs[0] = 0; out_offs[1] = st[WS_NOUT];
  info[0] = st[WS_EMIT]; info[1] = st[WS_NOUT]; info[2] = st[WS_ALIVE]; info[3] = st[WS_FLAGS] | path;
}

__global__ __launch_bounds__(FRAME_THREADS) void win_gather_kernel(WinView v, const double* __restrict__ pose, double* __restrict__ oxyz,
                                                                   float* __restrict__ oint, double* __restrict__ frame) {
  if (!v.st[WS_EMIT]) {                                                    // no cloud: an all-zero frame (point count 0, no average)
    if (threadIdx.x < 16) frame[threadIdx.x] = 0.0;
    return;
  }
  gather_frames_cloud((int64_t)v.st[WS_NOUT], v.order, v.win, v.xyz[v.st[WS_DST]], v.inten[v.st[WS_DST]], pose, v.grid.range, oxyz, oint,
                      frame);
}

__global__ __launch_bounds__(256) void win_clear_kernel(WinView v) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (!v.st[WS_EMIT] || s >= v.st[WS_ALIVE]) return;
  const int c = v.cell[s];
  v.tval[c] = ~0ull; v.tfirst[c] = ~0u; v.tbest[c] = ~0u;
}

}  // namespace

void window_fill_grid(WinView& v, double range, int polar) { v.grid = make_grid(range, polar); }

void launch_window_reset(hipStream_t st, const WinView& v) { hipLaunchKernelGGL(win_reset_kernel, dim3(1), dim3(64), 0, st, v); }

void launch_window_push(hipStream_t st, const WinView& v, const double* pose, const double* xyz_new, const float* inten_new,
                        const int* n_new_dev, int max_new, double* out_xyz, float* out_inten, int64_t* out_offs, double* out_frame, int* info) {
  const unsigned nblk = (unsigned)((v.cap + 255) / 256), nnew = (unsigned)((v.max_new + 255) / 256);
  hipLaunchKernelGGL(win_state_kernel, dim3(1), dim3(64), 0, st, v, pose, n_new_dev, max_new);
  hipLaunchKernelGGL(win_append_kernel, dim3(nnew), dim3(256), 0, st, v, xyz_new, inten_new);
  hipLaunchKernelGGL(win_count_kernel, dim3(nblk), dim3(256), 0, st, v, pose);
  hipLaunchKernelGGL(win_scan_kernel, dim3(1), dim3(256), 0, st, v, 0);
  hipLaunchKernelGGL(win_scatter_kernel, dim3(nblk), dim3(256), 0, st, v, pose);
  hipLaunchKernelGGL(win_winners_kernel, dim3(nblk), dim3(256), 0, st, v);
  hipLaunchKernelGGL(win_scan_kernel, dim3(1), dim3(256), 0, st, v, 1);
  hipLaunchKernelGGL(win_keys_kernel, dim3(nblk), dim3(256), 0, st, v);
  hipLaunchKernelGGL(win_order_kernel, dim3(1), dim3(64), 0, st, v, out_offs, info);
  hipLaunchKernelGGL(win_gather_kernel, dim3(1), dim3(FRAME_THREADS), 0, st, v, pose, out_xyz, out_inten, out_frame);
  hipLaunchKernelGGL(win_clear_kernel, dim3(nblk), dim3(256), 0, st, v);
}

}  // namespace pr
