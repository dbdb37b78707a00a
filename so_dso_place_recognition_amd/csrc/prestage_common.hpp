// prestage_common.hpp — the device arithmetic of the pre-stage (utils/pts_preprocess.h:135-232) that the batch form (prestage.hip) and the
// keyframe-at-a-time form (window.hip) share: camera transform + range test, cell id + ordering value, the ordered 0/1 compaction rank of a
// workgroup, and the one-workgroup-per-cloud emission that also leaves the cloud's PCA frame.  One copy, so that both forms decide and emit
// with the same bits.  Device code; include in files compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "frames.hpp"
#include "kernels.hpp"

namespace pr {

__device__ __forceinline__ bool to_camera(const double* __restrict__ w, const double* __restrict__ g, double range, double* l) {
#pragma unroll
  for (int r = 0; r < 3; r++) l[r] = ((w[4 * r] * g[0] + w[4 * r + 1] * g[1]) + w[4 * r + 2] * g[2]) + w[4 * r + 3] * 1.0;   // :141-142
  const double nrm = sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
  return nrm < range;                                                                                                   // :144
}

// block-wide exclusive scan of 0/1 flags (256 threads = 4 waves); returns this thread's rank and the block total
__device__ __forceinline__ int block_rank(bool flag, int* total) {
  __shared__ int wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int r = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { if (i < w) base += wsum[i]; tot += wsum[i]; }
  __syncthreads();
  *total = tot;
  return base + r;
}

__device__ __forceinline__ unsigned long long orderable(double v) {   // monotone map double -> u64 (-0.0 == +0.0)
  v = v + 0.0;
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ void cell_of(const Grid& g, const double* l, int* cell, unsigned long long* val) {
  if (g.polar) {                                                            // :100-119
    const double xz = sqrt(l[0] * l[0] + l[2] * l[2]);
    const int azi = (int)floor((atan2(l[2], l[0]) + M_PI) * g.inv);
    const int ele = (int)floor((atan2(l[1], xz) + M_PI / 2) * g.inv);
    *cell = azi + ele * g.azi_bins;
    *val = orderable(sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]));
  } else {                                                                  // :55-80
    const int xi = (int)floor((l[0] + g.range) * g.step[0]);
    const int yi = (int)floor((l[1] + g.range) * g.step[1]);
    const int zi = (int)floor((l[2] + g.range) * g.step[2]);
    *cell = xi + yi * g.dim[0] + zi * g.dim[0] * g.dim[1];
    *val = orderable(l[1]);
  }
}

inline Grid make_grid(double range, int polar) {
  Grid g;
  g.range = range;
  g.polar = polar;
  const double res[3] = {30, 60, 30};
  for (int a = 0; a < 3; a++) {                                 // :55-60
    const double r = range / res[a];
    g.step[a] = 1.0 / r;
    g.dim[a] = (int)(floor(2 * range * g.step[a]) + 1);
  }
  const double pres = 1.0 / 180.0 * M_PI;                       // :100-103
  g.inv = 1.0 / pres;
  g.azi_bins = (int)(floor(2 * M_PI * g.inv) + 1);
  return g;
}

// Emission of ONE cloud by one workgroup of FRAME_THREADS threads: output point i is the winner win[order[i]] of the i-th key of the
// iteration order, transformed again, with its intensity.  Thread t emits points t, t + 256, ... - the order in which cloud_frames_kernel
// (sc_gen.hip) reads them - and both use reduce_moments_to_frame, so the frame has the bits a moments pass over the emitted cloud would
// produce; the float intensity average is added too (frame[14], [15] = 1), and the generators then run their binning pass only
// (pr_*_generate_frames_dev).  oxyz / oint point at the cloud's first output point.
__device__ __forceinline__ void gather_frames_cloud(int64_t P, const int* __restrict__ order, const int* __restrict__ win,
                                                    const double* __restrict__ xyz, const float* __restrict__ inten,
                                                    const double* __restrict__ w, double range, double* __restrict__ oxyz,
                                                    float* __restrict__ oint, double* __restrict__ frame) {
  __shared__ double red[FRAME_THREADS / 64][9];
  __shared__ __attribute__((aligned(16))) float stage[2][2048 + 32];
  const int tid = threadIdx.x;
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double pv[3] = {0, 0, 0};                         // the pivot of the moments (frames.hpp): the first emitted point, as every thread computes it
  if (P > 0) {
    const int j = win[order[0]];
    const double gp[3] = {xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2]};
    (void)to_camera(w, gp, range, pv);
  }
  for (int64_t i = tid; i < P; i += FRAME_THREADS) {
    const int j = win[order[i]];
    const double gp[3] = {xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2]};
    double l[3];
    (void)to_camera(w, gp, range, l);
    oxyz[3 * i] = l[0]; oxyz[3 * i + 1] = l[1]; oxyz[3 * i + 2] = l[2];
    oint[i] = inten[j];
    const double x = l[0] - pv[0], y = l[1] - pv[1], z = l[2] - pv[2];
    s[0] += x; s[1] += y; s[2] += z;
    s[3] += x * x; s[4] += x * y; s[5] += x * z; s[6] += y * y; s[7] += y * z; s[8] += z * z;
  }
  reduce_moments_to_frame(s, (double)P, pv, red, frame);
  // ... and the reference's float average of the emitted intensities (in emission order), so that the generators have nothing left to do
  // but their binning pass
  __threadfence_block();
  __syncthreads();                                 // this workgroup's oint stores are visible to it
  const float a = block_sequential_average(oint, P, stage);
  if (tid == 0) { frame[14] = (double)a; frame[15] = 1.0; }
}

}  // namespace pr
