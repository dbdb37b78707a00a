// eval.hip — the evaluation half of match_signatures/run_test.m on the device: ground-truth loop pairs (:3-22) and the precision / recall
// sweep with top recall, lp_detected and the trapz AUC (:58-85).  The oracle is pr_ref_precision_recall (oracle/pr_ref.cpp), line for line;
// this file is compiled with -ffp-contract=off, every product and every sum below is rounded on its own as there.
//
// Ground truth: a masked brute-force nearest neighbour in fp64 with a FIRST-minimum rule.  A workgroup of 256 lanes owns 256 rq queries
// (rq = 1 | 4 per lane, their coordinates in registers) and a contiguous range of gt2 rows (grid.y splits n so that a small m still fills the
// chip), which it stages through LDS EVAL_TILE rows at a time; every lane reads the same row (a broadcast read) and walks j upwards with
// the reference's strict update `min_diff > diff` from (+Inf, -1): a NaN or +Inf diff never wins.  A tile no query of the workgroup can
// mask runs without the mask test.  Per-split (d, j) partials are combined by "smaller d, then smaller j" - the first-minimum rule under
// any partition, so the result does not depend on the launch geometry.  No floating-point atomics, no matrix cores.
//
// Sweep: the rank of query a is the number of queries in front of it under (key, index), key = a sortable u64 image of diff_v with every
// NaN after +Inf and -0.0 == +0.0: the total order std::stable_sort realises with the comparator of pr_ref.cpp:759-763.  The count is a
// tiled all-pairs pass (integer atomics gather the splits: exact whatever their order).  The ranks are classified, tp is an integer scan,
// precision / recall are IEEE divisions, the trapz terms are formed in parallel and added from 0.0 in index order by ONE lane: the
// reference's order is the value.
#include "kernels.hpp"

#include <limits.h>

namespace pr {
namespace {

constexpr int EV_THREADS = 256;
constexpr int RK_TILE = 1024;                   // keys per LDS tile of the rank count
constexpr int CHAIN = 2048;                     // trapz terms per LDS buffer of the ordered sum

// ------------------------------------------------------------------ ground-truth pairs
// C = 1..3: coordinates in registers, R queries per lane; C = 0: any cols, one query per lane, coordinates re-read (L1) per pair
template <int C, int R>
__global__ __launch_bounds__(EV_THREADS) void gt_kernel(const double* __restrict__ gt1, int m, const double* __restrict__ gt2, int n, int cols,
                                                         int mw, int chunk, double* __restrict__ out_d, int* __restrict__ out_j) {
  __shared__ double tile[EVAL_TILE * 3];
  const int i0 = blockIdx.x * (EV_THREADS * R), i1 = min(m, i0 + EV_THREADS * R) - 1;
  const int jbeg = blockIdx.y * chunk, jend = min(n, jbeg + chunk);
  constexpr int CC = C ? C : 1;
  double q[R][CC], bd[R];
  int qi[R], bj[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    qi[r] = i0 + r * EV_THREADS + threadIdx.x;
    bd[r] = INFINITY; bj[r] = -1;
#pragma unroll
    for (int c = 0; c < CC; c++) q[r][c] = (C && qi[r] < m) ? gt1[(size_t)qi[r] * C + c] : 0.0;
  }
  const int rows = C ? EVAL_TILE : (EVAL_TILE * 3) / cols;          // cols <= EVAL_MAX_COLS: at least one row
  for (int j0 = jbeg; j0 < jend; j0 += rows) {
    const int jn = min(rows, jend - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < jn * cols; e += EV_THREADS) tile[e] = gt2[(size_t)j0 * cols + e];
    __syncthreads();
    // masked are i - mw < j < i + mw: no query of [i0, i1] masks a row of this tile when it lies at or below i0 - mw or at or above i1 + mw
    const bool clear = mw <= 0 || (long long)j0 + jn - 1 <= (long long)i0 - mw || (long long)j0 >= (long long)i1 + mw;
    if constexpr (C > 0) {
      if (clear) {
#pragma unroll 4
        for (int jj = 0; jj < jn; jj++) {
          double g[CC];
#pragma unroll
          for (int c = 0; c < CC; c++) g[c] = tile[jj * C + c];
#pragma unroll
          for (int r = 0; r < R; r++) {
            double t = q[r][0] - g[0];
            double d = t * t;                                       // 0 + t^2 is t^2
#pragma unroll
            for (int c = 1; c < CC; c++) { t = q[r][c] - g[c]; d = d + t * t; }
            if (bd[r] > d) { bd[r] = d; bj[r] = j0 + jj; }
          }
        }
      } else {
#pragma unroll 2
        for (int jj = 0; jj < jn; jj++) {
          double g[CC];
#pragma unroll
          for (int c = 0; c < CC; c++) g[c] = tile[jj * C + c];
#pragma unroll
          for (int r = 0; r < R; r++) {
            double t = q[r][0] - g[0];
            double d = t * t;
#pragma unroll
            for (int c = 1; c < CC; c++) { t = q[r][c] - g[c]; d = d + t * t; }
            if (abs(qi[r] - (j0 + jj)) >= mw && bd[r] > d) { bd[r] = d; bj[r] = j0 + jj; }
          }
        }
      }
    } else {
      if (qi[0] < m) {
        const double* a = gt1 + (size_t)qi[0] * cols;
        for (int jj = 0; jj < jn; jj++) {
          if (!clear && abs(qi[0] - (j0 + jj)) < mw) continue;
          double d = 0.0;
          for (int c = 0; c < cols; c++) { const double t = a[c] - tile[jj * cols + c]; d = d + t * t; }
          if (bd[0] > d) { bd[0] = d; bj[0] = j0 + jj; }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; r++)
    if (qi[r] < m) {
      out_d[(size_t)blockIdx.y * m + qi[r]] = bd[r];
      out_j[(size_t)blockIdx.y * m + qi[r]] = bj[r];
    }
}

__global__ void gt_combine_kernel(const double* __restrict__ pd, const int* __restrict__ pj, int m, int nsplit, double* __restrict__ min_d,
                                  int* __restrict__ min_j) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double bd = INFINITY;
  int bj = -1;
  for (int s = 0; s < nsplit; s++) {
    const double d = pd[(size_t)s * m + i];
    const int j = pj[(size_t)s * m + i];
    if (j >= 0 && (d < bd || (d == bd && j < bj))) { bd = d; bj = j; }     // smaller d, then smaller j; (+Inf, -1) = no candidate
  }
  min_d[i] = bd;
  min_j[i] = bj;
}

// ------------------------------------------------------------------ two-level integer scan (EVAL_SCAN items per workgroup)
// inclusive scan of one value per lane over a workgroup of EVAL_SCAN lanes; ws: 17 ints of LDS; the total is ws[16] (valid until the next call)
__device__ __forceinline__ int block_scan(int v, int* ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  __syncthreads();
  if (lane == 63) ws[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0;
    for (int k = 0; k < EVAL_SCAN / 64; k++) { const int t = ws[k]; ws[k] = a; a += t; }
    ws[16] = a;
  }
  __syncthreads();
  return v + ws[w];
}

// loc[i] = inclusive count of flags within i's workgroup, bsum[block] = the workgroup's count.  flag: min_d[i] < thr (min_d given) or cls[i]
__global__ __launch_bounds__(EVAL_SCAN) void flag_scan_kernel(const double* __restrict__ min_d, double thr, const int* __restrict__ cls, int m,
                                                               int* __restrict__ loc, int* __restrict__ bsum) {
  __shared__ int ws[17];
  const int i = blockIdx.x * EVAL_SCAN + threadIdx.x;
  int f = 0;
  if (i < m) f = min_d ? (min_d[i] < thr ? 1 : 0) : cls[i];
  const int s = block_scan(f, ws);
  if (i < m) loc[i] = s;
  if (threadIdx.x == 0) bsum[blockIdx.x] = ws[16];
}

// boff[b] = sum of bsum[0 .. b - 1], *total = their sum; *init = init_v (the sweep's first-fp word starts at m)
__global__ __launch_bounds__(EVAL_SCAN) void sums_scan_kernel(const int* __restrict__ bsum, int nb, int* __restrict__ boff, int32_t* total,
                                                               int32_t* init, int init_v) {
  __shared__ int ws[17];
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += EVAL_SCAN) {
    const int b = b0 + threadIdx.x;
    const int v = b < nb ? bsum[b] : 0;
    const int s = block_scan(v, ws);
    if (b < nb) boff[b] = carry + s - v;
    carry += ws[16];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (total) *total = carry;
    if (init) *init = init_v;
  }
}

__global__ __launch_bounds__(EVAL_SCAN) void gt_write_kernel(const double* __restrict__ min_d, const int* __restrict__ min_j, int m, double thr,
                                                              const int* __restrict__ loc, const int* __restrict__ boff, int32_t* __restrict__ lp) {
  const int i = blockIdx.x * EVAL_SCAN + threadIdx.x;
  if (i >= m || !(min_d[i] < thr)) return;
  const int pos = boff[blockIdx.x] + loc[i] - 1;                  // < m: a count of flags among i' <= i
  lp[2 * (size_t)pos] = i;
  lp[2 * (size_t)pos + 1] = min_j[i];
}

// ------------------------------------------------------------------ sweep
// ascending u64 image of the comparator of pr_ref.cpp:759-763: x < y on the numbers, -0.0 == +0.0, every NaN equal and after +Inf
__device__ __forceinline__ unsigned long long sort_key(double x) {
  if (x != x) return ~0ull;
  if (x == 0.0) x = 0.0;
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// cnt[a] += the queries of [blockIdx.y chunk, + chunk) in front of a under (key, index)
__global__ __launch_bounds__(EV_THREADS) void rank_count_kernel(const double* __restrict__ diff_v, int ld, int m, int chunk, int* __restrict__ cnt) {
  __shared__ unsigned long long keys[RK_TILE];
  const int a0 = blockIdx.x * EV_THREADS, a = a0 + threadIdx.x, a1 = min(m, a0 + EV_THREADS) - 1;
  const unsigned long long ka = a < m ? sort_key(diff_v[(size_t)a * ld]) : 0ull;
  const int bbeg = blockIdx.y * chunk, bend = min(m, bbeg + chunk);
  int c = 0;
  for (int b0 = bbeg; b0 < bend; b0 += RK_TILE) {
    const int bn = min(RK_TILE, bend - b0);
    __syncthreads();
    for (int e = threadIdx.x; e < bn; e += EV_THREADS) keys[e] = sort_key(diff_v[(size_t)(b0 + e) * ld]);
    __syncthreads();
    if (b0 + bn - 1 < a0) {                      // every b in front of every a of the workgroup: ties count
#pragma unroll 8
      for (int e = 0; e < bn; e++) c += keys[e] <= ka ? 1 : 0;
    } else if (b0 > a1) {                        // every b behind: ties do not
#pragma unroll 8
      for (int e = 0; e < bn; e++) c += keys[e] < ka ? 1 : 0;
    } else {
      for (int e = 0; e < bn; e++) c += (keys[e] < ka || (keys[e] == ka && b0 + e < a)) ? 1 : 0;
    }
  }
  if (a < m && c) atomicAdd(&cnt[a], c);
}

__device__ __forceinline__ double pos_d2(const double* __restrict__ a, const double* __restrict__ b, int cols) {
  double s = 0.0;
  for (int c = 0; c < cols; c++) { const double t = a[c] - b[c]; s = s + t * t; }
  return s;
}

// run_test.m:67-75 at the query's place in the order: rank[pos] = a, bidx[pos] = its match (-1 read as 0), cls[pos] = 1 for a tp
__global__ void classify_kernel(const int32_t* __restrict__ diff_idx, int ld, int m, const double* __restrict__ gt1, const double* __restrict__ gt2,
                                int n, int cols, double thr, const int* __restrict__ cnt, int* __restrict__ rank, int* __restrict__ bidx,
                                int* __restrict__ cls) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const int pos = cnt[a];
  if ((unsigned)pos >= (unsigned)m) return;      // (cannot happen: the order is total)
  int b = diff_idx[(size_t)a * ld];
  if (b < 0) b = 0;
  const bool tp = b < n && pos_d2(gt1 + (size_t)a * cols, gt2 + (size_t)b * cols, cols) < thr;
  rank[pos] = a;
  bidx[pos] = b;
  cls[pos] = tp ? 1 : 0;
}

// run_test.m:76-77 and the trapz terms: term[i - 1] = ((recall[i] - recall[i - 1]) * (precision[i - 1] + precision[i])) / 2;
// scal->n_detected (set to m by sums_scan_kernel) = the first fp's rank
__global__ __launch_bounds__(EVAL_SCAN) void points_kernel(const int* __restrict__ cls, const int* __restrict__ loc, const int* __restrict__ boff,
                                                            int m, double* __restrict__ prec, double* __restrict__ rec, double* __restrict__ term,
                                                            EvalScalars* __restrict__ scal) {
  __shared__ int first;
  if (threadIdx.x == 0) first = INT_MAX;
  __syncthreads();
  const int i = blockIdx.x * EVAL_SCAN + threadIdx.x;
  if (i < m) {
    const int L = scal->n_gt;
    const double total = L == 0 ? 0.0 : (double)(L < 2 ? 2 : L);   // MATLAB length() of an L x 2 matrix (:22)
    const int c = cls[i], tp = boff[blockIdx.x] + loc[i];
    const double p = (double)tp / (double)(i + 1), r = (double)tp / total;
    prec[i] = p;
    rec[i] = r;
    if (i > 0) {
      const double pp = (double)(tp - c) / (double)i, rp = (double)(tp - c) / total;
      term[i - 1] = ((r - rp) * (pp + p)) / 2.0;
    }
    if (!c) atomicMin(&first, i);
  }
  __syncthreads();
  if (threadIdx.x == 0 && first != INT_MAX) atomicMin(&scal->n_detected, first);
}

__global__ void trapz_terms_kernel(const double* __restrict__ rec, const double* __restrict__ prec, int m, double* __restrict__ term) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 < m) term[i] = ((rec[i + 1] - rec[i]) * (prec[i] + prec[i + 1])) / 2.0;
}

// One workgroup: lane 0 adds term[0 .. nt - 1] to 0.0 in index order out of LDS while the others stage the next CHAIN terms;
// with scal: also top_recall and lp_detected of the n_detected ranks in front of the first fp (:79-85)
__global__ __launch_bounds__(EVAL_SCAN) void chain_kernel(const double* __restrict__ term, int nt, double* __restrict__ out, EvalScalars* scal,
                                                           const double* __restrict__ rec, const int* __restrict__ rank,
                                                           const int* __restrict__ bidx, int32_t* __restrict__ lp_detected) {
  __shared__ double buf[2][CHAIN];
  double area = 0.0;
  for (int e = threadIdx.x; e < min(CHAIN, nt); e += EVAL_SCAN) buf[0][e] = term[e];
  __syncthreads();
  for (int t0 = 0, k = 0; t0 < nt; t0 += CHAIN, k ^= 1) {
    const int nx = min(CHAIN, nt - t0 - CHAIN);
    for (int e = threadIdx.x; e < nx; e += EVAL_SCAN) buf[k ^ 1][e] = term[t0 + CHAIN + e];
    if (threadIdx.x == 0) {
      const int tn = min(CHAIN, nt - t0);
      const double* b = buf[k];
#pragma unroll 8
      for (int e = 0; e < tn; e++) area = area + b[e];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = area;
  if (!scal) return;
  const int top = scal->n_detected;
  if (threadIdx.x == 0) scal->top_recall = top > 0 ? rec[top - 1] : 0.0;
  if (lp_detected)
    for (int i = threadIdx.x; i < top; i += EVAL_SCAN) {
      lp_detected[2 * (size_t)i] = rank[i];
      lp_detected[2 * (size_t)i + 1] = bidx[i];
    }
}

template <int C, int R>
void gt_launch(hipStream_t st, dim3 grid, const double* gt1, int m, const double* gt2, int n, int cols, int mw, int chunk, double* out_d, int* out_j) {
  hipLaunchKernelGGL((gt_kernel<C, R>), grid, dim3(EV_THREADS), 0, st, gt1, m, gt2, n, cols, mw, chunk, out_d, out_j);
}

}  // namespace

void launch_eval_gt(hipStream_t st, const double* gt1, int m, const double* gt2, int n, int cols, int mask_width, int chunk, int nsplit, int rq,
                    double* out_d, int* out_j) {
  if (m <= 0) return;
  if (cols > 3) rq = 1;
  const dim3 grid((m + EV_THREADS * rq - 1) / (EV_THREADS * rq), nsplit);
  if (cols == 1) rq == 4 ? gt_launch<1, 4>(st, grid, gt1, m, gt2, n, cols, mask_width, chunk, out_d, out_j)
                         : gt_launch<1, 1>(st, grid, gt1, m, gt2, n, cols, mask_width, chunk, out_d, out_j);
  else if (cols == 2) rq == 4 ? gt_launch<2, 4>(st, grid, gt1, m, gt2, n, cols, mask_width, chunk, out_d, out_j)
                              : gt_launch<2, 1>(st, grid, gt1, m, gt2, n, cols, mask_width, chunk, out_d, out_j);
  else if (cols == 3) rq == 4 ? gt_launch<3, 4>(st, grid, gt1, m, gt2, n, cols, mask_width, chunk, out_d, out_j)
                              : gt_launch<3, 1>(st, grid, gt1, m, gt2, n, cols, mask_width, chunk, out_d, out_j);
  else gt_launch<0, 1>(st, grid, gt1, m, gt2, n, cols, mask_width, chunk, out_d, out_j);
}

void launch_eval_gt_combine(hipStream_t st, const double* part_d, const int* part_j, int m, int nsplit, double* min_d, int* min_j) {
  if (m <= 0) return;
  hipLaunchKernelGGL(gt_combine_kernel, dim3((m + 255) / 256), dim3(256), 0, st, part_d, part_j, m, nsplit, min_d, min_j);
}

void launch_eval_gt_pairs(hipStream_t st, const double* min_d, const int* min_j, int m, double thr, int* loc, int* bsum, int32_t* lp, int32_t* n_gt) {
  const int nb = (m + EVAL_SCAN - 1) / EVAL_SCAN;
  if (nb > 0) hipLaunchKernelGGL(flag_scan_kernel, dim3(nb), dim3(EVAL_SCAN), 0, st, min_d, thr, (const int*)nullptr, m, loc, bsum);
  hipLaunchKernelGGL(sums_scan_kernel, dim3(1), dim3(EVAL_SCAN), 0, st, bsum, nb, bsum + nb + 1, n_gt, (int32_t*)nullptr, 0);
  if (nb > 0 && lp) hipLaunchKernelGGL(gt_write_kernel, dim3(nb), dim3(EVAL_SCAN), 0, st, min_d, min_j, m, thr, loc, bsum + nb + 1, lp);
}

void launch_eval_sweep(hipStream_t st, const double* diff_v, const int32_t* diff_idx, int ld, int m, const double* gt1, const double* gt2, int n,
                       int cols, double thr, int* cnt, int* rank, int* bidx, int* cls, int* loc, int* bsum, double* prec, double* rec,
                       double* term, EvalScalars* scal, int32_t* lp_detected) {
  const int nb = (m + EVAL_SCAN - 1) / EVAL_SCAN;
  if (m > 0) {
    (void)hipMemsetAsync(cnt, 0, (size_t)m * sizeof(int), st);
    const int ab = (m + EV_THREADS - 1) / EV_THREADS, tiles = (m + RK_TILE - 1) / RK_TILE;
    int split = (1024 + ab - 1) / ab;
    split = split < 1 ? 1 : (split > tiles ? tiles : split);
    const int per = (tiles + split - 1) / split;
    split = (tiles + per - 1) / per;
    hipLaunchKernelGGL(rank_count_kernel, dim3(ab, split), dim3(EV_THREADS), 0, st, diff_v, ld, m, per * RK_TILE, cnt);
    hipLaunchKernelGGL(classify_kernel, dim3(ab), dim3(EV_THREADS), 0, st, diff_idx, ld, m, gt1, gt2, n, cols, thr, cnt, rank, bidx, cls);
    hipLaunchKernelGGL(flag_scan_kernel, dim3(nb), dim3(EVAL_SCAN), 0, st, (const double*)nullptr, 0.0, cls, m, loc, bsum);
  }
  hipLaunchKernelGGL(sums_scan_kernel, dim3(1), dim3(EVAL_SCAN), 0, st, bsum, nb, bsum + nb + 1, (int32_t*)nullptr, &scal->n_detected, m);
  if (m > 0) hipLaunchKernelGGL(points_kernel, dim3(nb), dim3(EVAL_SCAN), 0, st, cls, loc, bsum + nb + 1, m, prec, rec, term, scal);
  hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(EVAL_SCAN), 0, st, term, m > 0 ? m - 1 : 0, &scal->auc, scal, rec, rank, bidx, lp_detected);
}

void launch_eval_trapz(hipStream_t st, const double* rec, const double* prec, int m, double* term, double* out) {
  if (m > 1) hipLaunchKernelGGL(trapz_terms_kernel, dim3((m + 255) / 256), dim3(256), 0, st, rec, prec, m, term);
  hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(EVAL_SCAN), 0, st, term, m > 1 ? m - 1 : 0, out, (EvalScalars*)nullptr, (const double*)nullptr,
                     (const int*)nullptr, (const int*)nullptr, (int32_t*)nullptr);
}

}  // namespace pr
