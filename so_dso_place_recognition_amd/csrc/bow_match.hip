// bow_match.hip — an inverted-file (word-major CSR) form of processBoW.m:1-38 + run_test.m:47-57 on gfx950, exact in fp64.
//
// processBoW.m's merge adds, per (query, entry) pair and in ascending word order, ((score + |va - vb|) - |va|) - |vb| for every common
// word and ends with d = 1 - (-score / 2).  For CONFORMING rows (ids integers in [0, n_words), strictly ascending up to the terminator:
// what test_bow.cpp and bow_generate write) the merge visits exactly the set intersection of the two word lists, in ascending order.  So
// when every pair's accumulator receives its common words' terms in ascending word order, with this expression, from +0.0, the result
// is the merge's bit for bit - whichever thread applies a term and however the postings of one word are laid out.  An entry without a
// common word keeps +0.0 and gets d = 1.0 from the same formula.
//
//   bow_rows_check : one workgroup per row: the readable length (first column p < cols - 1 with !(id > -1); the last column is never read,
//                    as in the reference), conformance of the ids before it, the per-word posting counts and the total.  The first
//                    non-conforming row (global number) is left in `bad` by atomicMin.
//   bow_scan_*     : exclusive scan of the counts into 64-bit offsets [n_words + 1] (tile sums, one workgroup over the tile sums, apply),
//                    the cursor of the scatter a copy of the offsets.
//   bow_scatter    : postings (row, weight) into the word-major lists through an atomic cursor per word.  The order inside a word is
//                    not defined and does not matter: the postings of one word belong to distinct rows.
//   bow_fold       : main + tail -> one list per word (the main segment's postings, then the tail's): new offsets are the sums of the
//                    two segments' offsets.
//   bow_score      : one workgroup per query of a chunk over an fp64 accumulator row [n] in global scratch: zero it, walk the query's words
//                    in ascending order, all threads apply the word's postings (main, then tail - distinct rows), a workgroup barrier
//                    between two words (the next word reads what this one stored).  Then d, the mask on global row numbers (+Inf), and
//                    the k smallest (d, j) - ties to the lower index, NaN never selected, -1 / NaN fill (pr_ref_select_topk).  A
//                    non-conforming query row gets -1 / NaN in all k slots and raises flag[0] (PR_WARN_BOW_ROWS).  k = 0: the row of d
//                    stays in the accumulator (the exact distance matrix of pr_bow_distance_f64).
// Built with -ffp-contract=off (Makefile), like bow_gen.hip (the accumulation has no products; the flag keeps it so if it ever gets some).
#include <climits>

#include "kernels.hpp"

namespace pr {
namespace {

constexpr int CBT = 256;                        // threads of the row kernels
typedef unsigned long long u64;

__device__ __forceinline__ bool bow_before(double av, int aj, double bv, int bj) { return av < bv || (av == bv && aj < bj); }

// readable length of a row (all threads return it); s_len: an LDS word
template <int BT>
__device__ __forceinline__ int bow_row_length(const double* __restrict__ ids, int cols, int* s_len) {
  if (threadIdx.x == 0) *s_len = cols - 1;
  __syncthreads();
  for (int p = threadIdx.x; p < cols - 1; p += BT)
    if (!(ids[p] > -1.0)) atomicMin(s_len, p);
  __syncthreads();
  return *s_len;
}

// conformance of column p < length: an integer id in [0, n_words) above the previous one (id > -1 holds before the terminator)
__device__ __forceinline__ bool bow_id_ok(const double* __restrict__ ids, int p, int n_words) {
  const double x = ids[p];
  return x == rint(x) && x < (double)n_words && (p == 0 || x > ids[p - 1]);
}

__global__ __launch_bounds__(CBT) void bow_rows_check_kernel(const double* __restrict__ rows, int cols, int n_words, int row_name0,
                                                             int* __restrict__ counts, u64* __restrict__ total, int* __restrict__ bad) {
  __shared__ int s_len, s_bad;
  const int r = blockIdx.x;
  const double* ids = rows + (size_t)(2 * r) * cols;
  if (threadIdx.x == 0) s_bad = 0;
  const int L = bow_row_length<CBT>(ids, cols, &s_len);
  for (int p = threadIdx.x; p < L; p += CBT) {
    if (!bow_id_ok(ids, p, n_words)) s_bad = 1;
    else if (counts) atomicAdd(&counts[(int)ids[p]], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_bad) atomicMin(bad, row_name0 + r);
    if (total) atomicAdd(total, (u64)L);
  }
}

__global__ __launch_bounds__(CBT) void bow_scatter_kernel(const double* __restrict__ rows, int cols, int j0, u64* __restrict__ cursor,
                                                          int* __restrict__ prow, double* __restrict__ pw) {
  __shared__ int s_len;
  const int r = blockIdx.x;
  const double* ids = rows + (size_t)(2 * r) * cols;
  const int L = bow_row_length<CBT>(ids, cols, &s_len);
  for (int p = threadIdx.x; p < L; p += CBT) {
    const u64 pos = atomicAdd(&cursor[(int)ids[p]], 1ull);
    prow[pos] = j0 + r;
    pw[pos] = ids[cols + p];
  }
}

// ---- exclusive scan of int counts [nw] -> u64 offsets [nw + 1] (and the same into cursor): tiles of 1024, 4 per thread
constexpr int STILE = 4 * CBT;

__device__ __forceinline__ u64 block_excl_scan(u64 v, u64* sh, u64* tot) {   // CBT threads; sh: 4 LDS words
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  u64 base = 0, all = 0;
#pragma unroll
  for (int i = 0; i < CBT / 64; i++) { if (i < w) base += sh[i]; all += sh[i]; }
  __syncthreads();
  *tot = all;
  return base + incl - v;
}

__global__ __launch_bounds__(CBT) void bow_scan_sums_kernel(const int* __restrict__ counts, int nw, u64* __restrict__ tsum) {
  __shared__ u64 sh[CBT / 64];
  const int base = blockIdx.x * STILE + 4 * threadIdx.x;
  u64 s = 0;
#pragma unroll
  for (int e = 0; e < 4; e++) if (base + e < nw) s += (u64)counts[base + e];
  u64 tot;
  (void)block_excl_scan(s, sh, &tot);
  if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(CBT) void bow_scan_tiles_kernel(u64* __restrict__ tsum, int T, u64* __restrict__ off, u64* __restrict__ cursor,
                                                             int nw) {
  __shared__ u64 sh[CBT / 64];
  u64 carry = 0;
  for (int t0 = 0; t0 < T; t0 += CBT) {
    const int t = t0 + threadIdx.x;
    const u64 v = t < T ? tsum[t] : 0;
    u64 tot;
    const u64 ex = block_excl_scan(v, sh, &tot);
    if (t < T) tsum[t] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) { off[nw] = carry; cursor[nw] = carry; }
}

__global__ __launch_bounds__(CBT) void bow_scan_apply_kernel(const int* __restrict__ counts, int nw, const u64* __restrict__ tsum,
                                                             u64* __restrict__ off, u64* __restrict__ cursor) {
  __shared__ u64 sh[CBT / 64];
  const int base = blockIdx.x * STILE + 4 * threadIdx.x;
  u64 c[4], s = 0;
#pragma unroll
  for (int e = 0; e < 4; e++) { c[e] = base + e < nw ? (u64)counts[base + e] : 0; s += c[e]; }
  u64 tot;
  u64 x = tsum[blockIdx.x] + block_excl_scan(s, sh, &tot);
#pragma unroll
  for (int e = 0; e < 4; e++)
    if (base + e < nw) { off[base + e] = x; cursor[base + e] = x; x += c[e]; }
}

// one wave per word: main postings then tail postings into the new lists
__global__ __launch_bounds__(CBT) void bow_fold_kernel(int nw, const u64* __restrict__ moff, const int* __restrict__ mrow,
                                                       const double* __restrict__ mw, const u64* __restrict__ toff,
                                                       const int* __restrict__ trow, const double* __restrict__ tw,
                                                       u64* __restrict__ noff, int* __restrict__ nrow, double* __restrict__ nwt) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (CBT / 64) + (threadIdx.x >> 6);
  if (w >= nw) return;
  const u64 m0 = moff[w], mc = moff[w + 1] - m0, t0 = toff[w], tc = toff[w + 1] - t0, o = m0 + t0;
  for (u64 e = lane; e < mc; e += 64) { nrow[o + e] = mrow[m0 + e]; nwt[o + e] = mw[m0 + e]; }
  for (u64 e = lane; e < tc; e += 64) { nrow[o + mc + e] = trow[t0 + e]; nwt[o + mc + e] = tw[t0 + e]; }
  if (lane == 0) {
    noff[w] = o;
    if (w == nw - 1) noff[nw] = moff[nw] + toff[nw];
  }
}

// ---- scoring + selection
template <int BT>
struct ScoreLds {
  static constexpr int CAP = 8 * BT;             // survivors of the threshold pass
  union {
    struct { double va[BT]; u64 m0[BT], m1[BT], t0[BT], t1[BT]; } wb;   // one batch of the query's words
    struct { double lv[CAP]; int lj[CAP]; } sel;
  } u;
  double rv[BT];
  int rj[BT];
  double tau;
  int len, bad, cnt, ties, need;
};

template <int BT>
__device__ __forceinline__ void block_argmin(double& v, int& j, double* rv, int* rj) {   // (v, j), j < 0 = none; every thread gets the result
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const double ov = __shfl_xor(v, s, 64);
    const int oj = __shfl_xor(j, s, 64);
    if (oj >= 0 && (j < 0 || bow_before(ov, oj, v, j))) { v = ov; j = oj; }
  }
  if (BT > 64) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = v; rj[threadIdx.x >> 6] = j; }
    __syncthreads();
    for (int w = 0; w < BT / 64; w++) {
      const int oj = rj[w];
      if (oj >= 0 && (j < 0 || bow_before(rv[w], oj, v, j))) { v = rv[w]; j = oj; }
    }
    __syncthreads();
  }
}

template <int BT>
__global__ __launch_bounds__(BT) void bow_score_kernel(const double* __restrict__ q, int cols, int n_words, int q_row0,
                                                       const u64* __restrict__ moff, const int* __restrict__ mrow, const double* __restrict__ mw,
                                                       const u64* __restrict__ toff, const int* __restrict__ trow, const double* __restrict__ tw,
                                                       int n, int db_row0, int mask_width, int k, double* __restrict__ acc_base,
                                                       int32_t* __restrict__ idx, double* __restrict__ score, int* __restrict__ flag) {
  __shared__ ScoreLds<BT> S;
  constexpr int CAP = ScoreLds<BT>::CAP;
  const int tid = threadIdx.x, i = blockIdx.x;
  const double* ids = q + (size_t)(2 * i) * cols;
  const double* wts = ids + cols;
  double* acc = acc_base + (size_t)i * n;
  int32_t* oi = idx + (size_t)i * k;
  double* os = score + (size_t)i * k;
  const double NaN = __builtin_nan("");
  const double INF = __builtin_inf();

  if (tid == 0) S.bad = 0;
  const int L = bow_row_length<BT>(ids, cols, &S.len);
  for (int p = tid; p < L; p += BT)
    if (!bow_id_ok(ids, p, n_words)) S.bad = 1;
  __syncthreads();
  if (S.bad) {
    if (k > 0) for (int t = tid; t < k; t += BT) { oi[t] = -1; os[t] = NaN; }
    else for (int j = tid; j < n; j += BT) acc[j] = NaN;
    if (tid == 0) atomicOr(flag, 1);
    return;
  }
  for (int j = tid; j < n; j += BT) acc[j] = 0.0;
  __syncthreads();
  for (int p0 = 0; p0 < L; p0 += BT) {
    const int nb = min(BT, L - p0);
    if (tid < nb) {
      const int w = (int)ids[p0 + tid];
      S.u.wb.va[tid] = wts[p0 + tid];
      S.u.wb.m0[tid] = moff[w]; S.u.wb.m1[tid] = moff[w + 1];
      S.u.wb.t0[tid] = toff[w]; S.u.wb.t1[tid] = toff[w + 1];
    }
    __syncthreads();
    for (int t = 0; t < nb; t++) {
      const double va = S.u.wb.va[t], aa = fabs(va);
      const u64 m1 = S.u.wb.m1[t], t1 = S.u.wb.t1[t];
      for (u64 e = S.u.wb.m0[t] + tid; e < m1; e += BT) {
        const int j = mrow[e];
        const double vb = mw[e];
        acc[j] = ((acc[j] + fabs(va - vb)) - aa) - fabs(vb);            // processBoW.m:25, left to right
      }
      for (u64 e = S.u.wb.t0[t] + tid; e < t1; e += BT) {
        const int j = trow[e];
        const double vb = tw[e];
        acc[j] = ((acc[j] + fabs(va - vb)) - aa) - fabs(vb);
      }
      __syncthreads();                                                   // the next word reads these stores
    }
  }
  if (k == 0) {
    for (int j = tid; j < n; j += BT) acc[j] = 1.0 - (-acc[j] / 2.0);    // processBoW.m:37, :14
    return;
  }
  const long long ig = (long long)q_row0 + i;
  auto dval = [&](int j) -> double {
    double d = 1.0 - (-acc[j] / 2.0);
    long long dj = ig - ((long long)db_row0 + j);
    if (dj < 0) dj = -dj;
    if (dj < (long long)mask_width) d = INF;                             // run_test.m:47-53
    return d;
  };
  // pass A: every thread's minimum (NaN never selected)
  double mv = 0.0;
  int mj = -1;
  for (int j = tid; j < n; j += BT) {
    const double d = dval(j);
    if (d == d && (mj < 0 || d < mv)) { mv = d; mj = j; }               // j ascending per thread: strict < keeps the lower index
  }
  if (k == 1) {
    block_argmin<BT>(mv, mj, S.rv, S.rj);
    if (tid == 0) { oi[0] = mj < 0 ? -1 : db_row0 + mj; os[0] = mj < 0 ? NaN : mv; }
    return;
  }
  // tau = the k-th smallest thread minimum: k distinct elements are <= tau, so the k best all are (+Inf when fewer than k threads have one)
  S.rv[tid] = mv;
  S.rj[tid] = mj;
  if (tid == 0) { S.tau = INF; S.cnt = 0; S.ties = 0; }
  __syncthreads();
  if (mj >= 0) {
    int rank = 0;
    for (int t = 0; t < BT; t++) rank += (S.rj[t] >= 0 && bow_before(S.rv[t], S.rj[t], mv, mj));
    if (rank == k - 1) S.tau = mv;
  }
  __syncthreads();
  const double tau = S.tau;
  // pass B: every element <= tau into the list
  for (int j = tid; j < n; j += BT) {
    const double d = dval(j);
    if (d <= tau) {
      const int s = atomicAdd(&S.cnt, 1);
      if (s < CAP) { S.u.sel.lv[s] = d; S.u.sel.lj[s] = j; }
    }
  }
  __syncthreads();
  int cnt = S.cnt;
  bool listed = cnt <= CAP;
  if (!listed) {
    // masses of ties at tau (entries without a common word at d = 1, masked entries at +Inf): the elements below tau, then the ties in
    // index order, tile by tile, until k are listed
    __syncthreads();
    if (tid == 0) S.cnt = 0;
    __syncthreads();
    for (int j = tid; j < n; j += BT) {
      const double d = dval(j);
      if (d < tau) {
        const int s = atomicAdd(&S.cnt, 1);
        if (s < CAP) { S.u.sel.lv[s] = d; S.u.sel.lj[s] = j; }
      }
    }
    __syncthreads();
    cnt = S.cnt;
    if (cnt < k) {
      for (int j0 = 0; j0 < n; j0 += BT) {
        const int j = j0 + tid;
        if (j < n && dval(j) == tau) {
          const int s = atomicAdd(&S.cnt, 1);
          if (s < CAP) { S.u.sel.lv[s] = tau; S.u.sel.lj[s] = j; }
        }
        __syncthreads();
        const bool done = S.cnt >= k;
        __syncthreads();
        if (done) break;
      }
      cnt = S.cnt;
    }
    listed = cnt <= CAP;
  }
  if (listed) {
    // bitonic sort of the list padded to a power of two (>= 64) by (d, j); padding (+Inf, INT_MAX) sorts behind every real element
    int P = 64;
    while (P < cnt) P <<= 1;
    for (int s = cnt + tid; s < P; s += BT) { S.u.sel.lv[s] = INF; S.u.sel.lj[s] = INT_MAX; }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int e = tid; e < P / 2; e += BT) {
          const int pos = 2 * e - (e & (stride - 1)), par = pos + stride;
          const bool up = (pos & size) == 0;
          const double a = S.u.sel.lv[pos], b = S.u.sel.lv[par];
          const int aj = S.u.sel.lj[pos], bj = S.u.sel.lj[par];
          if (bow_before(b, bj, a, aj) == up) { S.u.sel.lv[pos] = b; S.u.sel.lj[pos] = bj; S.u.sel.lv[par] = a; S.u.sel.lj[par] = aj; }
        }
        __syncthreads();
      }
    for (int t = tid; t < k; t += BT) {
      const bool ok = t < cnt;
      oi[t] = ok ? db_row0 + S.u.sel.lj[t] : -1;
      os[t] = ok ? S.u.sel.lv[t] : NaN;
    }
    return;
  }
  // more than CAP elements below tau: k sweeps, each the smallest (d, j) after the previous one
  double pv = -INF;
  int pj = -1;
  for (int t = 0; t < k; t++) {
    double bv = 0.0;
    int bj = -1;
    for (int j = tid; j < n; j += BT) {
      const double d = dval(j);
      if (d == d && (pj < 0 || bow_before(pv, pj, d, j)) && (bj < 0 || d < bv)) { bv = d; bj = j; }
    }
    block_argmin<BT>(bv, bj, S.rv, S.rj);
    if (tid == 0) { oi[t] = bj < 0 ? -1 : db_row0 + bj; os[t] = bj < 0 ? NaN : bv; }
    if (bj < 0) {
      for (int u = t + 1 + tid; u < k; u += BT) { oi[u] = -1; os[u] = NaN; }
      return;
    }
    pv = bv; pj = bj;
  }
}

}  // namespace

void launch_bow_rows_check(hipStream_t st, const double* rows, int n, int cols, int n_words, int row_name0, int* counts, u64* total, int* bad) {
  if (n <= 0) return;
  hipLaunchKernelGGL(bow_rows_check_kernel, dim3(n), dim3(CBT), 0, st, rows, cols, n_words, row_name0, counts, total, bad);
}

void launch_bow_scatter(hipStream_t st, const double* rows, int n, int cols, int j0, u64* cursor, int* prow, double* pw) {
  if (n <= 0) return;
  hipLaunchKernelGGL(bow_scatter_kernel, dim3(n), dim3(CBT), 0, st, rows, cols, j0, cursor, prow, pw);
}

int bow_scan_tiles(int nw) { return (nw + STILE - 1) / STILE; }

void launch_bow_scan(hipStream_t st, const int* counts, int nw, u64* tsum, u64* off, u64* cursor) {
  const int T = bow_scan_tiles(nw);
  if (T > 0) hipLaunchKernelGGL(bow_scan_sums_kernel, dim3(T), dim3(CBT), 0, st, counts, nw, tsum);
  hipLaunchKernelGGL(bow_scan_tiles_kernel, dim3(1), dim3(CBT), 0, st, tsum, T, off, cursor, nw);
  if (T > 0) hipLaunchKernelGGL(bow_scan_apply_kernel, dim3(T), dim3(CBT), 0, st, counts, nw, tsum, off, cursor);
}

void launch_bow_fold(hipStream_t st, int nw, const u64* moff, const int* mrow, const double* mw, const u64* toff, const int* trow,
                     const double* tw, u64* noff, int* nrow, double* nwt) {
  if (nw <= 0) return;
  hipLaunchKernelGGL(bow_fold_kernel, dim3((nw + CBT / 64 - 1) / (CBT / 64)), dim3(CBT), 0, st, nw, moff, mrow, mw, toff, trow, tw, noff, nrow, nwt);
}

void launch_bow_score(hipStream_t st, int threads, const double* q, int m, int cols, int n_words, int q_row0, const u64* moff, const int* mrow,
                      const double* mw, const u64* toff, const int* trow, const double* tw, int n, int db_row0, int mask_width, int k,
                      double* acc, int32_t* idx, double* score, int* flag) {
  if (m <= 0) return;
  if (threads == 64)
    hipLaunchKernelGGL(bow_score_kernel<64>, dim3(m), dim3(64), 0, st, q, cols, n_words, q_row0, moff, mrow, mw, toff, trow, tw, n, db_row0,
                       mask_width, k, acc, idx, score, flag);
  else
    hipLaunchKernelGGL(bow_score_kernel<256>, dim3(m), dim3(256), 0, st, q, cols, n_words, q_row0, moff, mrow, mw, toff, trow, tw, n, db_row0,
                       mask_width, k, acc, idx, score, flag);
}

}  // namespace pr
