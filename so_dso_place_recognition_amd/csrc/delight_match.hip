// delight_match.hip — the device-resident DELIGHT matcher (processDELIGHT.m:7-37 + run_test.m:47-57), exact in fp64.
//
// The answer: for each of the four octant permutations (query row r against entry row r ^ X, X = 0, 5, 6, 3) ts = tc = 0, then for
// c = 0..255 outer, r = 0..15 inner (A(:) is column-major): sum = a + b; if (sum > 0) { ts += ((2 (a - b)) (a - b)) / sum; tc += 1 };
// ts = ts / tc; best = +Inf, if (best > ts) best = ts.  Masked entries +Inf, the k smallest by (score, index), NaN never selected.
// This file is compiled with -ffp-contract=off.  Two stages:
//   delight_dpack    rows -> fp32 image [sig][16][256] (16 KB), empty-bin masks (512 B) and one "coarse-exact" flag per row: every
//                    element a non-negative integer <= 2^24 (held exactly by the image); other rows get a zero image, count in stat[0]
//   delight_coarse   the arithmetic of delight_match_kernel (delight.hip: packed fp32, one v_rcp_f32 per four divisions, the 2^-30
//                    bias), one wave per query, 4 queries per workgroup, the entry rows through a double-buffered LDS tile; the key
//                    never leaves the wave: mask applied, the C smallest keys of the (query, slab) kept in an LDS list
//                    -> cand [m][S][C], ckey [m][S][C], w [m][S] = the largest listed key (+Inf: the list has room left)
//   delight_rerank   candidates sorted by key; those that can still be among the k best (key <= thr, see the kernel) get their exact
//                    distance; sorted by (score, index) -> the k best; containment: every row outside the lists has
//                    d >= L = (min_s w - ABS) / (1 + REL), so the answer is final iff the k-th score < L
//   delight_xdist    exact rows of the flagged queries; selection and compaction are gist_match.hip's (launch_gist_xselect / _compact)
// Exact distances (rerank and exact rows alike): exact_batch of delight_exact.hpp, a batch of 16 pairs per workgroup.
#include <climits>

#include "delight_exact.hpp"
#include "kernels.hpp"
#include "resident_common.hpp"

namespace pr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// |key - d| <= DM_REL d + DM_ABS for a pair of coarse-exact rows (tests/test_delight_match_cpu.py restates it)
constexpr double DM_REL = 4200.0 * 0x1p-24;
constexpr double DM_ABS = 0x1.01p-17;

// one wave per signature, lane l owns columns 4 l .. 4 l + 3 of the 16 rows (the lane layout of the matcher)
__global__ __launch_bounds__(64) void delight_dpack_kernel(const double* __restrict__ rows, int row0, float* __restrict__ img,
                                                            unsigned* __restrict__ mask, int* __restrict__ okflag,
                                                            unsigned* __restrict__ stat /* null | [0] += rows that are not coarse-exact */) {
  const int lane = threadIdx.x;
  const size_t sig = (size_t)row0 + blockIdx.x;
  const double* src = rows + (size_t)blockIdx.x * 4096 + 4 * lane;
  f32x4 v[16];
  int ok = 1;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const f64x2 x0 = *reinterpret_cast<const f64x2*>(src + r * 256), x1 = *reinterpret_cast<const f64x2*>(src + r * 256 + 2);
    const double x[4] = {x0[0], x0[1], x1[0], x1[1]};
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (!(x[c] >= 0.0 && x[c] <= 0x1p24 && x[c] == __builtin_floor(x[c]))) ok = 0;      // NaN fails the first comparison
      v[r][c] = (float)x[c];
    }
  }
  ok = __all(ok);
  unsigned w[2] = {0u, 0u};
  f32x4* dst = reinterpret_cast<f32x4*>(img) + sig * 1024 + lane;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    if (!ok) v[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; c++) w[r >> 3] |= (v[r][c] == 0.f ? 1u : 0u) << (4 * (r & 7) + c);
    dst[r * 64] = v[r];
  }
  mask[sig * 128 + 2 * lane] = w[0];
  mask[sig * 128 + 2 * lane + 1] = w[1];
  if (lane == 0) {
    okflag[sig] = ok;
    if (stat && !ok) atomicAdd(stat, 1u);
  }
}

// delight.hip: nibble r of the result = nibble r ^ X of v
template <int X>
__device__ __forceinline__ unsigned nibble_xor(unsigned v) {
  if (X & 1) v = ((v & 0x0f0f0f0fu) << 4) | ((v >> 4) & 0x0f0f0f0fu);
  if (X & 2) v = ((v & 0x00ff00ffu) << 8) | ((v >> 8) & 0x00ff00ffu);
  if (X & 4) v = (v << 16) | (v >> 16);
  return v;
}

// delight.hip chi2_perm4, unchanged: A holds a + 2^-30; the four divisions of a term share one v_rcp_f32
__device__ __forceinline__ void chi2_perm4(const f32x4 (&A)[16], const f32x4 (&B)[16], f32x2 (&acc)[4]) {
#pragma unroll
  for (int r = 0; r < 16; r++) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const f32x2 a = {A[r][2 * h], A[r][2 * h + 1]};
      const f32x2 b0 = {B[r][2 * h], B[r][2 * h + 1]}, b1 = {B[r ^ 5][2 * h], B[r ^ 5][2 * h + 1]};
      const f32x2 b2 = {B[r ^ 6][2 * h], B[r ^ 6][2 * h + 1]}, b3 = {B[r ^ 3][2 * h], B[r ^ 3][2 * h + 1]};
      const f32x2 s0 = a + b0, s1 = a + b1, s2 = a + b2, s3 = a + b3;
      const f32x2 d0 = a - b0, d1 = a - b1, d2 = a - b2, d3 = a - b3;
      const f32x2 p01 = s0 * s1, p23 = s2 * s3, P = p01 * p23;
      const f32x2 R = {__builtin_amdgcn_rcpf(P[0]), __builtin_amdgcn_rcpf(P[1])};
      const f32x2 q23 = R * p23, q01 = R * p01;
      acc[0] = __builtin_elementwise_fma(d0 * d0, q23 * s1, acc[0]);
      acc[1] = __builtin_elementwise_fma(d1 * d1, q23 * s0, acc[1]);
      acc[2] = __builtin_elementwise_fma(d2 * d2, q01 * s3, acc[2]);
      acc[3] = __builtin_elementwise_fma(d3 * d3, q01 * s2, acc[3]);
    }
  }
}

constexpr int DM_MAXC = 136;      // k + 8 at k = 128

// Workgroup = 4 queries (one per wave) x slab `s` of the entries, as delight_match_kernel; the list of a (query, slab) lives in LDS,
// its largest key T and that key's position in registers (wave-uniform: after the butterfly every lane holds the same key).
__global__ __launch_bounds__(256, 2) void delight_coarse_kernel(const float* __restrict__ q, const float* __restrict__ db,
                                                                 const unsigned* __restrict__ dbmask, int m, int n, int S, int C,
                                                                 long long q_row0, long long db_row0, int mask_width,
                                                                 int* __restrict__ cand, float* __restrict__ ckey, float* __restrict__ wout) {
  __shared__ f32x4 rowbuf[2][1024];
  __shared__ float lk[4][DM_MAXC];
  __shared__ int li[4][DM_MAXC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = (blockIdx.x / S) * 4 + w, s = blockIdx.x % S;
  const int j0 = (int)((long long)n * s / S), j1 = (int)((long long)n * (s + 1) / S);
  const bool valid = i < m;
  for (int e = lane; e < C; e += 64) { lk[w][e] = __builtin_inff(); li[w][e] = -1; }
  f32x4 A[16];
  unsigned za0 = 0u, za1 = 0u;
  {
    const f32x4* pa = reinterpret_cast<const f32x4*>(q + (size_t)(valid ? i : 0) * 4096) + lane;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      A[r] = pa[r * 64];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        (r < 8 ? za0 : za1) |= (A[r][c] == 0.f ? 1u : 0u) << (4 * (r & 7) + c);
        A[r][c] += 0x1p-30f;
      }
    }
  }
  const long long gq = q_row0 + i;
  float T = __builtin_inff();
  int tpos = 0;
  f32x4 st[4];
  if (j0 < j1) {
    const f32x4* src = reinterpret_cast<const f32x4*>(db + (size_t)j0 * 4096) + tid;
#pragma unroll
    for (int k = 0; k < 4; k++) rowbuf[0][tid + 256 * k] = src[256 * k];
  }
  __syncthreads();
  for (int j = j0; j < j1; j++) {
    const int cur = (j - j0) & 1;
    if (j + 1 < j1) {
      const f32x4* src = reinterpret_cast<const f32x4*>(db + (size_t)(j + 1) * 4096) + tid;
#pragma unroll
      for (int k = 0; k < 4; k++) st[k] = src[256 * k];
    }
    const unsigned zb0 = dbmask[(size_t)j * 128 + 2 * lane], zb1 = dbmask[(size_t)j * 128 + 2 * lane + 1];
    f32x4 B[16];
#pragma unroll
    for (int r = 0; r < 16; r++) B[r] = rowbuf[cur][r * 64 + lane];
    f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    chi2_perm4(A, B, acc);
    float ts[4];
    unsigned e01 = (unsigned)(__builtin_popcount(za0 & zb0) + __builtin_popcount(za1 & zb1)) |
                   (unsigned)(__builtin_popcount(za0 & nibble_xor<5>(zb0)) + __builtin_popcount(za1 & nibble_xor<5>(zb1))) << 16;
    unsigned e23 = (unsigned)(__builtin_popcount(za0 & nibble_xor<6>(zb0)) + __builtin_popcount(za1 & nibble_xor<6>(zb1))) |
                   (unsigned)(__builtin_popcount(za0 & nibble_xor<3>(zb0)) + __builtin_popcount(za1 & nibble_xor<3>(zb1))) << 16;
#pragma unroll
    for (int k = 0; k < 4; k++) ts[k] = acc[k][0] + acc[k][1];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
      for (int k = 0; k < 4; k++) ts[k] += __shfl_xor(ts[k], d);
      e01 += (unsigned)__shfl_xor((int)e01, d);
      e23 += (unsigned)__shfl_xor((int)e23, d);
    }
    const float tc[4] = {4096.f - (float)(e01 & 0xffffu), 4096.f - (float)(e01 >> 16), 4096.f - (float)(e23 & 0xffffu),
                         4096.f - (float)(e23 >> 16)};
    float best = __builtin_inff();
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float v = 2.f * ts[k] / tc[k];
      if (best > v) best = v;
    }
    long long dlt = gq - (db_row0 + j);
    dlt = dlt < 0 ? -dlt : dlt;
    // wave-uniform; +Inf and NaN keys fail best < T.  The entry written here is read by other lanes only after the barrier below.
    if (valid && !(dlt < (long long)mask_width) && best < T) {
      if (lane == 0) { lk[w][tpos] = best; li[w][tpos] = j; }
      float mv = -__builtin_inff();
      int mp = 0;
      for (int e = lane; e < C; e += 64) {
        const float x = e == tpos ? best : lk[w][e];
        if (x > mv) { mv = x; mp = e; }
      }
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(mv, d);
        const int op = __shfl_xor(mp, d);
        if (ov > mv || (ov == mv && op < mp)) { mv = ov; mp = op; }
      }
      T = mv;
      tpos = mp;
    }
    if (j + 1 < j1) {
#pragma unroll
      for (int k = 0; k < 4; k++) rowbuf[cur ^ 1][tid + 256 * k] = st[k];
    }
    __syncthreads();
  }
  if (valid) {
    const size_t o = ((size_t)i * S + s) * C;
    for (int e = lane; e < C; e += 64) { cand[o + e] = li[w][e]; ckey[o + e] = lk[w][e]; }
    if (lane == 0) wout[(size_t)i * S + s] = T;
  }
}

constexpr int DM_MAX_CAND = 2048;

__global__ __launch_bounds__(256) void delight_rerank_kernel(const double* __restrict__ q, const double* __restrict__ raw, int S, int C,
                                                             const int* __restrict__ cand, const float* __restrict__ ckey,
                                                             const float* __restrict__ wout, const int* __restrict__ qok,
                                                             const unsigned* __restrict__ dstat, int db_row0, int k,
                                                             int32_t* __restrict__ idx, double* __restrict__ score, int* __restrict__ flags) {
  __shared__ XShared sh;
  __shared__ double sk[DM_MAX_CAND];
  __shared__ int si[DM_MAX_CAND];
  __shared__ const double* pa[XB];
  __shared__ const double* pb[XB];
  __shared__ double dd[XB];
  __shared__ int nev;
  const int qi = blockIdx.x, tid = threadIdx.x, total = S * C;
  // a query or a DB row that the image does not hold exactly: no bound, the exact row answers (uniform over the workgroup)
  if (!qok[qi] || dstat[0] != 0u) {
    if (tid == 0) flags[qi] = 1;
    return;
  }
  int N = 256;
  while (N < total) N <<= 1;
  for (int e = tid; e < N; e += 256) {
    const int r = e < total ? cand[(size_t)qi * total + e] : -1;
    sk[e] = r >= 0 ? (double)ckey[(size_t)qi * total + e] : __builtin_inf();
    si[e] = r >= 0 ? r : INT_MAX;
  }
  if (tid == 0) nev = 0;
  sort_pairs(sk, si, N, tid);
  if (si[k - 1] == INT_MAX) {          // fewer than k rows listed
    if (tid == 0) flags[qi] = 1;
    return;
  }
  // The k rows of smallest key have d <= U = key_k / (1 - REL); a listed row with key > thr = U (1 + REL) + ABS has d > U, so it is
  // behind all of those k and cannot tie with them: only the rows up to thr need their exact distance.
  const double thr = sk[k - 1] * ((1.0 + DM_REL) / (1.0 - DM_REL)) * (1.0 + 0x1p-40) + DM_ABS;
  for (int e = tid; e < N; e += 256)
    if (si[e] != INT_MAX && sk[e] <= thr) atomicMax(&nev, e + 1);
  __syncthreads();
  const int E = nev;
  const double* A = q + (size_t)qi * 4096;
  for (int e0 = 0; e0 < E; e0 += XB) {
    const int np = E - e0 < XB ? E - e0 : XB;
    if (tid < XB) { pa[tid] = A; pb[tid] = raw + (size_t)si[e0 + (tid < np ? tid : 0)] * 4096; }
    __syncthreads();
    exact_batch(sh, tid, np, pa, pb, dd);
    if (tid < np) sk[e0 + tid] = dd[tid];
    __syncthreads();
  }
  for (int e = E + tid; e < N; e += 256) { sk[e] = __builtin_inf(); si[e] = INT_MAX; }
  sort_pairs(sk, si, N, tid);
  if (tid < k) {
    idx[(size_t)qi * k + tid] = db_row0 + si[tid];
    score[(size_t)qi * k + tid] = sk[tid];
  }
  if (tid == 0) {
    float w = __builtin_inff();
    for (int s = 0; s < S; s++) w = __builtin_fminf(w, wout[(size_t)qi * S + s]);
    // an unlisted coarse-exact row has key >= w and key <= d (1 + REL) + ABS
    double L = __builtin_inf();
    if (w < __builtin_inff()) {
      L = ((double)w - DM_ABS) / (1.0 + DM_REL) * (1.0 - 0x1p-40);
      if (!(L > 0.0)) L = 0.0;
    }
    flags[qi] = sk[k - 1] < L ? 0 : 1;      // an evaluated row was listed (si != INT_MAX) as E >= k
  }
}

// Exact rows: out[slot * ld + r] = d(query of the slot, DB row r), masked entries +Inf, for the slots [0, count) of this pass;
// slot -> query list[offset + slot] (list null: query offset + slot, count = direct_count).  A workgroup owns 16 DB rows and every 16th slot.
__global__ __launch_bounds__(256) void delight_xdist_kernel(const double* __restrict__ q, const double* __restrict__ raw, int n,
                                                            const int* __restrict__ list, const int* __restrict__ cnt, int offset,
                                                            int direct_count, int cap, double* __restrict__ out, size_t ld, long long q_row0,
                                                            long long db_row0, int mask_width) {
  __shared__ XShared sh;
  __shared__ const double* pa[XB];
  __shared__ const double* pb[XB];
  __shared__ double dd[XB];
  int count = list ? cnt[0] - offset : direct_count;
  if (count > cap) count = cap;
  const int tid = threadIdx.x;
  const int rb = blockIdx.x * XB;
  const int np = n - rb < XB ? n - rb : XB;
  for (int slot = blockIdx.y; slot < count; slot += gridDim.y) {      // uniform over the workgroup; no slot: the block leaves at once
    const int qi = list ? list[offset + slot] : offset + slot;
    if (tid < XB) { pa[tid] = q + (size_t)qi * 4096; pb[tid] = raw + (size_t)(rb + (tid < np ? tid : 0)) * 4096; }
    __syncthreads();
    exact_batch(sh, tid, np, pa, pb, dd);
    if (tid < np) {
      long long dlt = q_row0 + qi - (db_row0 + rb + tid);
      dlt = dlt < 0 ? -dlt : dlt;
      out[(size_t)slot * ld + rb + tid] = dlt < (long long)mask_width ? __builtin_inf() : dd[tid];
    }
    __syncthreads();
  }
}

}  // namespace

void launch_delight_dpack(hipStream_t st, const double* rows, int n, int row0, float* img, unsigned* mask, int* okflag, unsigned* stat) {
  if (n <= 0) return;
  hipLaunchKernelGGL(delight_dpack_kernel, dim3(n), dim3(64), 0, st, rows, row0, img, mask, okflag, stat);
}

void launch_delight_coarse(hipStream_t st, const float* q, int m, const float* db, const unsigned* dbmask, int n, int S, int C, int q_row0,
                           int db_row0, int mask_width, int* cand, float* ckey, float* wout) {
  if (m <= 0 || n <= 0) return;
  hipLaunchKernelGGL(delight_coarse_kernel, dim3((unsigned)((m + 3) / 4) * S), dim3(256), 0, st, q, db, dbmask, m, n, S, C,
                     (long long)q_row0, (long long)db_row0, mask_width, cand, ckey, wout);
}

void launch_delight_rerank(hipStream_t st, const double* q, const double* raw, int m, int S, int C, const int* cand, const float* ckey,
                           const float* wout, const int* qok, const unsigned* dstat, int db_row0, int k, int32_t* idx, double* score,
                           int* flags) {
  if (m <= 0) return;
  hipLaunchKernelGGL(delight_rerank_kernel, dim3(m), dim3(256), 0, st, q, raw, S, C, cand, ckey, wout, qok, dstat, db_row0, k, idx, score,
                     flags);
}

void launch_delight_xdist(hipStream_t st, const double* q, const double* raw, int n, const int* list, const int* cnt, int offset,
                          int direct_count, int cap, double* out, size_t ld, int q_row0, int db_row0, int mask_width) {
  if (n <= 0 || cap <= 0) return;
  hipLaunchKernelGGL(delight_xdist_kernel, dim3((n + XB - 1) / XB, cap < 16 ? cap : 16), dim3(256), 0, st, q, raw, n, list, cnt, offset, direct_count, cap,
                     out, ld, (long long)q_row0, (long long)db_row0, mask_width);
}

}  // namespace pr
