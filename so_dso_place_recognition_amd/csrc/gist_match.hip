// gist_match.hip — the device-resident GIST matcher (processGIST.m:1-10 + run_test.m:47-57), exact in fp64.
//
// The answer is d = ((0 + t_0) + t_1) + ... with t_c = RN(RN(a_c - b_c)^2) in ascending column order (this file is compiled with
// -ffp-contract=off), masked entries +Inf, the k smallest by (score, index), NaN never selected.  Two stages:
//   gist_pack     rows -> f16 image of (row - mu) in the operand layout of v_mfma_f32_32x32x16_f16 ([tile of 32 rows][K-step][lane][8 f16],
//                 f16 subnormals flushed to zero), nd = |a'|^2 (fp32), rs >= |(a - mu) - a'| (fp32, rounded up); NaN rows: nd = NaN and a
//                 zero image (never listed), rows that overflow f16: nd = rs = +Inf (the rerank then flags every query: exact rows)
//   gist_coarse   one wave per (tile of 32 queries, DB slab): key = |a'|^2 + |b'|^2 - 2 a'.b' with the product on the matrix cores, mask
//                 applied, the C smallest keys per query and slab kept in LDS (one private list per lane, the two lanes of a query merged at
//                 the end) -> cand [m][S][C], w [m][S] = the largest listed key (+Inf: the list holds every unmasked non-NaN row of the slab)
//   gist_rerank   the candidates' exact distances, sorted by (score, index) -> the k best; the containment test: every row outside the lists
//                 has d >= L = (sqrt(min_s w - Eacc) - rs_q - max rs_db)^2 (1 - slack), so the answer is final iff the k-th score < L
//   gist_xdist / gist_xselect   the exact rows of the flagged queries (all n distances, mask, k rounds of lexicographic arg-min)
#include <climits>

#include "kernels.hpp"
#include "resident_common.hpp"

namespace pr {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// mu[c] = mean over the first `nr` rows of the finite entries' sum (a non-finite entry counts as 0): any fixed vector is valid, this one is cheap
__global__ __launch_bounds__(256) void gist_mean_kernel(const double* __restrict__ rows, int nr, int cols, double* __restrict__ mu) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0;
  for (int r = 0; r < nr; r++) {
    const double v = rows[(size_t)r * cols + c];
    if (__builtin_isfinite(v)) s += v;
  }
  mu[c] = nr > 0 ? s / (double)nr : 0.0;
}

// one wave per row; row `row0 + blockIdx.x` of the image
__global__ __launch_bounds__(64) void gist_pack_kernel(const double* __restrict__ rows, int cols, int KS, const double* __restrict__ mu, int row0,
                                                       u32x4* __restrict__ img, float* __restrict__ nd, float* __restrict__ rs,
                                                       unsigned* __restrict__ stat /* null | [0] max nd, [1] max rs (float bits) */) {
  const int lane = threadIdx.x, row = row0 + blockIdx.x;
  const double* src = rows + (size_t)blockIdx.x * cols;
  u32x4* tile = img + (size_t)(row >> 5) * KS * 64;
  double nrm = 0.0, res = 0.0;
  int nan = 0, ovf = 0;
  for (int p = lane; p < KS * 2; p += 64) {
    const int k0 = p * 8;
    unsigned short h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int c = k0 + i;
      double v = 0.0;
      if (c < cols) {
        const double x = src[c];
        if (x != x) nan = 1;
        v = x - mu[c];
      }
      _Float16 hv = (_Float16)(float)v;
      if (!__builtin_isfinite(v) || !__builtin_isfinite((float)hv)) { ovf = 1; hv = (_Float16)0.0f; v = 0.0; }
      if (__builtin_fabsf((float)hv) < 0x1p-14f) hv = (_Float16)0.0f;      // no f16 subnormals on the matrix pipe
      const double hd = (double)(float)hv, e = v - hd;
      nrm += hd * hd;
      res += e * e;
      h[i] = __builtin_bit_cast(unsigned short, hv);
    }
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = h[2 * i] | ((unsigned)h[2 * i + 1] << 16);
    tile[(k0 >> 4) * 64 + ((row & 31) | (((k0 >> 3) & 1) << 5))] = o;
  }
  nrm = wave_sum(nrm);
  res = wave_sum(res);
  nan = __any(nan);
  ovf = __any(ovf);
  if (nan || ovf) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int p = lane; p < KS * 2; p += 64) tile[(p >> 1) * 64 + ((row & 31) | ((p & 1) << 5))] = z;
  }
  if (lane == 0) {
    float fn, fr;
    if (nan) { fn = __builtin_nanf(""); fr = 0.f; }
    else if (ovf) { fn = __builtin_inff(); fr = __builtin_inff(); }
    else {
      fn = (float)nrm;
      // |(a - mu) - a'| rounded up: the fp64 evaluation of the residual sum and of a - mu itself (2^-53 relative per entry) are inside the margins
      const double r = __builtin_sqrt(res) * (1.0 + 0x1p-20) + 0x1p-48 * (__builtin_sqrt(nrm) + __builtin_sqrt(res));
      fr = (float)r;
      if (r > 0.0 && fr < __builtin_inff()) fr = fr < 0x1p-120f ? 0x1p-120f : __uint_as_float(__float_as_uint(fr) + 1u);      // one ulp up
    }
    nd[row] = fn;
    rs[row] = fr;
    if (stat && !nan) {
      atomicMax(stat, __float_as_uint(fn));
      atomicMax(stat + 1, __float_as_uint(fr));
    }
  }
}

#define GM_MF(A, B, C) __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), C, 0, 0, 0)

__global__ __launch_bounds__(64) void gist_coarse_kernel(const u32x4* __restrict__ qpk, const float* __restrict__ qn, int m,
                                                         const u32x4* __restrict__ dpk, const float* __restrict__ dn, int n, int KS, int S, int C,
                                                         long long q_row0, long long db_row0, int mask_width, int* __restrict__ cand,
                                                         float* __restrict__ wout) {
  extern __shared__ __attribute__((aligned(16))) u32x4 lds[];
  const int lane = threadIdx.x;
  const int qt = blockIdx.x / S, s = blockIdx.x - qt * S;
  const int DT = (n + 31) >> 5;
  const int t0 = (int)((long long)DT * s / S), t1 = (int)((long long)DT * (s + 1) / S);
  {
    const u32x4* src = qpk + (size_t)qt * KS * 64;
    for (int i = lane; i < KS * 64; i += 64) lds[i] = src[i];
  }
  float* lk = reinterpret_cast<float*>(lds + (size_t)KS * 64);     // [C][64] keys, one private list per lane
  int* li = reinterpret_cast<int*>(lk + (size_t)C * 64);           // [C][64] local rows
  for (int e = 0; e < C; e++) { lk[e * 64 + lane] = __builtin_inff(); li[e * 64 + lane] = -1; }
  __syncthreads();
  const int qi = qt * 32 + (lane & 31);
  const float nq = qi < m ? qn[qi] : __builtin_nanf("");           // a NaN query row lists nothing
  const long long gq = q_row0 + qi;
  float T = __builtin_inff();                                       // the list's largest key, at entry tpos
  int tpos = 0;
#define GM_INSERT(key, r)                                                                  \
  {                                                                                        \
    lk[tpos * 64 + lane] = (key);                                                          \
    li[tpos * 64 + lane] = (r);                                                            \
    T = -__builtin_inff();                                                                 \
    for (int e = 0; e < C; e++) { const float v = lk[e * 64 + lane]; if (v > T) { T = v; tpos = e; } } \
  }
  const u32x4* la = lds + lane;
  for (int t = t0; t < t1; t++) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const u32x4* pb = dpk + (size_t)t * KS * 64 + lane;
    u32x4 b0 = pb[0], b1 = pb[64], b2 = pb[128], b3 = pb[192];
    for (int st = 0; st < KS; st += 4) {
      const u32x4 c0 = b0, c1 = b1, c2 = b2, c3 = b3;
      if (st + 4 < KS) { b0 = pb[(st + 4) * 64]; b1 = pb[(st + 5) * 64]; b2 = pb[(st + 6) * 64]; b3 = pb[(st + 7) * 64]; }
      const u32x4 a0 = la[st * 64], a1 = la[(st + 1) * 64], a2 = la[(st + 2) * 64], a3 = la[(st + 3) * 64];
      acc = GM_MF(c0, a0, acc);      // A = DB tile (rows of the result), B = query tile (its columns)
      acc = GM_MF(c1, a1, acc);
      acc = GM_MF(c2, a2, acc);
      acc = GM_MF(c3, a3, acc);
    }
    // result layout: column = lane & 31 (query), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (DB row of the tile)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int r = t * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      if (r < n) {
        const float key = __builtin_fmaf(-2.f, acc[reg], nq + dn[r]);
        long long dlt = gq - (db_row0 + r);
        dlt = dlt < 0 ? -dlt : dlt;
        if (!(dlt < (long long)mask_width) && key < T) GM_INSERT(key, r)
      }
    }
  }
  __syncthreads();
  if (lane < 32) {
    for (int e = 0; e < C; e++) {
      const float key = lk[e * 64 + lane + 32];
      const int r = li[e * 64 + lane + 32];
      if (key < T) GM_INSERT(key, r)
    }
    if (qi < m) {
      int* co = cand + ((size_t)qi * S + s) * C;
      for (int e = 0; e < C; e++) co[e] = li[e * 64 + lane];
      wout[(size_t)qi * S + s] = T;
    }
  }
#undef GM_INSERT
}

constexpr int GM_MAX_CAND = 2048;

__global__ __launch_bounds__(256) void gist_rerank_kernel(const double* __restrict__ q, const double* __restrict__ raw, int cols, int KP, int S, int C,
                                                          const int* __restrict__ cand, const float* __restrict__ wout,
                                                          const float* __restrict__ qn, const float* __restrict__ qr,
                                                          const unsigned* __restrict__ dstat, int db_row0, int k, int32_t* __restrict__ idx,
                                                          double* __restrict__ score, int* __restrict__ flags) {
  extern __shared__ double qs[];            // [cols]
  __shared__ double sk[GM_MAX_CAND];
  __shared__ int si[GM_MAX_CAND];
  const int qi = blockIdx.x, tid = threadIdx.x, total = S * C;
  int N = 256;
  while (N < total) N <<= 1;
  for (int c = tid; c < cols; c += 256) qs[c] = q[(size_t)qi * cols + c];
  __syncthreads();
  for (int e = tid; e < N; e += 256) {
    const int r = e < total ? cand[(size_t)qi * total + e] : -1;
    double d = __builtin_inf();
    if (r >= 0) {
      const double* b = raw + (size_t)r * cols;
      d = 0.0;
      for (int c = 0; c < cols; c++) { const double t = qs[c] - b[c]; d += t * t; }
    }
    sk[e] = d;
    si[e] = r >= 0 ? r : INT_MAX;
  }
  sort_pairs(sk, si, N, tid);
  if (tid < k) {
    const bool ok = si[tid] != INT_MAX;
    idx[(size_t)qi * k + tid] = ok ? db_row0 + si[tid] : -1;
    score[(size_t)qi * k + tid] = ok ? sk[tid] : __builtin_nan("");
  }
  if (tid == 0) {
    float w = __builtin_inff();
    for (int s = 0; s < S; s++) w = __builtin_fminf(w, wout[(size_t)qi * S + s]);
    double L = __builtin_inf();
    const double nq = (double)qn[qi], ndmax = (double)__uint_as_float(dstat[0]), rbmax = (double)__uint_as_float(dstat[1]);
    // A DB row outside the f16 range has key = +Inf and is never listed, not even by a slab whose list is not full (w = +Inf): with
    // such a row in the database (max nd or max rs not finite) no list is provably complete, whatever w says.
    if (!(ndmax < __builtin_inf()) || !(rbmax < __builtin_inf())) L = 0.0;
    else if (w < __builtin_inff()) {
      // |key - |a' - b'|^2| <= Eacc for every row; | |a - b| - |a' - b'| | <= rs_q + rs_db
      const double eacc = (double)(KP + 8) * 0x1p-23 * (nq + ndmax) * 1.01;
      const double x = (double)w - eacc;
      L = 0.0;
      if (x > 0.0) {
        const double y = __builtin_sqrt(x) * (1.0 - 0x1p-40) - (double)qr[qi] - rbmax;
        if (y > 0.0) L = y * y * (1.0 - (double)(cols + 8) * 0x1p-50);
      }
    }
    const bool full = si[k - 1] != INT_MAX;
    flags[qi] = (full && sk[k - 1] < L) ? 0 : 1;
  }
}

// flags [m] -> ascending list of the flagged queries + their count (cnt[0]; cnt[1] sums a call's chunks for pr_gist_flagged_count)
__global__ __launch_bounds__(64) void gist_compact_kernel(const int* __restrict__ flags, int m, int* __restrict__ list, int* __restrict__ cnt) {
  const int lane = threadIdx.x;
  int base = 0;
  for (int q0 = 0; q0 < m; q0 += 64) {
    const int qi = q0 + lane;
    const bool f = qi < m && flags[qi] != 0;
    const unsigned long long b = __ballot(f);
    if (f) list[base + __popcll(b & ((1ull << lane) - 1ull))] = qi;
    base += __popcll(b);
  }
  if (lane == 0) { cnt[0] = base; cnt[1] += base; }
}

__global__ __launch_bounds__(256) void gist_fill_kernel(int* __restrict__ p, int n, int v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

constexpr int XQ = 16;     // queries per workgroup of the exact-row kernel

// Exact rows: out[(slot) * ld + r] = d(query of the slot, DB row r) for the slots [0, count) of this pass; slot -> query list[offset + slot]
// (list null: query offset + slot, count = direct_count).  A workgroup owns 256 DB rows x 16 slots; rows and queries pass through LDS in
// pieces of 16 columns (coalesced 128-byte reads), every thread adds its row's terms in ascending column order.
__global__ __launch_bounds__(256) void gist_xdist_kernel(const double* __restrict__ q, const double* __restrict__ raw, int cols, int n,
                                                         const int* __restrict__ list, const int* __restrict__ cnt, int offset, int direct_count,
                                                         int cap, double* __restrict__ out, size_t ld, long long q_row0, long long db_row0,
                                                         int mask_width) {
  __shared__ double tile[256][17];
  __shared__ double qs[XQ][17];
  __shared__ int qidx[XQ];
  int count = list ? cnt[0] - offset : direct_count;
  if (count > cap) count = cap;
  const int slot0 = blockIdx.y * XQ, tid = threadIdx.x;
  if (slot0 >= count) return;
  const int nq = count - slot0 < XQ ? count - slot0 : XQ;
  if (tid < XQ) qidx[tid] = tid < nq ? (list ? list[offset + slot0 + tid] : offset + slot0 + tid) : -1;
  const int rb = blockIdx.x * 256, tr = tid >> 4, tc = tid & 15;
  double acc[XQ];
#pragma unroll
  for (int j = 0; j < XQ; j++) acc[j] = 0.0;
  for (int c0 = 0; c0 < cols; c0 += 16) {
    __syncthreads();
    const int cc = c0 + tc;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int rr = rb + i * 16 + tr;
      tile[i * 16 + tr][tc] = (rr < n && cc < cols) ? raw[(size_t)rr * cols + cc] : 0.0;
    }
    {
      const int qq = qidx[tr];
      qs[tr][tc] = (qq >= 0 && cc < cols) ? q[(size_t)qq * cols + cc] : 0.0;
    }
    __syncthreads();
    const int nc = cols - c0 < 16 ? cols - c0 : 16;
    for (int c = 0; c < nc; c++) {
      const double b = tile[tid][c];
#pragma unroll
      for (int j = 0; j < XQ; j++) { const double t = qs[j][c] - b; acc[j] += t * t; }
    }
  }
  const int r = rb + tid;
  if (r < n) {
#pragma unroll
    for (int j = 0; j < XQ; j++)
      if (j < nq) {
        long long dlt = q_row0 + qidx[j] - (db_row0 + r);
        dlt = dlt < 0 ? -dlt : dlt;
        out[(size_t)(slot0 + j) * ld + r] = dlt < (long long)mask_width ? __builtin_inf() : acc[j];
      }
  }
}

// the k smallest (score, index) of a slot's row, NaN skipped: k rounds of "smallest entry above the previous one"
__global__ __launch_bounds__(256) void gist_xselect_kernel(const double* __restrict__ rows, size_t ld, int n, const int* __restrict__ list,
                                                           const int* __restrict__ cnt, int offset, int cap, int db_row0, int k,
                                                           int32_t* __restrict__ idx, double* __restrict__ score) {
  __shared__ double ws[4];
  __shared__ int wi[4];
  int count = cnt[0] - offset;
  if (count > cap) count = cap;
  const int slot = blockIdx.x, tid = threadIdx.x;
  if (slot >= count) return;
  const int qi = list[offset + slot];
  const double* row = rows + (size_t)slot * ld;
  double ps = -__builtin_inf();
  int pi = -1;
  bool first = true;
  for (int j = 0; j < k; j++) {
    double bs = __builtin_inf();
    int bi = INT_MAX;
    for (int r = tid; r < n; r += 256) {
      const double v = row[r];
      if (v == v && (first || v > ps || (v == ps && r > pi)) && (v < bs || (v == bs && r < bi))) { bs = v; bi = r; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (os < bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { ws[tid >> 6] = bs; wi[tid >> 6] = bi; }
    __syncthreads();
    bs = ws[0]; bi = wi[0];
#pragma unroll
    for (int w = 1; w < 4; w++)
      if (ws[w] < bs || (ws[w] == bs && wi[w] < bi)) { bs = ws[w]; bi = wi[w]; }
    const bool found = bi != INT_MAX;
    if (tid == 0) {
      idx[(size_t)qi * k + j] = found ? db_row0 + bi : -1;
      score[(size_t)qi * k + j] = found ? bs : __builtin_nan("");
    }
    if (!found) {
      for (int jj = j + 1 + tid; jj < k; jj += 256) { idx[(size_t)qi * k + jj] = -1; score[(size_t)qi * k + jj] = __builtin_nan(""); }
      break;
    }
    ps = bs; pi = bi; first = false;
  }
}

}  // namespace

void launch_gist_mean(hipStream_t st, const double* rows, int nr, int cols, double* mu) {
  hipLaunchKernelGGL(gist_mean_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, rows, nr, cols, mu);
}

void launch_gist_pack(hipStream_t st, const double* rows, int n, int cols, int KS, const double* mu, int row0, void* img, float* nd, float* rs,
                      unsigned* stat) {
  if (n <= 0) return;
  hipLaunchKernelGGL(gist_pack_kernel, dim3(n), dim3(64), 0, st, rows, cols, KS, mu, row0, static_cast<u32x4*>(img), nd, rs, stat);
}

size_t gist_coarse_lds_bytes(int KS, int C) { return (size_t)KS * 64 * 16 + (size_t)C * 64 * 8; }

void launch_gist_coarse(hipStream_t st, const void* qpk, const float* qn, int m, const void* dpk, const float* dn, int n, int KS, int S, int C,
                        int q_row0, int db_row0, int mask_width, int* cand, float* wout) {
  const size_t lds = gist_coarse_lds_bytes(KS, C);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gist_coarse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(gist_coarse_kernel, dim3(((m + 31) / 32) * S), dim3(64), lds, st, static_cast<const u32x4*>(qpk), qn, m,
                     static_cast<const u32x4*>(dpk), dn, n, KS, S, C, (long long)q_row0, (long long)db_row0, mask_width, cand, wout);
}

void launch_gist_rerank(hipStream_t st, const double* q, const double* raw, int cols, int KP, int m, int S, int C, const int* cand,
                        const float* wout, const float* qn, const float* qr, const unsigned* dstat, int db_row0, int k, int32_t* idx,
                        double* score, int* flags) {
  hipLaunchKernelGGL(gist_rerank_kernel, dim3(m), dim3(256), (size_t)cols * sizeof(double), st, q, raw, cols, KP, S, C, cand, wout, qn, qr,
                     dstat, db_row0, k, idx, score, flags);
}

void launch_gist_compact(hipStream_t st, const int* flags, int m, int* list, int* cnt) {
  hipLaunchKernelGGL(gist_compact_kernel, dim3(1), dim3(64), 0, st, flags, m, list, cnt);
}

void launch_gist_fill(hipStream_t st, int* p, int n, int v) {
  if (n > 0) hipLaunchKernelGGL(gist_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, p, n, v);
}

void launch_gist_xdist(hipStream_t st, const double* q, const double* raw, int cols, int n, const int* list, const int* cnt, int offset,
                       int direct_count, int cap, double* out, size_t ld, int q_row0, int db_row0, int mask_width) {
  if (n <= 0 || cap <= 0) return;
  hipLaunchKernelGGL(gist_xdist_kernel, dim3((n + 255) / 256, (cap + XQ - 1) / XQ), dim3(256), 0, st, q, raw, cols, n, list, cnt, offset,
                     direct_count, cap, out, ld, (long long)q_row0, (long long)db_row0, mask_width);
}

void launch_gist_xselect(hipStream_t st, const double* rows, size_t ld, int n, const int* list, const int* cnt, int offset, int cap, int db_row0,
                         int k, int32_t* idx, double* score) {
  if (cap <= 0) return;
  hipLaunchKernelGGL(gist_xselect_kernel, dim3(cap), dim3(256), 0, st, rows, ld, n, list, cnt, offset, cap, db_row0, k, idx, score);
}

}  // namespace pr
