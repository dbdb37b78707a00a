// seqmatch.hip — sequence matching on gfx950: trajectory-summed scores over the two fp32 distance matrices and their top-k per query row
// (the rule: include/place_recognition.h, "sequence matching"; restated in tests/seqmatch_np.py).
//
// A true revisit is a LINE in the distance matrix (query i - l matches DB row j - steps[v][l]), an alias an isolated cell.  For every cell
// the fused scores f are summed along V short trajectories of up to L lags, the best mean is the cell's score S, and the k smallest
// (S, j) of a row are its candidates.
//
//   seq_select_kernel   a workgroup owns SEQ_R query rows and walks a run of slabs of SEQ_W columns.  Per slab it forms f ONCE for
//                       SEQ_R + L - 1 rows by SEQ_W + 2 SEQ_REACH columns and keeps it in LDS as fp64 - a cell that cannot be a term
//                       (outside the matrix, masked) is stored as NaN, so "a dropped velocity" is "a NaN sum" and the inner loop is one
//                       LDS read and one add per term.  A wave owns two of the rows: each lane sums four cells of a row per velocity,
//                       and the row's k best stay in the wave's REGISTERS (lane t holds entry t, ascending by (S, j)); a cell that beats
//                       the k-th is inserted by lane shifts.  No atomics, no barrier besides the two around the tile.
//   seq_merge_kernel    few row tiles: the slabs of a tile are cut into P runs (seq_parts: a function of (m, n) only); one wave per row
//                       merges the P lists by the same insertion.
// Every distance is fetched from HBM (SEQ_R + L - 1) / SEQ_R x (SEQ_W + 2 SEQ_REACH) / SEQ_W times instead of L V times.
#include <cmath>

#include "div_rn.hpp"
#include "seqmatch.hpp"

namespace pr {
namespace {

constexpr int TC = SEQ_W + 2 * SEQ_REACH;       // columns of the LDS tile
constexpr int NCH = SEQ_W / 64;                 // cells of a row that a lane owns in a slab

__device__ __forceinline__ bool seq_less(double av, int aj, double bv, int bj) { return av < bv || (av == bv && aj < bj); }

// the k best (S, j, v) of a row, held by a wave: lane t < cnt holds the t-th; (ths, thj) is the k-th once the list is full
struct WaveTop {
  double s; int j; int v;
  int cnt; double ths; int thj;
};

__device__ __forceinline__ void top_init(WaveTop& T) { T.s = 0.0; T.j = -1; T.v = -1; T.cnt = 0; T.ths = 0.0; T.thj = -1; }

// every lane offers one (s, j, v) (cand: it is a candidate; the j of a row are distinct).  All 64 lanes call this together.
__device__ __forceinline__ void top_offer(WaveTop& T, int k, bool cand, double s, int j, int v, int lane) {
  bool want = cand && (T.cnt < k || seq_less(s, j, T.ths, T.thj));
  unsigned long long mk = __ballot(want);
  while (mk) {
    const int src = __ffsll((long long)mk) - 1;
    const double ns = __shfl(s, src, 64);
    const int nj = __shfl(j, src, 64), nv = __shfl(v, src, 64);
    const bool front = lane < T.cnt && !seq_less(ns, nj, T.s, T.j);        // entries that stay in front of the new one: a prefix
    const int pos = __popcll(__ballot(front));
    const double us = __shfl_up(T.s, 1, 64);
    const int uj = __shfl_up(T.j, 1, 64), uv = __shfl_up(T.v, 1, 64);
    if (lane > pos) { T.s = us; T.j = uj; T.v = uv; }
    else if (lane == pos) { T.s = ns; T.j = nj; T.v = nv; }
    if (T.cnt < k) T.cnt++;
    if (T.cnt == k) { T.ths = __shfl(T.s, k - 1, 64); T.thj = __shfl(T.j, k - 1, 64); }
    want = want && lane != src && (T.cnt < k || seq_less(s, j, T.ths, T.thj));
    mk = __ballot(want);
  }
}

// (d - mean) / sd as the IEEE quotient: Markstein's sequence from the row's reciprocal where div_rn.hpp is correctly rounded (a row
// whose sd is an ordinary number - `fast` -, a finite x whose quotient can neither overflow nor underflow), the division itself elsewhere
__device__ __forceinline__ double seq_div(double x, double s, double r, bool fast) {
  const double ax = fabs(x);
  if (fast && ax >= 1e-100 && ax <= 1e100) return div_rn(x, s, r);
  return x / s;
}

__device__ __forceinline__ bool seq_fast_sd(double s) {
  return s > 1e-100 && s < 1e100 && (__double_as_longlong(s) & 0xfffffffffffffll) != 0xfffffffffffffll;
}

__global__ __launch_bounds__(256) void seq_select_kernel(const float* __restrict__ d_p, const float* __restrict__ d_i, int m, int n,
                                                          const double* __restrict__ mom, const int* __restrict__ steps, int V, int L,
                                                          int q_row0, int db_row0, int mask_width, double p_weight, int k, int P,
                                                          int32_t* __restrict__ idx, double* __restrict__ score, int32_t* __restrict__ vel,
                                                          double* __restrict__ d_S) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int TR = SEQ_R + L - 1;
  double* tile = reinterpret_cast<double*>(smem);                 // [TR][TC] f, NaN where the cell cannot be a term
  double* st = tile + (size_t)TR * TC;                            // [TR][6] mean_p, sd_p, 1 / sd_p, mean_i, sd_i, 1 / sd_i
  int* lsteps = reinterpret_cast<int*>(st + (size_t)TR * 6);      // [V][L]
  int* vok = lsteps + SEQ_MAX_V * SEQ_MAX_L;                      // [V] the table's row can be used
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * SEQ_R, p = blockIdx.y;
  const int nslabs = (n + SEQ_W - 1) / SEQ_W;
  const int s_begin = (int)((long long)nslabs * p / P), s_end = (int)((long long)nslabs * (p + 1) / P);
  const bool plain = d_i == nullptr;

  for (int t = tid; t < V * L; t += 256) lsteps[t] = steps[t];
  for (int a = tid; a < TR; a += 256) {
    const int ga = r0 - (L - 1) + a;
    double mp = 0.0, sp = 1.0, mi = 0.0, si = 1.0;
    if (!plain && ga >= 0 && ga < m) {
      const double* o = mom + (size_t)ga * 6;
      mp = o[1]; sp = sqrt(o[2] / (o[0] - 1.0));
      mi = o[4]; si = sqrt(o[5] / (o[3] - 1.0));
    }
    double* w = st + a * 6;
    w[0] = mp; w[1] = sp; w[2] = 1.0 / sp; w[3] = mi; w[4] = si; w[5] = 1.0 / si;
  }
  __syncthreads();
  if (tid < V) {      // a row of a DEVICE table that breaks the rule (first step not 0, a step beyond the halo) is a dropped velocity
    bool ok = lsteps[tid * L] == 0;
    for (int l = 0; l < L; l++) ok = ok && lsteps[tid * L + l] <= SEQ_REACH && lsteps[tid * L + l] >= -SEQ_REACH;
    vok[tid] = ok ? 1 : 0;
  }

  WaveTop T[2];
  top_init(T[0]); top_init(T[1]);
  const double nan = __builtin_nan("");
  for (int slab = s_begin; slab < s_end; slab++) {
    const int c0 = slab * SEQ_W;
    __syncthreads();                                              // the sums of the slab before are done (first slab: st, vok are written)
    // Two tile rows are 3 x 256 cells: slot s of a row pair is one cell per thread.  The loads of two row pairs (6 cells, 12 loads of a
    // thread) are requested before the first of them is used.  A cell that is no term is read at offset 0 and discarded, so no load
    // hangs on a branch.  (Four row pairs at a time spilled scalar registers.)
    auto cell_of = [&](int a2, int s, int& a, int& cc) {
      if (s == 0) { a = a2; cc = tid; }
      else if (s == 2) { a = a2 + 1; cc = tid + 128; }
      else if (tid < 128) { a = a2; cc = tid + 256; }
      else { a = a2 + 1; cc = tid - 128; }
    };
    for (int a4 = 0; a4 < TR; a4 += 4) {
      float vp[6], vi[6];
      bool ok[6];
#pragma unroll
      for (int u = 0; u < 6; u++) {
        int a, cc;
        cell_of(a4 + 2 * (u / 3), u % 3, a, cc);
        const int ga = r0 - (L - 1) + a, c = c0 - SEQ_REACH + cc;
        bool o = a < TR && ga >= 0 && ga < m && c >= 0 && c < n;
        long long dij = ((long long)q_row0 + ga) - ((long long)db_row0 + c);
        if (dij < 0) dij = -dij;
        o = o && !(dij < (long long)mask_width);
        const size_t off = o ? (size_t)ga * n + c : 0;
        ok[u] = o;
        vp[u] = d_p[off];
        vi[u] = plain ? 0.f : d_i[off];
      }
#pragma unroll
      for (int u = 0; u < 6; u++) {
        int a, cc;
        cell_of(a4 + 2 * (u / 3), u % 3, a, cc);
        if (a >= TR) continue;
        double f = nan;
        if (ok[u]) {
          if (plain) {
            f = (double)vp[u];
          } else {
            const double* w = st + a * 6;
            const double mp = w[0], sp = w[1], rsp = w[2], mi = w[3], si = w[4], rsi = w[5];
            const bool fast = seq_fast_sd(sp) && seq_fast_sd(si);
            f = p_weight * seq_div((double)vp[u] - mp, sp, rsp, fast) + seq_div((double)vi[u] - mi, si, rsi, fast);
          }
        }
        tile[a * TC + cc] = f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int ri = wave + 4 * h, i = r0 + ri;
      if (i >= m) continue;                                       // (whole wave)
      const int Li = L < i + 1 ? L : i + 1;
      const double dLi = (double)Li;
      double bs[NCH], bq[NCH];
      int bv[NCH];
#pragma unroll
      for (int c = 0; c < NCH; c++) { bs[c] = 0.0; bq[c] = 0.0; bv[c] = -1; }
      const double* base = tile + (L - 1 + ri) * TC + SEQ_REACH + lane;
      for (int v = 0; v < V; v++) {
        if (!vok[v]) continue;
        double s[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) s[c] = 0.0;
        const int* sv = lsteps + v * L;
        // eight lags at a time: their steps, then their 32 cells, are requested together (one lag per turn left the wave waiting for
        // two dependent LDS reads per term); the additions stay in ascending l
        int l = 0;
        for (; l + 8 <= Li; l += 8) {
          int sl[8];
#pragma unroll
          for (int u = 0; u < 8; u++) sl[u] = sv[l + u];
          double t[8][NCH];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const double* rp = base - (l + u) * TC - sl[u];
#pragma unroll
            for (int c = 0; c < NCH; c++) t[u][c] = rp[64 * c];
          }
#pragma unroll
          for (int u = 0; u < 8; u++)
#pragma unroll
            for (int c = 0; c < NCH; c++) s[c] += t[u][c];
        }
        for (; l < Li; l++) {
          const double* rp = base - l * TC - sv[l];
#pragma unroll
          for (int c = 0; c < NCH; c++) s[c] += rp[64 * c];
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) {
          // a smaller sum is a smaller or equal mean (the division is monotone): only then is the mean formed and compared, strictly
          if (s[c] == s[c] && (bv[c] < 0 || s[c] < bs[c])) {
            const double q = s[c] / dLi;
            if (bv[c] < 0 || q < bq[c]) { bq[c] = q; bv[c] = v; }
            bs[c] = s[c];
          }
        }
      }
#pragma unroll
      for (int c = 0; c < NCH; c++) {
        const int j = c0 + 64 * c + lane;
        const bool valid = j < n, cand = valid && bv[c] >= 0;
        if (d_S && valid) d_S[(size_t)i * n + j] = cand ? bq[c] : __builtin_inf();
        top_offer(T[h], k, cand, bq[c], j, bv[c], lane);
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int i = r0 + wave + 4 * h;
    if (i >= m || lane >= k) continue;
    const bool has = lane < T[h].cnt;
    const size_t o = ((size_t)(P > 1 ? p : 0) * m + i) * k + lane;
    idx[o] = has ? (P > 1 ? T[h].j : db_row0 + T[h].j) : -1;
    score[o] = has ? T[h].s : nan;
    vel[o] = has ? T[h].v : -1;
  }
}

// lists [P][m][k] of (S, local j, v), -1 where a list ran out -> the k best of every row by (S, j); one wave per row
__global__ __launch_bounds__(256) void seq_merge_kernel(const int32_t* __restrict__ lidx, const double* __restrict__ lscore,
                                                         const int32_t* __restrict__ lvel, int P, int m, int k, int db_row0,
                                                         int32_t* __restrict__ idx, double* __restrict__ score, int32_t* __restrict__ vel) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= m) return;                                             // (whole wave)
  WaveTop T;
  top_init(T);
  const int E = P * k;
  for (int e0 = 0; e0 < E; e0 += 64) {
    const int e = e0 + lane;
    double s = 0.0;
    int j = -1, v = -1;
    if (e < E) {
      const size_t o = ((size_t)(e / k) * m + q) * k + (e % k);
      j = lidx[o]; s = lscore[o]; v = lvel[o];
    }
    top_offer(T, k, j >= 0, s, j, v, lane);
  }
  if (lane < k) {
    const bool has = lane < T.cnt;
    const size_t o = (size_t)q * k + lane;
    idx[o] = has ? db_row0 + T.j : -1;
    score[o] = has ? T.s : __builtin_nan("");
    vel[o] = has ? T.v : -1;
  }
}

// ------------------------------------------------------------------------------------------------------------------ the online form
// One keyframe per push, three launches whose grids depend on the create sizes only:
//   seq_push_stats_kernel    one workgroup: the switch, the clamped count and the push counter into ctl; per channel (mean, sd) of the row
//                            over its non-NaN entries j < n in the header's one order (256 partial sums, then the tree)
//   seq_push_score_kernel    256 columns a workgroup: F_n[j] into the ring's slot, S(n, j) over the earlier pushed rows, and the
//                            workgroup's cells sorted by (S, j) (bitonic network in LDS): its min(k, 256) best into the lists
//   seq_push_select_kernel   one workgroup: the k best of the lists by (S, j) in k arg-min rounds, the outputs, and - by ONE thread -
//                            the slot's row id and the counter
constexpr int SEQ_NONE_J = 0x7fffffff;

__device__ __forceinline__ double tree256(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void seq_push_stats_kernel(SeqView v, const double* __restrict__ rows, const int* __restrict__ count,
                                                              const int* __restrict__ emitted, int normalize) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const bool on = !(emitted && emitted[0] == 0);
  int n = count[0];
  n = n < 0 ? 0 : (n > v.capacity ? v.capacity : n);             // clamped before any address is formed from it
  if (tid == 0) { v.ctl[0] = on ? 1 : 0; v.ctl[1] = n; v.ctl[2] = v.count[0]; v.ctl[3] = 0; }
  if (!on || !normalize) return;
  for (int c = 0; c < v.channels; c++) {
    const double* x = rows + (size_t)c * v.capacity;
    double s = 0.0, cn = 0.0;
    for (int j = tid; j < n; j += 256) { const double a = x[j]; if (a == a) { s += a; cn += 1.0; } }
    const double S = tree256(s, red, tid), C = tree256(cn, red, tid);
    const double mean = S / C;
    double m2 = 0.0;
    for (int j = tid; j < n; j += 256) { const double a = x[j]; if (a == a) { const double d = a - mean; m2 += d * d; } }
    const double M2 = tree256(m2, red, tid);
    if (tid == 0) { v.stats[2 * c] = mean; v.stats[2 * c + 1] = sqrt(M2 / (C - 1.0)); }
  }
}

__global__ __launch_bounds__(256) void seq_push_score_kernel(SeqView v, const double* __restrict__ rows, SeqWeights w, int normalize,
                                                              int mask_width, int k) {
  __shared__ double sv[256];
  __shared__ int sj[256], sl_v[256];
  __shared__ int lsteps[SEQ_MAX_V * SEQ_MAX_L];
  const int tid = threadIdx.x;
  const int on = v.ctl[0], n = v.ctl[1], pushes = v.ctl[2];
  if (!on) return;
  const int kk = k < SEQ_PUSH_COLS ? k : SEQ_PUSH_COLS;
  const int base = blockIdx.x * SEQ_PUSH_COLS, j = base + tid;
  double* ls = v.lscore + (size_t)blockIdx.x * v.max_k;
  int* lj = v.lj + (size_t)blockIdx.x * v.max_k;
  int* lv = v.lv + (size_t)blockIdx.x * v.max_k;
  if (base >= n) {                                                // (whole workgroup) nothing of the row here: an empty list
    if (tid < kk) { ls[tid] = __builtin_inf(); lj[tid] = -1; lv[tid] = -1; }
    return;
  }
  const int L = v.L, cap = v.capacity;
  for (int t = tid; t < v.V * L; t += 256) lsteps[t] = v.steps[t];
  __syncthreads();
  const int slot = pushes % L, Ln = L < pushes + 1 ? L : pushes + 1;
  double S = __builtin_inf();
  int bv = -1;
  if (j < n) {
    double F;
    if (normalize) {
      F = 0.0;
      for (int c = 0; c < v.channels; c++) F = F + w.w[c] * ((rows[(size_t)c * cap + j] - v.stats[2 * c]) / v.stats[2 * c + 1]);
    } else {
      F = rows[j];
    }
    v.ring[(size_t)slot * cap + j] = F;
    double bq = 0.0;
    const double dLn = (double)Ln;
    for (int vv = 0; vv < v.V; vv++) {
      double s = 0.0 + F;
      for (int l = 1; l < Ln; l++) {                              // the l-th earlier pushed row: another slot than this push's (l < L)
        const int sl = (pushes - l) % L, nl = v.ids[sl];
        const int c = j - lsteps[vv * L + l];
        double term = __builtin_nan("");
        if (c >= 0 && c < nl && nl - c >= mask_width) term = v.ring[(size_t)sl * cap + c];
        s += term;
      }
      const double q = s / dLn;
      if (q == q && (bv < 0 || q < bq)) { bq = q; bv = vv; }
    }
    if (n - j < mask_width) bv = -1;
    if (bv >= 0) S = bq;
  }
  sv[tid] = S; sj[tid] = bv >= 0 ? j : SEQ_NONE_J; sl_v[tid] = bv;
  __syncthreads();
  for (int size = 2; size <= 256; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < 128) {
        const int pos = 2 * tid - (tid & (stride - 1)), par = pos + stride;
        const bool up = (pos & size) == 0;
        const double a = sv[pos], b = sv[par];
        const int aj = sj[pos], bj = sj[par];
        if (seq_less(b, bj, a, aj) == up) {
          const int av = sl_v[pos], bvv = sl_v[par];
          sv[pos] = b; sj[pos] = bj; sl_v[pos] = bvv; sv[par] = a; sj[par] = aj; sl_v[par] = av;
        }
      }
      __syncthreads();
    }
  if (tid < kk) { const bool has = sj[tid] != SEQ_NONE_J; ls[tid] = sv[tid]; lj[tid] = has ? sj[tid] : -1; lv[tid] = has ? sl_v[tid] : -1; }
}

__global__ __launch_bounds__(1024) void seq_push_select_kernel(SeqView v, int k, int32_t* __restrict__ idx, double* __restrict__ score,
                                                                int32_t* __restrict__ vel, int32_t* __restrict__ info) {
  __shared__ double rv[16];
  __shared__ int rj[16], re[16];
  __shared__ double pick_v;
  __shared__ int pick_j;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int on = v.ctl[0], n = v.ctl[1], pushes = v.ctl[2];
  if (!on) {
    if (tid < k) { idx[tid] = -1; score[tid] = __builtin_nan(""); vel[tid] = -1; }
    if (tid == 0) { info[0] = 0; info[1] = 0; info[2] = pushes; info[3] = 0; }
    return;
  }
  const int kk = k < SEQ_PUSH_COLS ? k : SEQ_PUSH_COLS;
  const int E = ((n + SEQ_PUSH_COLS - 1) / SEQ_PUSH_COLS) * kk;   // the lists of the workgroups that hold a part of the row
  double pv = 0.0;
  int pj = -1;                                                    // the pick of the round before (none yet)
  for (int t = 0; t < k; t++) {
    double bs = 0.0;
    int bj = -1, be = -1;
    for (int e = tid; e < E; e += 1024) {
      const int o = (e / kk) * v.max_k + (e % kk);
      const int j = v.lj[o];
      if (j < 0) continue;
      const double s = v.lscore[o];
      if (pj >= 0 && !seq_less(pv, pj, s, j)) continue;           // picked already
      if (bj < 0 || seq_less(s, j, bs, bj)) { bs = s; bj = j; be = o; }
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
      const double os = __shfl_xor(bs, sft, 64);
      const int oj = __shfl_xor(bj, sft, 64), oe = __shfl_xor(be, sft, 64);
      if (oj >= 0 && (bj < 0 || seq_less(os, oj, bs, bj))) { bs = os; bj = oj; be = oe; }
    }
    if (lane == 0) { rv[wave] = bs; rj[wave] = bj; re[wave] = be; }
    __syncthreads();
    if (tid == 0) {
      for (int u = 1; u < 16; u++)
        if (rj[u] >= 0 && (bj < 0 || seq_less(rv[u], rj[u], bs, bj))) { bs = rv[u]; bj = rj[u]; be = re[u]; }
      idx[t] = bj;                                                // (-1 when the candidates ran out)
      score[t] = bj >= 0 ? bs : __builtin_nan("");
      vel[t] = bj >= 0 ? v.lv[be] : -1;
      pick_v = bs; pick_j = bj;
    }
    __syncthreads();
    pv = pick_v; pj = pick_j;
    if (pj < 0) {                                                 // (uniform) no candidate left: the remaining slots
      for (int u = t + 1 + tid; u < k; u += 1024) { idx[u] = -1; score[u] = __builtin_nan(""); vel[u] = -1; }
      break;
    }
  }
  if (tid == 0) {                                                 // the push is committed by one thread
    const int L = v.L;
    v.ids[pushes % L] = n;
    v.count[0] = pushes + 1;
    info[0] = 1; info[1] = L < pushes + 1 ? L : pushes + 1; info[2] = pushes + 1; info[3] = 0;
  }
}

size_t seq_lds_bytes(int L) {
  const size_t TR = SEQ_R + L - 1;
  return TR * TC * 8 + TR * 6 * 8 + (size_t)(SEQ_MAX_V * SEQ_MAX_L + SEQ_MAX_V) * 4;
}

}  // namespace

void launch_seq_push(hipStream_t st, const SeqView& v, const double* rows, const int* count, const int* emitted, const SeqWeights& w,
                     int normalize, int mask_width, int k, int32_t* idx, double* score, int32_t* vel, int32_t* info) {
  hipLaunchKernelGGL(seq_push_stats_kernel, dim3(1), dim3(256), 0, st, v, rows, count, emitted, normalize);
  hipLaunchKernelGGL(seq_push_score_kernel, dim3(v.blocks), dim3(256), 0, st, v, rows, w, normalize, mask_width, k);
  hipLaunchKernelGGL(seq_push_select_kernel, dim3(1), dim3(1024), 0, st, v, k, idx, score, vel, info);
}

void launch_seq_select(hipStream_t st, const float* d_p, const float* d_i, int m, int n, const double* mom, const int* d_steps, int V, int L,
                       int q_row0, int db_row0, int mask_width, double p_weight, int k, int32_t* idx, double* score, int32_t* vel, double* d_S,
                       void* scratch) {
  if (m <= 0) return;
  // (up to 124 KB of dynamic LDS at L = 32: above the 64 KB a launch gets without asking)
  if (seq_lds_bytes(L) > 60 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(seq_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)seq_lds_bytes(L));
  const int tiles = (m + SEQ_R - 1) / SEQ_R;
  int P = scratch ? seq_parts(m, n) : 1;
  if ((size_t)P * m * k > SEQ_LIST_ENTRIES) P = 1;
  if (P > 1) {
    double* lscore = static_cast<double*>(scratch);
    int32_t* lidx = reinterpret_cast<int32_t*>(lscore + SEQ_LIST_ENTRIES);
    int32_t* lvel = lidx + SEQ_LIST_ENTRIES;
    hipLaunchKernelGGL(seq_select_kernel, dim3(tiles, P), dim3(256), seq_lds_bytes(L), st, d_p, d_i, m, n, mom, d_steps, V, L, q_row0, db_row0,
                       mask_width, p_weight, k, P, lidx, lscore, lvel, d_S);
    hipLaunchKernelGGL(seq_merge_kernel, dim3((m + 3) / 4), dim3(256), 0, st, lidx, lscore, lvel, P, m, k, db_row0, idx, score, vel);
    return;
  }
  hipLaunchKernelGGL(seq_select_kernel, dim3(tiles, 1), dim3(256), seq_lds_bytes(L), st, d_p, d_i, m, n, mom, d_steps, V, L, q_row0, db_row0,
                     mask_width, p_weight, k, 1, idx, score, vel, d_S);
}

}  // namespace pr
