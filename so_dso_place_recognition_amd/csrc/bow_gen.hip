// bow_gen.hip — ORBVocabulary::transform (DBoW2 TemplatedVocabulary.h:1127-1260, BowVector.cpp:30-69, ScoringObject.h:74-90) as looped
// by BoW/test_bow.cpp:127-135 on gfx950.  The vocabulary tree is held in BFS order (bow.cpp): a node's children are contiguous, in file
// order, so one level of one descent reads its siblings' descriptors as one run of 32-byte rows.
//
//   bow_descend   : G lanes per descriptor (G = 1..16).  Per level each lane XORs the descriptor against one child (chunks of G children
//                   for larger families), popcounts the 256 bits (FORB.cpp:81-97) and the group takes the first minimum by a min-reduction
//                   over (distance << 5 | lane): ties go to the first child in file order, as the reference's strict `d < best_d` does.
//                   The descent stops at a node without children (isLeaf() is children.empty(), :326), whatever its file flag says.
//   bow_aggregate : one workgroup per image.  (word << 32 | feature) keys of the descriptors whose weight is > 0 are bitonic-sorted in LDS
//                   (global scratch above BOW_LDS_KEYS descriptors), so every word's run lists its features in input order: the run's
//                   value is the reference's sequence of fp64 additions (addWeight, TF / TF_IDF) or its first weight (addIfNotExist,
//                   IDF / BINARY).  DOT_PRODUCT divides TF / TF_IDF values by the word count; the other scorings normalise by ONE
//                   sequential sum of |v| (L1) or v^2 then sqrt (L2) in ascending word order (BowVector::normalize) - no tree reduction.
// Rows do not depend on an image's position in the batch: each image is one workgroup's, in the same order whatever surrounds it.
// Built with -ffp-contract=off (Makefile): v * v + norm is not fused, divisions are IEEE.
#include "kernels.hpp"

namespace pr {
namespace {

constexpr int BT = 256;                          // threads per workgroup (both kernels)
constexpr unsigned long long NOKEY = ~0ull;      // stopped descriptor / sort padding: sorts behind every real key

template <int G>
__global__ __launch_bounds__(BT) void bow_descend_kernel(const uint8_t* __restrict__ desc, int64_t n_desc, const uint4* __restrict__ vdesc,
                                                         const int2* __restrict__ child, const int* __restrict__ word,
                                                         int* __restrict__ node_out, int* __restrict__ feat_words) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t step = (int64_t)gridDim.x * (BT / G);
  for (int64_t f = (int64_t)blockIdx.x * (BT / G) + threadIdx.x / G; f < n_desc; f += step) {
    const uint4* fp = reinterpret_cast<const uint4*>(desc + f * 32);
    const uint4 a = fp[0], b = fp[1];
    int nd = 0;
    int2 ch = child[0];
    while (ch.y > 0) {                          // every lane of the group takes the same path (same descriptor, same node)
      int best_d = 0x7fffffff, best_c = 0;
      for (int c0 = 0; c0 < ch.y; c0 += G) {
        const int c = c0 + lane;
        int key = 0x7fffffff;
        if (c < ch.y) {
          const uint4* p = vdesc + 2 * (int64_t)(ch.x + c);
          const uint4 x = p[0], y = p[1];
          const int d = __popc(a.x ^ x.x) + __popc(a.y ^ x.y) + __popc(a.z ^ x.z) + __popc(a.w ^ x.w) + __popc(b.x ^ y.x) +
                        __popc(b.y ^ y.y) + __popc(b.z ^ y.z) + __popc(b.w ^ y.w);
          key = (d << 5) | lane;
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o, G));
        if ((key >> 5) < best_d) {             // strictly smaller: an earlier chunk keeps a tie
          best_d = key >> 5;
          best_c = c0 + (key & 31);
        }
      }
      nd = ch.x + best_c;
      ch = child[nd];
    }
    if (lane == 0) {
      node_out[f] = nd;
      if (feat_words) feat_words[f] = word[nd];
    }
  }
}

__device__ __forceinline__ unsigned kword(unsigned long long k) { return (unsigned)(k >> 32); }
__device__ __forceinline__ int kfeat(unsigned long long k) { return (int)(k & 0xffffffffu); }

// One image: n descriptors from lo, keys = LDS (GLOBAL false, n <= BOW_LDS_KEYS) or this image's 2n-entry region of the global scratch.
template <bool GLOBAL>
__device__ __forceinline__ void bow_image(unsigned long long* keys, int n, int64_t lo, const int* __restrict__ node, const int* __restrict__ word,
                                          const double* __restrict__ weight, int weighting, int scoring, int cols, double* wgt, double* vals,
                                          double* out_ids, double* out_vals, int* scan, int* s_m, double* s_norm, int& D) {
  const int t = threadIdx.x;
  int P = 1;
  while (P < n) P <<= 1;
  for (int j = t; j < P; j += BT) {
    unsigned long long key = NOKEY;
    if (j < n) {
      const int nd = node[lo + j];
      const double w = weight[nd];
      wgt[lo + j] = w;
      if (w > 0) key = ((unsigned long long)(unsigned)word[nd] << 32) | (unsigned)j;   // `if(w > 0) // not stopped` (:1153, :1177)
    }
    keys[j] = key;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int q = t; q < P / 2; q += BT) {
        const int i = ((q & ~(jj - 1)) << 1) | (q & (jj - 1));
        const unsigned long long x = keys[i], y = keys[i + jj];
        if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[i + jj] = x; }
      }
      __syncthreads();
    }
  for (int j = t; j < P; j += BT)               // the number of real keys (0 when the first one is padding; *s_m was zeroed at entry)
    if (keys[j] != NOKEY && (j + 1 == P || keys[j + 1] == NOKEY)) *s_m = j + 1;
  __syncthreads();
  const int M = *s_m;
  const int C = (M + BT - 1) / BT, j0 = min(t * C, M), j1 = min(j0 + C, M);
  int cnt = 0;
  for (int j = j0; j < j1; j++) cnt += (j == 0 || kword(keys[j]) != kword(keys[j - 1]));
  scan[t] = cnt;
  __syncthreads();
  for (int o = 1; o < BT; o <<= 1) {            // inclusive scan of the run starts per thread
    const int v = t >= o ? scan[t - o] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  D = scan[BT - 1];
  int rank = scan[t] - cnt;
  const bool tf = weighting == 0 || weighting == 1;   // TF_IDF, TF: addWeight; IDF, BINARY: addIfNotExist
  for (int j = j0; j < j1; j++) {
    const unsigned wd = kword(keys[j]);
    if (j > 0 && wd == kword(keys[j - 1])) continue;
    double s = wgt[lo + kfeat(keys[j])];
    if (tf)
      for (int q = j + 1; q < M && kword(keys[q]) == wd; q++) s += wgt[lo + kfeat(keys[q])];
    vals[lo + rank] = s;
    if (rank < cols) out_ids[rank] = (double)wd;
    rank++;
  }
  __syncthreads();
  double* v = vals + lo;
  if (!GLOBAL) {                                // the keys are dead: the values go to LDS for the sequential norm
    v = reinterpret_cast<double*>(keys);
    for (int r = t; r < D; r += BT) v[r] = vals[lo + r];
    __syncthreads();
  }
  const bool must = scoring != 5;               // every scoring but DOT_PRODUCT normalises (ScoringObject.h:74-90)
  if (!must && tf && D > 0) {
    const double nd = (double)D;
    for (int r = t; r < D; r += BT) v[r] /= nd;
  }
  if (must) {
    if (t == 0) {
      double norm = 0.0;
      if (scoring == 1) {
        for (int r = 0; r < D; r++) norm += v[r] * v[r];
        norm = sqrt(norm);
      } else {
        for (int r = 0; r < D; r++) norm += fabs(v[r]);
      }
      *s_norm = norm;
    }
    __syncthreads();
    const double norm = *s_norm;
    if (norm > 0.0)
      for (int r = t; r < D; r += BT) v[r] /= norm;
  }
  for (int r = t; r < cols; r += BT) {
    if (r < D) {
      out_vals[r] = v[r];
    } else {
      out_ids[r] = -1.0;
      out_vals[r] = -1.0;
    }
  }
}

__global__ __launch_bounds__(BT) void bow_aggregate_kernel(const int64_t* __restrict__ offs, int64_t n_desc, const int* __restrict__ node,
                                                           const int* __restrict__ word, const double* __restrict__ weight, int weighting,
                                                           int scoring, int cols, double* wgt, double* vals, unsigned long long* gkeys,
                                                           double* __restrict__ out, int* __restrict__ n_words, int* __restrict__ flags) {
  __shared__ unsigned long long lkeys[BOW_LDS_KEYS];
  __shared__ int scan[BT];
  __shared__ int s_m;
  __shared__ double s_norm;
  const int i = blockIdx.x;
  int64_t lo = offs[i], hi = offs[i + 1];
  lo = lo < 0 ? 0 : lo > n_desc ? n_desc : lo;
  hi = hi < lo ? lo : hi > n_desc ? n_desc : hi;
  const int n = node ? (int)(hi - lo) : 0;      // no words in the vocabulary: an empty vector (:1135-1138)
  if (threadIdx.x == 0) s_m = 0;
  __syncthreads();
  double* ids = out + (size_t)2 * i * cols;
  double* vs = ids + cols;
  int D = 0;
  if (n <= BOW_LDS_KEYS)
    bow_image<false>(lkeys, n, lo, node, word, weight, weighting, scoring, cols, wgt, vals, ids, vs, scan, &s_m, &s_norm, D);
  else
    bow_image<true>(gkeys + 2 * lo, n, lo, node, word, weight, weighting, scoring, cols, wgt, vals, ids, vs, scan, &s_m, &s_norm, D);
  if (threadIdx.x == 0) {
    if (n_words) n_words[i] = D;
    if (D > cols) *flags = 1;
  }
}

__global__ void bow_fill_words_kernel(int* p, int64_t n, int v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

template <int G>
void descend(hipStream_t st, const uint8_t* desc, int64_t n_desc, const uint4* vdesc, const int2* child, const int* word, int* node,
             int* feat_words) {
  const int64_t blocks = (n_desc + BT / G - 1) / (BT / G);
  hipLaunchKernelGGL(bow_descend_kernel<G>, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(BT), 0, st, desc, n_desc, vdesc, child,
                     word, node, feat_words);
}

}  // namespace

void launch_bow_descend(hipStream_t st, const uint8_t* desc, int64_t n_desc, const uint4* vdesc, const int2* child, const int* word,
                        int lanes, int* node, int* feat_words) {
  if (n_desc <= 0) return;
  switch (lanes) {
    case 1: descend<1>(st, desc, n_desc, vdesc, child, word, node, feat_words); break;
    case 2: descend<2>(st, desc, n_desc, vdesc, child, word, node, feat_words); break;
    case 4: descend<4>(st, desc, n_desc, vdesc, child, word, node, feat_words); break;
    case 8: descend<8>(st, desc, n_desc, vdesc, child, word, node, feat_words); break;
    default: descend<16>(st, desc, n_desc, vdesc, child, word, node, feat_words); break;
  }
}

void launch_bow_aggregate(hipStream_t st, const int64_t* offs, int N, int64_t n_desc, const int* node, const int* word, const double* weight,
                          int weighting, int scoring, int cols, double* wgt, double* vals, unsigned long long* gkeys, double* out,
                          int* n_words, int* flags) {
  if (N <= 0) return;
  hipLaunchKernelGGL(bow_aggregate_kernel, dim3(N), dim3(BT), 0, st, offs, n_desc, node, word, weight, weighting, scoring, cols, wgt, vals,
                     gkeys, out, n_words, flags);
}

void launch_bow_fill_words(hipStream_t st, int* feat_words, int64_t n, int v) {
  if (n <= 0) return;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(bow_fill_words_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, feat_words, n, v);
}

}  // namespace pr
