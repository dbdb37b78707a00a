// gist_gen.hip — GIST descriptor of a 256 x 256 grayscale image (GIST/src/libgist.cpp:914-951, bw_gist_scaletab) on gfx950.
//
//   gist_logpad   : log(x + 1) and the 5-pixel symmetric padding (libgist.cpp:276-290, :32-65) -> A [266 x 266], row stride 272
//   gist_gemm     : the whitening low-pass ifft2(fft2(X) gfc) / (w h) of prefilt (:314-395) as C X C (C: the real symmetric
//                   266 x 266 circulant of the separable Gaussian gfc, built on the host, gist.cpp): two fp32 GEMMs per low-pass,
//                   64 x 64 output tiles, 4 x 4 per thread.  The epilogues fold in the contrast normalisation (:340-395) and the
//                   removal of the padding.
//   gist_fft_*    : 256-point transforms as 16 x 16 (radix-16 twice, each 16-point DFT radix-4 x radix-4 in registers), 16 lines per
//                   workgroup, one LDS transpose between the two radix-16 steps.  Forward: rows then columns -> F [256][256] c64.
//   gist_gabor_*  : per (image, filter) pair (gist_gabor, :685-759): inverse columns of F G_k -> Z (scratch of a group of pairs,
//                   Infinity-Cache resident), then inverse rows fused with |.| / (W H) and the row sums of the x blocks of down_N
//                   (:600-629): the filtered images never reach memory.
//   gist_blocks   : block means from the row sums in a fixed order, res[k N + l] with k the x (column) block; a row with a
//                   non-finite value is written as NaN (bw_gist_scaletab refuses it, :936-945).
// Every image is computed by the same launches in the same order whatever its position in the batch: rows are bit-identical
// whether an image is generated alone or inside a batch.
#include "kernels.hpp"

namespace pr {
namespace {

constexpr int GS = 256;       // image side
constexpr int GP = 266;       // padded side
constexpr int LS = 273;       // float2 per line in the LDS transpose (16 x 17 used; odd stride spreads the banks)

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// 4-point DFT in place, W4 = -i (forward) or +i (inverse)
template <bool INV>
__device__ __forceinline__ void dft4(float2& a0, float2& a1, float2& a2, float2& a3) {
  const float2 s02 = cadd(a0, a2), d02 = csub(a0, a2), s13 = cadd(a1, a3), d13 = csub(a1, a3);
  const float2 jd = INV ? make_float2(-d13.y, d13.x) : make_float2(d13.y, -d13.x);   // W4 (a1 - a3)
  a0 = cadd(s02, s13);
  a1 = cadd(d02, jd);
  a2 = csub(s02, s13);
  a3 = csub(d02, jd);
}

// W16^j = exp(-+ 2 pi i j / 16), j = b c <= 9
__device__ __forceinline__ float2 w16(int j, bool inv) {
  constexpr float C[10] = {1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f, 0.0f,
                           -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f, -1.0f, -0.92387953251128674f};
  constexpr float S[10] = {0.0f, 0.38268343236508977f, 0.70710678118654752f, 0.92387953251128674f, 1.0f,
                           0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f, 0.0f, -0.38268343236508977f};
  return make_float2(C[j], inv ? S[j] : -S[j]);
}

// 16-point DFT of v[0..15] in place: n = 4a + b, k = c + 4d
template <bool INV>
__device__ __forceinline__ void dft16(float2 (&v)[16]) {
#pragma unroll
  for (int b = 0; b < 4; b++) dft4<INV>(v[b], v[4 + b], v[8 + b], v[12 + b]);   // v[4c + b] = U_b[c]
#pragma unroll
  for (int b = 1; b < 4; b++)
#pragma unroll
    for (int c = 1; c < 4; c++) v[4 * c + b] = cmul(v[4 * c + b], w16(b * c, INV));
  float2 u[16];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    float2 a0 = v[4 * c], a1 = v[4 * c + 1], a2 = v[4 * c + 2], a3 = v[4 * c + 3];
    dft4<INV>(a0, a1, a2, a3);
    u[c] = a0; u[c + 4] = a1; u[c + 8] = a2; u[c + 12] = a3;
  }
#pragma unroll
  for (int k = 0; k < 16; k++) v[k] = u[k];
}

// 256-point DFT of one line, 16 threads per line: on entry v[n1] = x[16 n1 + t], on exit v[k2] = X[t + 16 k2].
// sl: this line's LDS (LS float2), tw: W256^m (forward sign) for m < 256.  Contains one __syncthreads (call from every thread).
template <bool INV>
__device__ __forceinline__ void fft256(float2 (&v)[16], int t, float2* sl, const float2* tw) {
  dft16<INV>(v);
#pragma unroll
  for (int k1 = 1; k1 < 16; k1++) {
    float2 w = tw[t * k1];
    if (INV) w.y = -w.y;
    v[k1] = cmul(v[k1], w);
  }
#pragma unroll
  for (int k1 = 0; k1 < 16; k1++) sl[17 * k1 + t] = v[k1];
  __syncthreads();
#pragma unroll
  for (int n2 = 0; n2 < 16; n2++) v[n2] = sl[17 * t + n2];
  dft16<INV>(v);
}

__device__ __forceinline__ void load_tw(float2* tw_s, const float2* tw) {
  tw_s[threadIdx.x] = tw[threadIdx.x];
  __syncthreads();
}

__device__ __forceinline__ int pad_src(int r) { return r < 5 ? 4 - r : (r >= GS + 5 ? 2 * GS + 4 - r : r - 5); }

template <typename T>
__global__ __launch_bounds__(256) void gist_logpad_kernel(const T* __restrict__ img, float* __restrict__ A) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= GP * GP) return;
  const int r = e / GP, c = e - r * GP;
  const float x = (float)img[(size_t)b * GS * GS + pad_src(r) * GS + pad_src(c)];
  A[(size_t)b * GIST_LD * GIST_LD + r * GIST_LD + c] = logf(x + 1.0f);
}

// Out = Lm Rm over the 266 x 266 valid part (row stride GIST_LD).  MODE 0: Lm = C, Rm = X[b], T[b] = product.
// MODE 1: Lm = T[b], Rm = C: L = product, A2[b] = A[b] - L, A[b] = A2^2.   MODE 2: Lm = T[b], Rm = C: L2 = product,
// P[b] (in A[b], 256 x 256 dense) = A2 / (0.2 + sqrt|L2|) on the unpadded part.
template <int MODE>
__global__ __launch_bounds__(256) void gist_gemm_kernel(const float* __restrict__ Cm, float* __restrict__ X, float* __restrict__ T,
                                                        float* __restrict__ A2) {
  __shared__ float Ls[16][64 + 4];
  __shared__ float Rs[16][64 + 4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = (blockIdx.x / 5) * 64, n0 = (blockIdx.x % 5) * 64;
  const size_t img = (size_t)b * GIST_LD * GIST_LD;
  const float* Lm = MODE == 0 ? Cm : T + img;
  const float* Rm = MODE == 0 ? X + img : Cm;
  const int ty = tid >> 4, tx = tid & 15;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < GIST_LD; k0 += 16) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int e = tid + 256 * q;
      const int lr = e >> 4, lk = e & 15;          // Lm tile: 64 rows x 16 k
      const int gr = m0 + lr, gk = k0 + lk;
      Ls[lk][lr] = (gr < GP && gk < GP) ? Lm[gr * GIST_LD + gk] : 0.0f;
      const int rk = e >> 6, rc = e & 63;          // Rm tile: 16 k x 64 columns
      const int hk = k0 + rk, hc = n0 + rc;
      Rs[rk][rc] = (hk < GP && hc < GP) ? Rm[hk * GIST_LD + hc] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; kk++) {
      float a[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { a[i] = Ls[kk][ty + 16 * i]; w[i] = Rs[kk][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = fmaf(a[i], w[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int r = m0 + ty + 16 * i, c = n0 + tx + 16 * j;
      if (r >= GP || c >= GP) continue;
      const size_t o = img + r * GIST_LD + c;
      if (MODE == 0) {
        T[o] = acc[i][j];
      } else if (MODE == 1) {
        const float v = X[o] - acc[i][j];          // libgist.cpp:340
        A2[o] = v;
        X[o] = v * v;                              // :342
      } else if (r >= 5 && r < GS + 5 && c >= 5 && c < GS + 5) {
        X[(size_t)b * GIST_LD * GIST_LD + (r - 5) * GS + (c - 5)] = A2[o] / (0.2f + sqrtf(fabsf(acc[i][j])));   // :386-393, :395
      }
    }
}

// forward transform of the rows of P (real, 256 x 256 dense at the start of each A[b] slot) -> F[b]
__global__ __launch_bounds__(256) void gist_fft_rows_fwd_kernel(const float* __restrict__ P, const float2* __restrict__ tw,
                                                                float2* __restrict__ F) {
  __shared__ float2 s[16 * LS];
  __shared__ float2 tw_s[256];
  load_tw(tw_s, tw);
  const int b = blockIdx.y, line = threadIdx.x >> 4, t = threadIdx.x & 15, r = blockIdx.x * 16 + line;
  const float* p = P + (size_t)b * GIST_LD * GIST_LD + r * GS;
  float2 v[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; n1++) v[n1] = make_float2(p[16 * n1 + t], 0.0f);
  fft256<false>(v, t, s + line * LS, tw_s);
  float2* f = F + (size_t)b * GS * GS + r * GS;
#pragma unroll
  for (int k2 = 0; k2 < 16; k2++) f[t + 16 * k2] = v[k2];
}

// forward transform of the columns of F[b], in place (a workgroup reads its 16-column panel before it writes it)
__global__ __launch_bounds__(256) void gist_fft_cols_fwd_kernel(float2* __restrict__ F, const float2* __restrict__ tw) {
  __shared__ float2 s[16 * LS];
  __shared__ float2 tw_s[256];
  load_tw(tw_s, tw);
  const int b = blockIdx.y, c = threadIdx.x & 15, t = threadIdx.x >> 4, i = blockIdx.x * 16 + c;
  float2* f = F + (size_t)b * GS * GS + i;
  float2 v[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; n1++) v[n1] = f[(16 * n1 + t) * GS];
  fft256<false>(v, t, s + c * LS, tw_s);
#pragma unroll
  for (int k2 = 0; k2 < 16; k2++) f[(t + 16 * k2) * GS] = v[k2];
}

// pair p0 + y = (image (p0 + y) / nf, filter (p0 + y) % nf): inverse columns of F G_k -> Z[y]
__global__ __launch_bounds__(256) void gist_gabor_cols_kernel(const float2* __restrict__ F, const float* __restrict__ G,
                                                              const float2* __restrict__ tw, float2* __restrict__ Z, int p0, int nf) {
  __shared__ float2 s[16 * LS];
  __shared__ float2 tw_s[256];
  load_tw(tw_s, tw);
  const int p = p0 + blockIdx.y, b = p / nf, k = p - b * nf;
  const int c = threadIdx.x & 15, t = threadIdx.x >> 4, i = blockIdx.x * 16 + c;
  const float2* f = F + (size_t)b * GS * GS + i;
  const float* g = G + (size_t)k * GS * GS + i;
  float2 v[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; n1++) {
    const float2 x = f[(16 * n1 + t) * GS];
    const float gv = g[(16 * n1 + t) * GS];
    v[n1] = make_float2(x.x * gv, x.y * gv);      // libgist.cpp:732-737
  }
  fft256<true>(v, t, s + c * LS, tw_s);
  float2* z = Z + (size_t)blockIdx.y * GS * GS + i;
#pragma unroll
  for (int k2 = 0; k2 < 16; k2++) z[(t + 16 * k2) * GS] = v[k2];
}

// inverse rows of Z[y], |.| / (W H) (libgist.cpp:741-748), then the sums of each row over the x blocks of down_N:
// rowsum[p][r][kb] = sum_{nx[kb] <= i < nx[kb+1]} |y(r, i)|, in ascending i
__global__ __launch_bounds__(256) void gist_gabor_rows_kernel(const float2* __restrict__ Z, const float2* __restrict__ tw,
                                                              float* __restrict__ rowsum, int p0, int nb) {
  __shared__ float2 s[16 * LS];
  __shared__ float2 tw_s[256];
  load_tw(tw_s, tw);
  const int line = threadIdx.x >> 4, t = threadIdx.x & 15, r = blockIdx.x * 16 + line;
  const float2* z = Z + (size_t)blockIdx.y * GS * GS + r * GS;
  float2 v[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; n1++) v[n1] = z[16 * n1 + t];
  fft256<true>(v, t, s + line * LS, tw_s);
  __syncthreads();                                   // every line's transpose reads are done: reuse s for the magnitudes
  float* mag = reinterpret_cast<float*>(s) + line * GS;
#pragma unroll
  for (int k2 = 0; k2 < 16; k2++) mag[t + 16 * k2] = sqrtf(v[k2].x * v[k2].x + v[k2].y * v[k2].y) / (float)(GS * GS);
  __syncthreads();
  const int kb = t;
  if (kb < nb) {
    const int i0 = kb * GS / nb, i1 = (kb + 1) * GS / nb;
    float sum = 0.0f;
    for (int i = i0; i < i1; i++) sum += mag[i];
    rowsum[((size_t)(p0 + blockIdx.y) * GS + r) * nb + kb] = sum;
  }
}

// out[b][k N^2 + kb N + l] = (sum over the rows of y block l of rowsum, ascending) / area   (down_N, libgist.cpp:611-624)
__global__ __launch_bounds__(256) void gist_blocks_kernel(const float* __restrict__ rowsum, int nf, int nb, float* __restrict__ out) {
  const int b = blockIdx.x, D = nf * nb * nb;
  float* o = out + (size_t)b * D;
  int bad = 0;
  for (int e = threadIdx.x; e < D; e += 256) {
    const int k = e / (nb * nb), rem = e - k * nb * nb, kb = rem / nb, l = rem - kb * nb;
    const int y0 = l * GS / nb, y1 = (l + 1) * GS / nb, x0 = kb * GS / nb, x1 = (kb + 1) * GS / nb;
    const float* rs = rowsum + (size_t)(b * nf + k) * GS * nb + kb;
    float mean = 0.0f;
    for (int r = y0; r < y1; r++) mean += rs[r * nb];
    const float denom = (float)(y1 - y0) * (float)(x1 - x0);
    const float v = mean / denom;
    bad |= !isfinite(v);
    o[e] = v;
  }
  if (__syncthreads_or(bad))
    for (int e = threadIdx.x; e < D; e += 256) o[e] = __builtin_nanf("");
}

}  // namespace

size_t gist_scratch_floats(int chunk, int nf, int nb) {
  return (size_t)3 * chunk * GIST_LD * GIST_LD + (size_t)2 * chunk * GS * GS + (size_t)2 * GIST_PAIRS * GS * GS +
         (size_t)chunk * nf * GS * nb;
}

void launch_gist(hipStream_t st, const void* img, bool u8, int n, int nb, int nf, const float* circ, const float* gabor,
                 const float2* tw, float* scratch, float* out) {
  float* A = scratch;
  float* T = A + (size_t)n * GIST_LD * GIST_LD;
  float* A2 = T + (size_t)n * GIST_LD * GIST_LD;
  float2* F = reinterpret_cast<float2*>(A2 + (size_t)n * GIST_LD * GIST_LD);
  float2* Z = F + (size_t)n * GS * GS;
  float* rowsum = reinterpret_cast<float*>(Z + (size_t)GIST_PAIRS * GS * GS);
  const dim3 blk(256);
  if (u8) gist_logpad_kernel<uint8_t><<<dim3((GP * GP + 255) / 256, n), blk, 0, st>>>(static_cast<const uint8_t*>(img), A);
  else gist_logpad_kernel<float><<<dim3((GP * GP + 255) / 256, n), blk, 0, st>>>(static_cast<const float*>(img), A);
  gist_gemm_kernel<0><<<dim3(25, n), blk, 0, st>>>(circ, A, T, A2);
  gist_gemm_kernel<1><<<dim3(25, n), blk, 0, st>>>(circ, A, T, A2);
  gist_gemm_kernel<0><<<dim3(25, n), blk, 0, st>>>(circ, A, T, A2);
  gist_gemm_kernel<2><<<dim3(25, n), blk, 0, st>>>(circ, A, T, A2);
  gist_fft_rows_fwd_kernel<<<dim3(16, n), blk, 0, st>>>(A, tw, F);
  gist_fft_cols_fwd_kernel<<<dim3(16, n), blk, 0, st>>>(F, tw);
  const int pairs = n * nf;
  for (int p0 = 0; p0 < pairs; p0 += GIST_PAIRS) {
    const int np = pairs - p0 < GIST_PAIRS ? pairs - p0 : GIST_PAIRS;
    gist_gabor_cols_kernel<<<dim3(16, np), blk, 0, st>>>(F, gabor, tw, Z, p0, nf);
    gist_gabor_rows_kernel<<<dim3(16, np), blk, 0, st>>>(Z, tw, rowsum, p0, nb);
  }
  gist_blocks_kernel<<<dim3(n), blk, 0, st>>>(rowsum, nf, nb, out);
}

}  // namespace pr
