// gist_tables.hpp — the host-built tables of the GIST generator (gist.cpp uploads them, gist_gen.hip reads them): the Gabor bank of
// create_gabor (GIST/src/libgist.cpp:190-272) in the reference's own float / double arithmetic and the whitening circulant of prefilt
// (:314-395).  Plain C++ (tests/native/gist_tables_dump.cpp builds it on the host for tests/test_gist_tables.py).
#pragma once
#include <cmath>
#include <vector>

namespace pr {
namespace gist {

constexpr int GS = 256;                              // image side
constexpr int GP = 266;                              // padded side (5 px each way, libgist.cpp:288)
constexpr int LD = 272;                              // row stride of the padded planes (kernels.hpp: GIST_LD)
constexpr double REF_PI = 3.14159265358979323846;   // libgist.cpp:20 (a double constant)

// fftshift of an even-sized w x w plane (libgist.cpp:158-186): element (j, i) moves to ((j + w/2) % w, (i + w/2) % w)
inline void fftshift(std::vector<float>& a, int w) {
  std::vector<float> b(a.size());
  for (int j = 0; j < w; j++)
    for (int i = 0; i < w; i++) b[((j + w / 2) % w) * w + (i + w / 2) % w] = a[j * w + i];
  a.swap(b);
}

// create_gabor (libgist.cpp:190-272) at 256 x 256, type by type: param[] are floats computed in double, fr and f in float
// (sqrt / atan2 of floats), the exponent mixes a float product with a double term (M_PI), exp in double, stored as float.
inline std::vector<float> gabor_table(int n_scale, const int* orients) {
  std::vector<float> fr(GS * GS), f(GS * GS);
  for (int j = 0; j < GS; j++)
    for (int i = 0; i < GS; i++) {
      const float fx = (float)i - GS / 2.0f, fy = (float)j - GS / 2.0f;
      fr[j * GS + i] = std::sqrt(fx * fx + fy * fy);
      f[j * GS + i] = std::atan2(fy, fx);
    }
  fftshift(fr, GS);
  fftshift(f, GS);
  std::vector<float> G;
  for (int s = 1; s <= n_scale; s++)
    for (int o = 1; o <= orients[s - 1]; o++) {
      const float p0 = 0.35f;
      const float p1 = (float)(0.3 / std::pow((double)1.85f, (double)(s - 1)));
      const float p2 = (float)(16 * std::pow((double)orients[s - 1], 2.0) / std::pow(32.0, 2.0));
      const float p3 = (float)(REF_PI / orients[s - 1] * (o - 1));
      const size_t base = G.size();
      G.resize(base + GS * GS);
      for (int e = 0; e < GS * GS; e++) {
        float tmp = f[e] + p3;
        if (tmp < -REF_PI) tmp = (float)(tmp + 2.0f * REF_PI);
        else if (tmp > REF_PI) tmp = (float)(tmp - 2.0f * REF_PI);
        const float a = -10.0f * p0 * (fr[e] / GS / p1 - 1) * (fr[e] / GS / p1 - 1);
        const double bterm = 2.0f * p2 * REF_PI * tmp * tmp;
        G[base + e] = (float)std::exp(a - bterm);
      }
    }
  return G;
}

// The whitening low-pass of prefilt (libgist.cpp:314-395) on the 266 x 266 padded image, ifft2(fft2(X) gfc) / (w h), with
// gfc = exp(-(fx^2 + fy^2) / s1^2) = g(fx) g(fy): C X C with C[i][j] = c[(i - j) mod 266], c[d] = (1/266) sum_p g(p) cos(2 pi p d / 266)
// (g even, so the product is real; FFTW's imaginary part is rounding noise).  g and c in double, C stored as float.
inline std::vector<float> circulant() {
  const float s1 = (float)(4 / std::sqrt(std::log(2.0)));   // fc = 4 (bw_gist_scaletab, :929)
  std::vector<double> g(GP), c(GP);
  for (int p = 0; p < GP; p++) {
    const double fx = p < GP / 2 ? p : p - GP;               // frequency at fftshifted position p
    g[p] = std::exp(-(fx * fx) / ((double)s1 * s1));
  }
  for (int d = 0; d <= GP / 2; d++) {                        // c is even: computed once per distance, so C is exactly symmetric (C X C = C X C^T)
    double acc = 0.0;
    for (int p = 0; p < GP; p++) acc += g[p] * std::cos(2.0 * REF_PI * (double)((p * d) % GP) / GP);
    c[d] = c[(GP - d) % GP] = acc / GP;
  }
  std::vector<float> C((size_t)LD * LD, 0.0f);
  for (int i = 0; i < GP; i++)
    for (int j = 0; j < GP; j++) C[(size_t)i * LD + j] = (float)c[(i - j + GP) % GP];
  return C;
}

}  // namespace gist
}  // namespace pr
