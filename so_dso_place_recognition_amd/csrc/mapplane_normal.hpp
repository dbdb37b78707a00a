// mapplane_normal.hpp — the normal of ONE world row through the localiser's voxel index (the rule of pr_mapplane_normals_dev,
// include/place_recognition.h) as inlined device code.  mapplane.hip (one lane per row of out_capacity) and mapgrow.hip
// (the rows around a keyframe's new rows) include it, so both run the same instructions on the same inputs and leave the same bits.
// Both files are built with -ffp-contract=off.  A row word read from the table is compared with out_capacity before an address is formed;
// the probe is a bounded for loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pr {
namespace mapplane_dev {

typedef unsigned long long u64;

constexpr u64 EMPTY = ~(u64)0;
constexpr double CELL_LIM = 1048576.0;                           // 2^20
constexpr int MP_SWEEPS = 8;                                     // cyclic Jacobi sweeps of the 3 x 3 (fixed)

struct TableView { const ulonglong2* tab; const double* xyz; const int* state; int64_t ocap; double cell; int log2T; };

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the row the table holds for three biased voxel indices (2^20 is voxel 0), or EMPTY: at most T steps
__device__ __forceinline__ u64 held_row(const TableView& v, unsigned c0, unsigned c1, unsigned c2) {
  if (!(c0 < 2097152u && c1 < 2097152u && c2 < 2097152u)) return EMPTY;       // a key outside the 21-bit range is dropped
  const u64 key = ((u64)c0 << 42) | ((u64)c1 << 21) | (u64)c2;
  const u64 Tn = (u64)1 << v.log2T, mask = Tn - 1;
  u64 a = (key * 0x9E3779B97F4A7C15ull) >> (64 - v.log2T);
  for (u64 step = 0; step < Tn; step++, a = (a + 1) & mask) {                // ends at an empty slot, at the key or after T steps
    const ulonglong2 e = v.tab[a];
    if (e.x == EMPTY) return EMPTY;
    if (e.x == key) return e.y;
  }
  return EMPTY;
}

// a finite row's biased voxel indices by the index's formula (IEEE division, compared as a double); false when one is out of range
__device__ __forceinline__ bool voxel_of(const double x[3], double cell, int f[3]) {
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double c = floor(x[a] / cell);
    const bool ok = c >= -CELL_LIM && c < CELL_LIM;
    in = in && ok;
    f[a] = ok ? (int)c + 1048576 : 0;
  }
  return in;
}

// one Jacobi rotation of the symmetric A about (p, q), r the third index; V's columns follow
__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&V)[3][3], int p, int q, int r) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[p][p] = A[p][p] - t * apq;
  A[q][q] = A[q][q] + t * apq;
  A[p][q] = 0.0; A[q][p] = 0.0;
  const double arp = A[r][p], arq = A[r][q];
  A[r][p] = c * arp - s * arq; A[p][r] = A[r][p];
  A[r][q] = s * arp + c * arq; A[q][r] = A[r][q];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double vp = V[a][p], vq = V[a][q];
    V[a][p] = c * vp - s * vq;
    V[a][q] = s * vp + c * vq;
  }
}

// the normal n and the ninfo word of row j (0 <= j < out_capacity) under the count R (clamped by the caller into 0 .. out_capacity)
__device__ __forceinline__ void row_normal(const TableView& v, int64_t j, int64_t R, double r2, int min_nbrs, double max_ratio, double n[3],
                                           int* ninfo) {
  n[0] = 0.0; n[1] = 0.0; n[2] = 0.0;
  int info = 0;
  bool indexed = false;
  double x[3] = {0.0, 0.0, 0.0};
  int f[3] = {0, 0, 0};
  if (j < R) {
    const double* q = v.xyz + 3 * (size_t)j;
    x[0] = q[0]; x[1] = q[1]; x[2] = q[2];
    if (finite3(x[0], x[1], x[2])) {
      const bool in = voxel_of(x, v.cell, f);
      indexed = in && held_row(v, (unsigned)f[0], (unsigned)f[1], (unsigned)f[2]) == (u64)j;      // the smallest row of its key
    }
  }
  if (indexed) {
    int k = 0;
    double s[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // S: 00 01 02 11 12 22
    for (int d0 = -1; d0 <= 1; d0++)
      for (int kk = 0; kk < 9; kk++) {
        const u64 row = held_row(v, (unsigned)(f[0] + d0), (unsigned)(f[1] + (kk / 3 - 1)), (unsigned)(f[2] + (kk % 3 - 1)));
        if (row >= (u64)v.ocap) continue;                        // (EMPTY included) row < out_capacity before an address is formed
        const double* q = v.xyz + 3 * (size_t)row;
        const double dx = q[0] - x[0], dy = q[1] - x[1], dz = q[2] - x[2];
        const double d2 = ((dx * dx) + dy * dy) + dz * dz;
        if (!(d2 < r2)) continue;
        k++;
        s[0] += dx; s[1] += dy; s[2] += dz;
        S[0] += dx * dx; S[1] += dx * dy; S[2] += dx * dz; S[3] += dy * dy; S[4] += dy * dz; S[5] += dz * dz;
      }
    const double kd = (double)k;
    double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    A[0][0] = S[0] - (s[0] * s[0]) / kd; A[0][1] = S[1] - (s[0] * s[1]) / kd; A[0][2] = S[2] - (s[0] * s[2]) / kd;
    A[1][1] = S[3] - (s[1] * s[1]) / kd; A[1][2] = S[4] - (s[1] * s[2]) / kd; A[2][2] = S[5] - (s[2] * s[2]) / kd;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    for (int sweep = 0; sweep < MP_SWEEPS; sweep++) {
      jacobi_rotate(A, V, 0, 1, 2);
      jacobi_rotate(A, V, 0, 2, 1);
      jacobi_rotate(A, V, 1, 2, 0);
    }
    double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2], t;
    int i0 = 0, i1 = 1, i2 = 2, ti;                              // a stable sort of three: the lower index first on ties
    if (l1 < l0) { t = l0; l0 = l1; l1 = t; ti = i0; i0 = i1; i1 = ti; }
    if (l2 < l1) { t = l1; l1 = l2; l2 = t; ti = i1; i1 = i2; i2 = ti; }
    if (l1 < l0) { t = l0; l0 = l1; l1 = t; ti = i0; i0 = i1; i1 = ti; }
    const bool valid = k >= min_nbrs && finite3(l0, l1, l2) && l1 > 0.0 && l0 <= max_ratio * l1;
    info = valid ? k : -k;
    if (valid) {
      double e[3];
#pragma unroll
      for (int a = 0; a < 3; a++) e[a] = i0 == 0 ? V[a][0] : (i0 == 1 ? V[a][1] : V[a][2]);
      const double nrm = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
#pragma unroll
      for (int a = 0; a < 3; a++) e[a] = e[a] / nrm;
      double mag = fabs(e[0]), lead = e[0];                        // the component of largest magnitude, the lowest index on a tie
      if (fabs(e[1]) > mag) { mag = fabs(e[1]); lead = e[1]; }
      if (fabs(e[2]) > mag) lead = e[2];
      const bool flip = lead < 0.0;
#pragma unroll
      for (int a = 0; a < 3; a++) n[a] = flip ? -e[a] : e[a];
    }
  }
  *ninfo = info;
}

}  // namespace mapplane_dev
}  // namespace pr
