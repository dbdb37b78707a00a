// submap.hip — local submaps (no reference counterpart): for every slot of a pair list the clouds of the map rows
// centre - w .. centre + w gathered into ONE cloud in the centre row's camera frame, as a CSR set pr_icp_pairs_dev reads as it stands.  The
// rule is in include/place_recognition.h and restated in tests/submap_np.py; the device equals it bit for bit (fp64, no contraction, - x +
// only).  Every grid depends on the create sizes only and the map's count is read from device memory, so one captured run serves every count.
//   plan     a wave per slot, a lane per walked row (2 w + 1 <= 63): eligibility, the slot's capacity rule by a wave prefix sum, the slot's
//            entry list in walk order (row, source start, length, start inside the slot), total, flags, rows taken
//   scan     one workgroup: the slots' totals scanned in chunks of 256 with the overflow rule (a chunk that does not fit as a whole is
//            placed slot by slot), out_offs, out_rows, info, every slot's base
//   gather   a workgroup per (slot, entry) and chunk, a lane per point in a grid-stride loop: the centre row copied bit for bit, every
//            other row through y = R_c (R_r^T (x - t_r)) + t_c, the two poses loaded once (uniform addresses)
// No floating-point atomics, integer atomics on LDS words only, no workgroup waits for another, every loop is bounded by a create size.
// Plain C++, vector stores only.
#include "submap.hpp"
#include "trajeval.hpp"

namespace pr {
namespace {

using namespace traj;

constexpr int T = SUBMAP_T;
constexpr int WAVES = SUBMAP_T / 64;
static_assert(2 * SUBMAP_MAX_W + 1 <= 63, "a lane per walked row");

// ------------------------------------------------------------------------------------------------ plan
__global__ __launch_bounds__(T) void submap_plan_kernel(SubmapView v, SubmapIn in, SubmapParams prm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * WAVES + wave, L = v.L;
  if (p >= v.slot_capacity) return;                              // a whole wave; the kernel has no barrier
  const size_t o = (size_t)p * L + lane;
  if (p >= in.c) {                                               // a slot the call does not use: nothing taken
    if (lane < L) v.dst[o] = -1;
    if (lane == 0) { v.total[p] = 0; v.flags[p] = 0; v.taken[p] = 0; }
    return;
  }
  const int n = clampi(in.n[0], v.keyframe_capacity);            // a scribbled count never forms an address
  const int centre = in.center[p];                               // p < c <= slot_capacity
  const bool odd = (lane & 1) != 0;
  const int dist = (lane + 1) >> 1;
  const long long r = (long long)centre + (odd ? -dist : dist);  // lane 0: the centre, then centre - 1, centre + 1, centre - 2, ...
  const bool walked = lane < 2 * prm.w + 1 && (lane == 0 || odd || prm.past_only == 0);
  bool ok = walked && centre >= 0 && r >= 0 && r < n;
  if (ok) {
    const double* q = in.poses + (size_t)r * 12;                 // 0 <= r < n <= keyframe_capacity
    for (int k = 0; k < 12; k++) ok = ok && fin(q[k]);
  }
  const bool cen_ok = __shfl(ok ? 1 : 0, 0) != 0;                // every lane takes part in the shuffle
  if (ok && lane > 0 && in.avoid != nullptr) {                   // the centre is exempt; 64 bits: the difference cannot wrap
    long long d = r - (long long)in.avoid[p];
    if (d < 0) d = -d;
    ok = d > (long long)prm.avoid_gap;
  }
  long long a = 0;
  int len = 0;
  if (ok) {
    a = in.offs[r];
    const long long b = in.offs[r + 1];                          // offs holds keyframe_capacity + 1 entries
    ok = a >= 0 && b >= a && b - a <= (long long)v.max_cloud_points;       // a scribbled length forms no address
    len = ok ? (int)(b - a) : 0;
  }
  if (!cen_ok) ok = false;
  long long incl = ok ? len : 0;                                 // points up to and including this lane's row, in walk order
  for (int d = 1; d < 64; d <<= 1) {
    const long long u = __shfl_up(incl, d);
    if (lane >= d) incl += u;
  }
  const unsigned long long over = __ballot(ok && incl > (long long)prm.max_pts);
  const int cut = over ? __builtin_ctzll(over) : 64;             // the first row that does not fit ends the walk
  const bool take = ok && lane < cut;
  const unsigned long long tm = __ballot(take);
  const long long upto = __shfl(incl, cut > 0 ? cut - 1 : 0);
  if (lane < L) {
    v.row[o] = take || (lane == 0 && cen_ok) ? (int)r : -1;       // the centre's pose is read even where its own cloud is skipped
    v.dst[o] = take ? (int)(incl - len) : -1;
    v.len[o] = take ? len : 0;
    v.src[o] = take ? a : 0;
  }
  if (lane == 0) {
    v.total[p] = cut > 0 ? (int)upto : 0;                        // <= max_pts
    v.flags[p] = (over ? SUBMAP_TRUNCATED : 0) | (centre >= 0 && !cen_ok ? SUBMAP_NO_CENTER : 0);
    v.taken[p] = __popcll(tm);
  }
}

// ------------------------------------------------------------------------------------------------ scan
__global__ __launch_bounds__(T) void submap_scan_kernel(SubmapView v, SubmapIn in, SubmapOut out) {
  __shared__ long long s_scan[T];
  __shared__ long long s_base;
  __shared__ int s_nonempty, s_flags;
  const int tid = threadIdx.x, c = in.c, S = v.slot_capacity;
  if (tid == 0) { s_base = 0; s_nonempty = 0; s_flags = 0; }
  __syncthreads();
  for (int p0 = 0; p0 < c; p0 += T) {                            // block-uniform bounds
    const int p = p0 + tid;
    const bool act = p < c;
    const int tot = act ? v.total[p] : 0, fl = act ? v.flags[p] : 0, tk = act ? v.taken[p] : 0;
    s_scan[tid] = tot;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {
      const long long u = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += u;
      __syncthreads();
    }
    const long long base0 = s_base, incl = s_scan[tid], chunk = s_scan[T - 1];
    __syncthreads();                                             // everyone holds base0 and the chunk's sum
    long long start;
    bool placed = true;
    if (base0 + chunk <= v.point_capacity) {                     // the whole chunk fits: the scan places it
      start = base0 + incl - tot;
      if (tid == 0) s_base = base0 + chunk;
    } else {                                                     // slot by slot: one that does not fit is empty, the next goes behind the last that fits
      s_scan[tid] = tot;
      __syncthreads();
      if (tid == 0) {
        long long cur = base0;
        for (int k = 0; k < T; k++) {
          const long long t = s_scan[k];
          if (cur + t <= v.point_capacity) { s_scan[k] = cur; cur += t; }
          else s_scan[k] = -1 - cur;
        }
        s_base = cur;
      }
      __syncthreads();
      const long long x = s_scan[tid];
      placed = x >= 0;
      start = placed ? x : -1 - x;
    }
    if (act) {
      out.offs[p] = start;
      out.rows[2 * (size_t)p] = placed ? tk : 0;
      out.rows[2 * (size_t)p + 1] = fl | (placed ? 0 : SUBMAP_OVERFLOW);
      v.base[p] = placed ? start : -1;
      if (placed && tk > 0) atomicAdd(&s_nonempty, 1);
      const int f = fl | (placed ? 0 : SUBMAP_OVERFLOW);
      if (f) atomicOr(&s_flags, f);
    }
    __syncthreads();                                             // s_base and s_scan before the next chunk
  }
  const long long end = s_base;
  for (int p = c + tid; p <= S; p += T) {
    out.offs[p] = end;
    if (p < S) { out.rows[2 * (size_t)p] = 0; out.rows[2 * (size_t)p + 1] = 0; v.base[p] = -1; }
  }
  if (tid == 0) {
    out.info[0] = s_nonempty;
    out.info[1] = (int)(unsigned)(end & 0xffffffffll);
    out.info[2] = (int)(end >> 32);
    out.info[3] = s_flags;
  }
}

// ------------------------------------------------------------------------------------------------ gather
__global__ __launch_bounds__(T) void submap_gather_kernel(SubmapView v, SubmapIn in, SubmapOut out) {
  const int item = blockIdx.x, L = v.L;
  const int p = item / L, j = item - p * L;
  if (p >= in.c) return;                                         // block-uniform: the kernel has no barrier
  const long long base = v.base[p];
  if (base < 0) return;
  const size_t o = (size_t)p * L + j;
  const int dst = v.dst[o];
  if (dst < 0) return;
  const int len = v.len[o];                                      // 0 <= len <= max_cloud_points, dst + len <= the slot's total
  const int step = T * (int)gridDim.y;
  const int i0 = (int)blockIdx.y * T + (int)threadIdx.x;
  if (j == 0) {                                                  // the centre row: the bits as they are
    const unsigned long long* x = reinterpret_cast<const unsigned long long*>(in.xyz) + (size_t)v.src[o] * 3;
    unsigned long long* y = reinterpret_cast<unsigned long long*>(out.xyz) + (size_t)(base + dst) * 3;
    for (int i = i0; i < len; i += step) {
      const unsigned long long x0 = x[(size_t)i * 3], x1 = x[(size_t)i * 3 + 1], x2 = x[(size_t)i * 3 + 2];
      y[(size_t)i * 3] = x0; y[(size_t)i * 3 + 1] = x1; y[(size_t)i * 3 + 2] = x2;
    }
    return;
  }
  const double* x = in.xyz + (size_t)v.src[o] * 3;
  double* y = out.xyz + (size_t)(base + dst) * 3;
  double Rc[9], tc[3], Rr[9], tr[3];
  load_pose(in.poses + (size_t)v.row[(size_t)p * L] * 12, Rc, tc);         // rows the plan found below n; uniform addresses
  load_pose(in.poses + (size_t)v.row[o] * 12, Rr, tr);
  for (int i = i0; i < len; i += step) {
    const double d0 = x[(size_t)i * 3] - tr[0], d1 = x[(size_t)i * 3 + 1] - tr[1], d2 = x[(size_t)i * 3 + 2] - tr[2];
    const double u0 = (Rr[0] * d0 + Rr[3] * d1) + Rr[6] * d2;
    const double u1 = (Rr[1] * d0 + Rr[4] * d1) + Rr[7] * d2;
    const double u2 = (Rr[2] * d0 + Rr[5] * d1) + Rr[8] * d2;
    y[(size_t)i * 3] = ((Rc[0] * u0 + Rc[1] * u1) + Rc[2] * u2) + tc[0];
    y[(size_t)i * 3 + 1] = ((Rc[3] * u0 + Rc[4] * u1) + Rc[5] * u2) + tc[1];
    y[(size_t)i * 3 + 2] = ((Rc[6] * u0 + Rc[7] * u1) + Rc[8] * u2) + tc[2];
  }
}

}  // namespace

void launch_submap(hipStream_t st, const SubmapView& v, const SubmapIn& in, const SubmapParams& prm, const SubmapOut& out) {
  const dim3 blk(T);
  hipLaunchKernelGGL(submap_plan_kernel, dim3((v.slot_capacity + WAVES - 1) / WAVES), blk, 0, st, v, in, prm);
  hipLaunchKernelGGL(submap_scan_kernel, dim3(1), blk, 0, st, v, in, out);
  hipLaunchKernelGGL(submap_gather_kernel, dim3(v.slot_capacity * v.L, v.chunks), blk, 0, st, v, in, out);
}

}  // namespace pr
