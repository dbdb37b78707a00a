// snapshot.hip — the resident state packed into one self-describing blob and unpacked from one, on the device.  The
// format and the rule are in include/place_recognition.h and restated in tests/snapshot_np.py; the blob equals the restatement's bytes.
// Every grid depends on the create capacities only and every count is read from device memory, so one captured call serves every count.
//   pack:    plan    one thread: the counts, clamped; rows, offset and length of every section; does the blob fit
//            copy    grid (x, section): a lane takes 16 bytes of a section, stores them (zeros behind the section's end up to its 64-byte
//                    pad) and mixes its two 8-byte words into the section's checksum: ONE read of the data
//            finish  one thread: header, section table (counts, checksums, state words, capacities), the table's own checksum, info
//   unpack:  header  one thread: magic, version, the table against the handle's sections and the destination's capacities
//            sum     grid (x, section): the checksum of every section that passed, read through validated extents only
//            verify  one workgroup: checksums, the map's offsets, the session starts; the decision; info
//            scatter grid (x, section): switched off by the decision; the saved rows into the destination, the state words as saved
// Integer arithmetic only; the only atomics are 64-bit integer adds, whose sum does not depend on their order, and integer LDS atomics.
// No workgroup waits for another.  Plain C++, vector stores only.
#include "snapshot.hpp"

namespace pr {
namespace {

typedef unsigned long long u64;
typedef long long i64;

__device__ __forceinline__ i64 clampll(i64 v, i64 lo, i64 hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ i64 pad64(i64 b) { return (b + 63) & ~63LL; }

// the fixed integer mix of (word, word index): a bijection of the word for every index, so a changed word changes its term
__device__ __forceinline__ u64 mix(u64 w, u64 i) {
  u64 x = w ^ ((i + 1) * 0x9E3779B97F4A7C15ULL);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27; x *= 0x94D049BB133111EBULL;
  x ^= x >> 31;
  return x;
}

// the 16 bytes at byte b of a section of `len` bytes (a multiple of 4): one 16-byte load where the unit is whole and the address allows
// it, else 4-byte loads below the section's end and zeros behind it
__device__ __forceinline__ uint4 load_unit(const char* p, i64 b, i64 len, bool aligned16) {
  uint4 q = make_uint4(0u, 0u, 0u, 0u);
  if (aligned16 && b + 16 <= len) return *reinterpret_cast<const uint4*>(p + b);
  if (b < len) q.x = *reinterpret_cast<const unsigned*>(p + b);
  if (b + 4 < len) q.y = *reinterpret_cast<const unsigned*>(p + b + 4);
  if (b + 8 < len) q.z = *reinterpret_cast<const unsigned*>(p + b + 8);
  if (b + 12 < len) q.w = *reinterpret_cast<const unsigned*>(p + b + 12);
  return q;
}
// the unit's two checksum terms: words 2u and 2u + 1 of the section, those that begin below its end (a 4-byte tail is zero-extended)
__device__ __forceinline__ u64 unit_terms(uint4 q, i64 u, i64 len) {
  u64 a = 0;
  if (16 * u < len) a += mix((u64)q.x | ((u64)q.y << 32), (u64)(2 * u));
  if (16 * u + 8 < len) a += mix((u64)q.z | ((u64)q.w << 32), (u64)(2 * u + 1));
  return a;
}
// the workgroup's sum by a fixed tree, then ONE integer atomic add per workgroup
__device__ __forceinline__ void block_add(u64 acc, u64* sums, int s) {
  __shared__ u64 sh[256];
  const int tid = threadIdx.x;
  sh[tid] = acc;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  if (tid == 0 && sh[0] != 0) atomicAdd(&sums[s], sh[0]);
}
__device__ __forceinline__ i64* ctl_of(const SnapshotView& v, int s) { return v.ctl + 8 + 4 * s; }
__device__ __forceinline__ i64 header_extent(int ns) { return SNAPSHOT_HEADER_BYTES + (i64)SNAPSHOT_ENTRY_BYTES * ns; }

// ------------------------------------------------------------------------------------------------ pack
__global__ void snapshot_pack_plan_kernel(SnapshotView v, i64 blob_capacity) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  i64 off = header_extent(v.ns);
  for (int p = 0; p < v.np; p++) {
    const SnapshotPart& P = v.part[p];
    const i64 n = clampll(P.state[0], P.count_min, P.caps[0]);                  // a scribbled count never forms an address
    const i64 pts = P.offs ? clampll(P.offs[n], 0, P.caps[1]) : 0;              // n <= keyframe_capacity: offs has that row
    for (int s = P.first_section; s < P.first_section + P.sections; s++) {
      const SnapshotSection& S = v.sec[s];
      const i64 rows = S.rows_of == SNAPSHOT_ROWS_POINTS ? pts : (S.rows_of == SNAPSHOT_ROWS_N1 ? n + 1 : n);
      const i64 len = rows * S.row_bytes;
      i64* c = ctl_of(v, s);
      c[0] = rows; c[1] = off; c[2] = len; c[3] = 0;
      v.sums[s] = 0;
      off += pad64(len);
    }
  }
  const bool ok = off <= blob_capacity;
  v.ctl[0] = ok ? 1 : 0; v.ctl[1] = ok ? 0 : SNAPSHOT_OVERFLOW; v.ctl[2] = -1; v.ctl[3] = off;
}

__global__ __launch_bounds__(256) void snapshot_pack_copy_kernel(SnapshotView v, char* __restrict__ blob) {
  const int s = blockIdx.y;
  if (v.ctl[0] == 0) return;                                                     // the blob would not fit: nothing behind the header
  const i64* c = ctl_of(v, s);
  const i64 off = c[1], len = c[2], units = pad64(len) >> 4;
  const char* src = static_cast<const char*>(v.sec[s].base);
  char* dst = blob + off;                                                        // 16-byte aligned: the blob is, and off is a multiple of 64
  const bool aligned16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  u64 acc = 0;
  for (i64 u = (i64)blockIdx.x * 256 + threadIdx.x; u < units; u += (i64)gridDim.x * 256) {
    const uint4 q = load_unit(src, 16 * u, len, aligned16);
    *reinterpret_cast<uint4*>(dst + 16 * u) = q;
    acc += unit_terms(q, u, len);
  }
  block_add(acc, v.sums, s);
}

__global__ void snapshot_pack_finish_kernel(SnapshotView v, char* __restrict__ blob, i64 blob_capacity, i64* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const i64 ext = header_extent(v.ns);
  const bool ok = v.ctl[0] != 0;
  if (ext <= blob_capacity) {
    i64* h = reinterpret_cast<i64*>(blob);
    u64 tsum = 0;
    for (int s = 0; s < v.ns; s++) {
      const SnapshotSection& S = v.sec[s];
      const SnapshotPart& P = v.part[S.part];
      const i64* c = ctl_of(v, s);
      i64 e[16];
      e[0] = S.kind; e[1] = S.subtype; e[2] = S.array; e[3] = c[0]; e[4] = S.row_bytes; e[5] = c[1]; e[6] = c[2];
      e[7] = ok ? (i64)v.sums[s] : 0;
      e[8] = (i64)((u64)(unsigned)P.state[0] | ((u64)(unsigned)P.state[1] << 32));   // the four state words verbatim
      e[9] = (i64)((u64)(unsigned)P.state[2] | ((u64)(unsigned)P.state[3] << 32));
      e[10] = P.caps[0]; e[11] = P.caps[1]; e[12] = P.caps[2]; e[13] = P.caps[3]; e[14] = S.part; e[15] = 0;
      i64* t = h + 8 + 16 * s;
      for (int k = 0; k < 16; k++) { t[k] = e[k]; tsum += mix((u64)e[k], (u64)(16 * s + k)); }
    }
    h[0] = SNAPSHOT_MAGIC; h[1] = SNAPSHOT_VERSION; h[2] = v.ns; h[3] = v.ctl[3]; h[4] = ext; h[5] = (i64)tsum; h[6] = 0; h[7] = 0;
  }
  info[0] = v.ctl[3]; info[1] = v.ns; info[2] = v.ctl[1]; info[3] = 0;
}

// ------------------------------------------------------------------------------------------------ unpack
__global__ void snapshot_unpack_header_kernel(SnapshotView v, const char* __restrict__ blob, i64 blob_bytes) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int flags = 0, first = 0x7fffffff;
  for (int s = 0; s < v.ns; s++) {
    i64* c = ctl_of(v, s);
    c[0] = 0; c[1] = -1; c[2] = 0; c[3] = 0;                                     // offset -1: the section did not pass
    v.sums[s] = 0;
  }
  const i64* h = reinterpret_cast<const i64*>(blob);
  bool table = false;
  i64 nsec = 0;
  if (blob_bytes < SNAPSHOT_HEADER_BYTES) flags |= SNAPSHOT_TRUNCATED;
  else if (h[0] != SNAPSHOT_MAGIC) flags |= SNAPSHOT_BAD_MAGIC;
  else if (h[1] != SNAPSHOT_VERSION) flags |= SNAPSHOT_BAD_VERSION;
  else {
    nsec = h[2];
    if (nsec < 0 || nsec > SNAPSHOT_MAX_SECTIONS || header_extent((int)nsec) > blob_bytes) flags |= SNAPSHOT_TRUNCATED;
    else table = true;
  }
  if (table) {
    u64 tsum = 0;
    for (int k = 0; k < 16 * (int)nsec; k++) tsum += mix((u64)h[8 + k], (u64)k);
    if ((i64)tsum != h[5]) flags |= SNAPSHOT_CHECKSUM;                           // the table's own checksum: no section is named
    if (nsec != v.ns) { flags |= SNAPSHOT_MISSING; first = (int)(nsec < v.ns ? nsec : v.ns); }
    i64 prev_end = header_extent((int)nsec);
    for (int s = 0; s < v.ns && s < (int)nsec; s++) {
      const SnapshotSection& S = v.sec[s];
      const i64* e = h + 8 + 16 * s;
      int bad = 0;
      const i64 rows = e[3], off = e[5], len = e[6];
      if (e[0] != S.kind || e[1] != S.subtype || e[2] != S.array || e[4] != S.row_bytes) bad = SNAPSHOT_MISSING;
      else if (rows < 0 || rows > S.cap_rows) bad = SNAPSHOT_CAPACITY;           // the DESTINATION's capacity
      else if (len != rows * S.row_bytes || off < prev_end || (off & 63) != 0 || off > blob_bytes || len > blob_bytes - off)
        bad = SNAPSHOT_TRUNCATED;
      if (bad) { flags |= bad; if (s < first) first = s; continue; }
      i64* c = ctl_of(v, s);
      c[0] = rows; c[1] = off; c[2] = len; c[3] = e[7];
      prev_end = off + pad64(len);
    }
    // the sections of one part agree on its counts
    for (int p = 0; p < v.np; p++) {
      const SnapshotPart& P = v.part[p];
      i64 n = -1, pts = -1;
      for (int s = P.first_section; s < P.first_section + P.sections; s++) {
        const i64* c = ctl_of(v, s);
        if (c[1] < 0) continue;
        const int ro = v.sec[s].rows_of;
        const i64 r = ro == SNAPSHOT_ROWS_N1 ? c[0] - 1 : c[0];
        i64& want = ro == SNAPSHOT_ROWS_POINTS ? pts : n;
        if (want < 0 && r >= 0) want = r;
        else if (r != want) { flags |= SNAPSHOT_TRUNCATED; if (s < first) first = s; }
      }
    }
  }
  v.ctl[0] = 0; v.ctl[1] = flags; v.ctl[2] = first; v.ctl[3] = 0;
}

__global__ __launch_bounds__(256) void snapshot_unpack_sum_kernel(SnapshotView v, const char* __restrict__ blob) {
  const int s = blockIdx.y;
  const i64* c = ctl_of(v, s);
  const i64 off = c[1], len = c[2];
  if (off < 0) return;                                                           // only validated extents form an address
  const char* src = blob + off;
  const i64 units = (len + 15) >> 4;
  u64 acc = 0;
  for (i64 u = (i64)blockIdx.x * 256 + threadIdx.x; u < units; u += (i64)gridDim.x * 256) acc += unit_terms(load_unit(src, 16 * u, len, true), u, len);
  block_add(acc, v.sums, s);
}

__global__ __launch_bounds__(256) void snapshot_unpack_verify_kernel(SnapshotView v, const char* __restrict__ blob, i64* __restrict__ info) {
  __shared__ int sflags, sfirst;
  const int tid = threadIdx.x;
  if (tid == 0) { sflags = (int)v.ctl[1]; sfirst = (int)v.ctl[2]; }
  __syncthreads();
  if (tid < v.ns) {
    const i64* c = ctl_of(v, tid);
    if (c[1] >= 0 && (i64)v.sums[tid] != c[3]) { atomicOr(&sflags, SNAPSHOT_CHECKSUM); atomicMin(&sfirst, tid); }
  }
  for (int s = 0; s < v.ns; s++) {
    const SnapshotSection& S = v.sec[s];
    const i64* c = ctl_of(v, s);
    if (c[1] < 0) continue;
    if (S.kind == SNAPSHOT_MAP && S.rows_of == SNAPSHOT_ROWS_N1) {                // the map's offsets: rows = keyframes + 1 >= 1
      const i64* o = reinterpret_cast<const i64*>(blob + c[1]);
      const i64 n = c[0] - 1;
      int bad = 0;
      if (n < 0) bad |= SNAPSHOT_OFFSETS;
      for (i64 i = tid; i < n; i += 256) {
        const i64 a = o[i], b = o[i + 1];
        if (b < a) bad |= SNAPSHOT_OFFSETS;
        else if (b - a > v.max_cloud_points) bad |= SNAPSHOT_CAPACITY;           // a cloud the destination could not have stored
      }
      if (tid == 0 && n >= 0) {
        if (o[0] != 0) bad |= SNAPSHOT_OFFSETS;
        const i64* cx = ctl_of(v, v.part[S.part].first_section);                 // the part's first section holds the points
        if (cx[1] >= 0 && o[n] != cx[0]) bad |= SNAPSHOT_OFFSETS;                // offs[keyframes] is the saved point count (<= point_capacity)
      }
      if (bad) { atomicOr(&sflags, bad); atomicMin(&sfirst, s); }
    }
    if (S.kind == SNAPSHOT_SESSION) {                                            // the starts in the order begin can produce
      const int* st = reinterpret_cast<const int*>(blob + c[1]);
      const i64 n = c[0];
      int bad = 0;
      if (tid == 0 && (n < 1 || st[0] != 0)) bad = SNAPSHOT_SESSIONS;
      for (i64 q = 1 + tid; q < n; q += 256)
        if (st[q] <= st[q - 1]) bad = SNAPSHOT_SESSIONS;
      if (bad) { atomicOr(&sflags, bad); atomicMin(&sfirst, s); }
    }
  }
  __syncthreads();
  if (tid == 0) {
    const bool ok = sflags == 0;
    v.ctl[0] = ok ? 1 : 0; v.ctl[1] = sflags;
    info[0] = ok ? v.ns : 0; info[1] = sfirst == 0x7fffffff ? -1 : sfirst; info[2] = sflags; info[3] = 0;
  }
}

__global__ __launch_bounds__(256) void snapshot_unpack_scatter_kernel(SnapshotView v, const char* __restrict__ blob) {
  const int s = blockIdx.y;
  if (v.ctl[0] == 0) return;                                                     // a failed check: no byte of a destination changes
  const i64* c = ctl_of(v, s);
  const i64 off = c[1], len = c[2];
  const SnapshotSection& S = v.sec[s];
  const char* src = blob + off;
  char* dst = static_cast<char*>(S.base);
  const bool aligned16 = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const i64 units = (len + 15) >> 4;
  for (i64 u = (i64)blockIdx.x * 256 + threadIdx.x; u < units; u += (i64)gridDim.x * 256) {
    const i64 b = 16 * u;
    const uint4 q = load_unit(src, b, len, true);
    if (aligned16 && b + 16 <= len) *reinterpret_cast<uint4*>(dst + b) = q;
    else {                                                                       // rows at and above the saved count keep their bytes
      if (b < len) *reinterpret_cast<unsigned*>(dst + b) = q.x;
      if (b + 4 < len) *reinterpret_cast<unsigned*>(dst + b + 4) = q.y;
      if (b + 8 < len) *reinterpret_cast<unsigned*>(dst + b + 8) = q.z;
      if (b + 12 < len) *reinterpret_cast<unsigned*>(dst + b + 12) = q.w;
    }
  }
  const SnapshotPart& P = v.part[S.part];
  if (blockIdx.x == 0 && threadIdx.x == 0 && s == P.first_section) {             // the part's state words as saved
    const int* e = reinterpret_cast<const int*>(blob + SNAPSHOT_HEADER_BYTES + (i64)SNAPSHOT_ENTRY_BYTES * s + 64);
    P.state[0] = e[0]; P.state[1] = e[1]; P.state[2] = e[2]; P.state[3] = e[3];
  }
}

}  // namespace

void launch_snapshot_pack(hipStream_t st, const SnapshotView& v, void* blob, long long blob_capacity, long long* info) {
  char* b = static_cast<char*>(blob);
  snapshot_pack_plan_kernel<<<1, 64, 0, st>>>(v, blob_capacity);
  snapshot_pack_copy_kernel<<<dim3(v.grid_x, v.ns), 256, 0, st>>>(v, b);
  snapshot_pack_finish_kernel<<<1, 64, 0, st>>>(v, b, blob_capacity, info);
}

void launch_snapshot_unpack(hipStream_t st, const SnapshotView& v, const void* blob, long long blob_bytes, long long* info) {
  const char* b = static_cast<const char*>(blob);
  snapshot_unpack_header_kernel<<<1, 64, 0, st>>>(v, b, blob_bytes);
  snapshot_unpack_sum_kernel<<<dim3(v.grid_x, v.ns), 256, 0, st>>>(v, b);
  snapshot_unpack_verify_kernel<<<1, 256, 0, st>>>(v, b, info);
  snapshot_unpack_scatter_kernel<<<dim3(v.grid_x, v.ns), 256, 0, st>>>(v, b);
}

}  // namespace pr
