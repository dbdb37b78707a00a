// snapshot.hpp — what snapshot.hip (the kernels) and snapshot.cpp (the C ABI) of the state snapshot share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pr {

constexpr long long SNAPSHOT_MAGIC = 0x3150414E53415250LL;   // the bytes "PRASNAP1" in file order
constexpr int SNAPSHOT_VERSION = 1;
constexpr int SNAPSHOT_HEADER_BYTES = 64, SNAPSHOT_ENTRY_BYTES = 128;
constexpr int SNAPSHOT_MAX_SECTIONS = 17, SNAPSHOT_MAX_PARTS = 7;
constexpr int SNAPSHOT_MAP = 1, SNAPSHOT_ONLINE = 2, SNAPSHOT_ONLINESET = 3, SNAPSHOT_GRAPH = 4, SNAPSHOT_SESSION = 5;   // kinds
constexpr int SNAPSHOT_ROWS_N = 0, SNAPSHOT_ROWS_POINTS = 1, SNAPSHOT_ROWS_N1 = 2;      // which count of its part a section's rows are
constexpr int SNAPSHOT_OVERFLOW = 1, SNAPSHOT_BAD_MAGIC = 2, SNAPSHOT_BAD_VERSION = 4, SNAPSHOT_TRUNCATED = 8, SNAPSHOT_MISSING = 16,
              SNAPSHOT_CAPACITY = 32, SNAPSHOT_CHECKSUM = 64, SNAPSHOT_OFFSETS = 128, SNAPSHOT_SESSIONS = 256;   // = PR_SNAPSHOT_*
constexpr int SNAPSHOT_CTL_WORDS = 8 + 4 * SNAPSHOT_MAX_SECTIONS;     // ok, flags, first, total, 4 spare | rows, offset, length, sum of a section
constexpr int SNAPSHOT_GRID_MAX = 1024;                                // most workgroups over one section

inline long long snapshot_pad64(long long b) { return (b + 63) & ~63LL; }

// one section: one array of one part.  base is the caller's buffer; cap_rows the rows it has at the create capacity.
struct SnapshotSection {
  void* base;
  long long row_bytes, cap_rows;
  int kind, subtype, array, part, rows_of, pad;
};
// one part: its state words, its counts' clamps, and for the map the offsets its point count is read from
struct SnapshotPart {
  int* state;
  const long long* offs;            // the map's offs, else NULL
  long long caps[4];                // the capacities a snapshot records: the count's capacity first
  int count_min, first_section, sections, pad;
};
struct SnapshotView {
  int ns, np, grid_x, max_cloud_points;
  SnapshotSection sec[SNAPSHOT_MAX_SECTIONS];
  SnapshotPart part[SNAPSHOT_MAX_PARTS];
  unsigned long long* sums;         // [SNAPSHOT_MAX_SECTIONS]  the checksum partials, combined by integer atomic adds
  long long* ctl;                   // [SNAPSHOT_CTL_WORDS]
};

void launch_snapshot_pack(hipStream_t st, const SnapshotView& v, void* blob, long long blob_capacity, long long* info);
void launch_snapshot_unpack(hipStream_t st, const SnapshotView& v, const void* blob, long long blob_bytes, long long* info);

}  // namespace pr
