// snapshot.cpp — host side of the state snapshot (snapshot.hip): the opaque pr_snapshot over the caller's buffer records,
// its ONE allocation (control words, checksum partials, the info of the host forms), the argument checks, the two stream-ordered entry
// points, and the host forms that write and read a file.  The host forms alone take and free a staging blob; they are not capturable.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/place_recognition.h"
#include "handle_core.hpp"
#include "kernels.hpp"
#include "snapshot.hpp"

static_assert(pr::SNAPSHOT_OVERFLOW == PR_SNAPSHOT_OVERFLOW && pr::SNAPSHOT_BAD_MAGIC == PR_SNAPSHOT_BAD_MAGIC &&
              pr::SNAPSHOT_BAD_VERSION == PR_SNAPSHOT_BAD_VERSION && pr::SNAPSHOT_TRUNCATED == PR_SNAPSHOT_TRUNCATED &&
              pr::SNAPSHOT_MISSING == PR_SNAPSHOT_MISSING && pr::SNAPSHOT_CAPACITY == PR_SNAPSHOT_CAPACITY &&
              pr::SNAPSHOT_CHECKSUM == PR_SNAPSHOT_CHECKSUM && pr::SNAPSHOT_OFFSETS == PR_SNAPSHOT_OFFSETS &&
              pr::SNAPSHOT_SESSIONS == PR_SNAPSHOT_SESSIONS, "flag bits");
static_assert(pr::SNAPSHOT_MAP == PR_SNAPSHOT_MAP && pr::SNAPSHOT_ONLINE == PR_SNAPSHOT_ONLINE && pr::SNAPSHOT_ONLINESET == PR_SNAPSHOT_ONLINESET &&
              pr::SNAPSHOT_GRAPH == PR_SNAPSHOT_GRAPH && pr::SNAPSHOT_SESSION == PR_SNAPSHOT_SESSION, "section kinds");
static_assert(sizeof(pr_snapshot_desc) == 112, "pointers, int32 pairs and one int64, no padding");
static_assert(sizeof(pr::SnapshotView) <= 2048, "the view travels as a kernel argument");

struct pr_snapshot : pr::Handle {    // scratch: ctl | sums | the info of the host forms
  pr::SnapshotView v;
  long long* stage_info = nullptr;    // [4]
  long long bound = 0;
};

namespace {

using pr::fail;

constexpr int32_t MAX_KEYFRAMES = 1 << 20, MAX_SIGS = PR_MAX_SIGS, MAX_EDGES = 1 << 20, MAX_SESSIONS = 1024;
constexpr int64_t MAX_POINTS = (int64_t)1 << 38;

// the sections of a desc in blob order; returns 0 and leaves a text in `why` for a desc create refuses
struct Plan {
  pr::SnapshotView v;
  long long bound;
};

void add_part(pr::SnapshotView& v, int* state, const long long* offs, long long c0, long long c1, long long c2, int count_min) {
  pr::SnapshotPart& P = v.part[v.np];
  P.state = state; P.offs = offs; P.caps[0] = c0; P.caps[1] = c1; P.caps[2] = c2; P.caps[3] = 0;
  P.count_min = count_min; P.first_section = v.ns; P.sections = 0; P.pad = 0;
  v.np++;
}
void add_section(pr::SnapshotView& v, void* base, long long row_bytes, long long cap_rows, int kind, int subtype, int rows_of) {
  pr::SnapshotPart& P = v.part[v.np - 1];
  pr::SnapshotSection& S = v.sec[v.ns];
  S.base = base; S.row_bytes = row_bytes; S.cap_rows = cap_rows; S.kind = kind; S.subtype = subtype; S.array = P.sections;
  S.part = v.np - 1; S.rows_of = rows_of; S.pad = 0;
  P.sections++;
  v.ns++;
}

bool plan_of(const pr_snapshot_desc* d, Plan& pl, char* why, size_t why_len) {
  pr::SnapshotView& v = pl.v;
  memset(&v, 0, sizeof v);
  auto no = [&](const char* fmt, long long a, long long b) { snprintf(why, why_len, fmt, a, b); return false; };
  if (d->map) {
    const pr_map_buffers* m = d->map;
    if (!m->xyz || !m->inten || !m->offs || !m->frames || !m->poses || !m->ids || !m->state)
      return no("a buffer of the map is NULL (xyz, inten, offs, frames, poses, ids, state)", 0, 0);
    if (d->keyframe_capacity < 1 || d->keyframe_capacity > MAX_KEYFRAMES)
      return no("keyframe_capacity=%lld outside 1 .. %lld", d->keyframe_capacity, MAX_KEYFRAMES);
    if (d->point_capacity < 1 || d->point_capacity > MAX_POINTS) return no("point_capacity=%lld outside 1 .. 2^38", d->point_capacity, 0);
    if (d->max_cloud_points < 1 || d->max_cloud_points > d->point_capacity)
      return no("max_cloud_points=%lld outside 1 .. point_capacity=%lld", d->max_cloud_points, d->point_capacity);
    const long long kc = d->keyframe_capacity, pc = d->point_capacity;
    add_part(v, m->state, reinterpret_cast<const long long*>(m->offs), kc, pc, d->max_cloud_points, 0);
    add_section(v, m->xyz, 24, pc, PR_SNAPSHOT_MAP, 0, pr::SNAPSHOT_ROWS_POINTS);
    add_section(v, m->inten, 4, pc, PR_SNAPSHOT_MAP, 0, pr::SNAPSHOT_ROWS_POINTS);
    add_section(v, m->offs, 8, kc + 1, PR_SNAPSHOT_MAP, 0, pr::SNAPSHOT_ROWS_N1);
    add_section(v, m->frames, 128, kc, PR_SNAPSHOT_MAP, 0, pr::SNAPSHOT_ROWS_N);
    add_section(v, m->poses, 96, kc, PR_SNAPSHOT_MAP, 0, pr::SNAPSHOT_ROWS_N);
    add_section(v, m->ids, 4, kc, PR_SNAPSHOT_MAP, 0, pr::SNAPSHOT_ROWS_N);
    v.max_cloud_points = d->max_cloud_points;
  }
  for (int k = 0; k < 2; k++) {
    const pr_online_buffers* o = d->online[k];
    if (!o) continue;
    if (!o->sig || !o->state) return no("a buffer of online database %lld is NULL (sig, state)", k, 0);
    if (d->online_type[k] != PR_TYPE_SC && d->online_type[k] != PR_TYPE_M2DP)
      return no("online_type[%lld]=%lld is neither PR_TYPE_SC nor PR_TYPE_M2DP", k, d->online_type[k]);
    if (d->online_capacity[k] < 1 || d->online_capacity[k] > MAX_SIGS) return no("online_capacity[%lld]=%lld outside 1 .. PR_MAX_SIGS", k, d->online_capacity[k]);
    add_part(v, o->state, nullptr, d->online_capacity[k], 0, 0, 0);
    add_section(v, o->sig, d->online_type[k] == PR_TYPE_SC ? 2400 * 8 : 4 * 384 * 8, d->online_capacity[k], PR_SNAPSHOT_ONLINE, d->online_type[k],
                pr::SNAPSHOT_ROWS_N);
  }
  if (d->onlineset) {
    const pr_onlineset_buffers* o = d->onlineset;
    if (d->onlineset_kind != PR_ONLINESET_FUSED && d->onlineset_kind != PR_ONLINESET_DELIGHT)
      return no("onlineset_kind=%lld is neither PR_ONLINESET_FUSED nor PR_ONLINESET_DELIGHT", d->onlineset_kind, 0);
    const bool fused = d->onlineset_kind == PR_ONLINESET_FUSED;
    if (!o->state || (fused ? (!o->sc || !o->m2dp || o->delight) : (!o->delight || o->sc || o->m2dp)))
      return no("the online set's buffers do not fit its kind (fused: sc, m2dp, state; DELIGHT: delight, state)", 0, 0);
    if (d->onlineset_capacity < 1 || d->onlineset_capacity > MAX_SIGS) return no("onlineset_capacity=%lld outside 1 .. PR_MAX_SIGS", d->onlineset_capacity, 0);
    add_part(v, o->state, nullptr, d->onlineset_capacity, 0, 0, 0);
    if (fused) {
      add_section(v, o->sc, 2400 * 8, d->onlineset_capacity, PR_SNAPSHOT_ONLINESET, d->onlineset_kind, pr::SNAPSHOT_ROWS_N);
      add_section(v, o->m2dp, 4 * 384 * 8, d->onlineset_capacity, PR_SNAPSHOT_ONLINESET, d->onlineset_kind, pr::SNAPSHOT_ROWS_N);
    } else {
      add_section(v, o->delight, 16 * 256 * 8, d->onlineset_capacity, PR_SNAPSHOT_ONLINESET, d->onlineset_kind, pr::SNAPSHOT_ROWS_N);
    }
  }
  for (int k = 0; k < 2; k++) {
    const pr_posegraph_buffers* g = d->graph[k];
    if (!g) continue;
    if (!g->edge_ij || !g->edge_Z || !g->edge_w || !g->state) return no("a buffer of closure log %lld is NULL (edge_ij, edge_Z, edge_w, state)", k, 0);
    if (d->edge_capacity[k] < 1 || d->edge_capacity[k] > MAX_EDGES) return no("edge_capacity[%lld]=%lld outside 1 .. 2^20", k, d->edge_capacity[k]);
    add_part(v, g->state, nullptr, d->edge_capacity[k], 0, 0, 0);
    add_section(v, g->edge_ij, 8, d->edge_capacity[k], PR_SNAPSHOT_GRAPH, k, pr::SNAPSHOT_ROWS_N);
    add_section(v, g->edge_Z, 96, d->edge_capacity[k], PR_SNAPSHOT_GRAPH, k, pr::SNAPSHOT_ROWS_N);
    add_section(v, g->edge_w, 16, d->edge_capacity[k], PR_SNAPSHOT_GRAPH, k, pr::SNAPSHOT_ROWS_N);
  }
  if (d->sessions) {
    if (!d->sessions->start || !d->sessions->state) return no("a buffer of the session table is NULL (start, state)", 0, 0);
    if (d->session_capacity < 1 || d->session_capacity > MAX_SESSIONS) return no("session_capacity=%lld outside 1 .. %lld", d->session_capacity, MAX_SESSIONS);
    add_part(v, d->sessions->state, nullptr, d->session_capacity, 0, 0, 1);
    add_section(v, d->sessions->start, 4, d->session_capacity, PR_SNAPSHOT_SESSION, 0, pr::SNAPSHOT_ROWS_N);
  }
  if (v.ns == 0) return no("the desc names no part", 0, 0);
  long long bound = pr::SNAPSHOT_HEADER_BYTES + (long long)pr::SNAPSHOT_ENTRY_BYTES * v.ns, widest = 0;
  for (int s = 0; s < v.ns; s++) {
    const long long b = pr::snapshot_pad64(v.sec[s].cap_rows * v.sec[s].row_bytes);
    bound += b;
    if (b > widest) widest = b;
  }
  const long long wg = (widest / 16 + 255) / 256;                   // a lane per 16 bytes of the widest section, grid-strided above the cap
  v.grid_x = (int)(wg < 1 ? 1 : (wg > pr::SNAPSHOT_GRID_MAX ? pr::SNAPSHOT_GRID_MAX : wg));
  pl.bound = bound;
  return true;
}

// what both forms check of a blob before any device is touched; `who` names the entry point
int blob_check(const char* who, pr_snapshot* s, const void* blob, long long bytes, const void* info) {
  pr_ctx* ctx = s ? s->ctx : nullptr;
  if (!blob) return fail(ctx, PR_EINVAL, "%s: the blob is NULL", who);
  if (!info) return fail(ctx, PR_EINVAL, "%s: info is NULL", who);
  if (bytes < 0) return fail(ctx, PR_EINVAL, "%s: a negative blob size", who);
  if (reinterpret_cast<uintptr_t>(blob) & 15) return fail(ctx, PR_EINVAL, "%s: the blob must lie on a 16-byte boundary", who);
  if (!s) return fail(nullptr, PR_EINVAL, "%s: snapshot is NULL", who);
  return PR_OK;
}

}  // namespace

extern "C" {

int pr_snapshot_create(pr_ctx* ctx, const pr_snapshot_desc* desc, pr_snapshot** out) {
  // the value checks come first and need no device: with ctx == NULL their text goes to pr_last_error(NULL)
  if (!out) return fail(ctx, PR_EINVAL, "pr_snapshot_create: out is NULL");
  *out = nullptr;
  if (!desc) return fail(ctx, PR_EINVAL, "pr_snapshot_create: desc is NULL");
  Plan pl;
  char why[256];
  if (!plan_of(desc, pl, why, sizeof why)) return fail(ctx, PR_EINVAL, "pr_snapshot_create: %s", why);
  if (!ctx) return fail(nullptr, PR_EINVAL, "pr_snapshot_create: ctx is NULL");
  const size_t words = pr::SNAPSHOT_CTL_WORDS + pr::SNAPSHOT_MAX_SECTIONS + 4;
  pr::Owned<pr_snapshot> s;
  if (int rc = pr::make(ctx, "pr_snapshot_create", 8 * words, s)) return rc;
  s->v = pl.v;
  s->bound = pl.bound;
  long long* w = static_cast<long long*>(s->scratch);
  s->v.ctl = w;
  s->v.sums = reinterpret_cast<unsigned long long*>(w + pr::SNAPSHOT_CTL_WORDS);
  s->stage_info = w + pr::SNAPSHOT_CTL_WORDS + pr::SNAPSHOT_MAX_SECTIONS;
  pr::Transfer t(ctx);
  t.fill(s->scratch, 0, 8 * words);
  return pr::commit(s, t, "pr_snapshot_create", out);
}

void pr_snapshot_destroy(pr_snapshot* s) { pr::destroy(s); }    // the buffers are the caller's

int pr_snapshot_desc_bound(const pr_snapshot_desc* desc, int64_t* bytes) {
  if (!bytes) return fail(nullptr, PR_EINVAL, "pr_snapshot_desc_bound: bytes is NULL");
  *bytes = 0;
  if (!desc) return fail(nullptr, PR_EINVAL, "pr_snapshot_desc_bound: desc is NULL");
  Plan pl;
  char why[256];
  if (!plan_of(desc, pl, why, sizeof why)) return fail(nullptr, PR_EINVAL, "pr_snapshot_desc_bound: %s", why);
  *bytes = pl.bound;
  return PR_OK;
}

int pr_snapshot_bound(pr_snapshot* s, int64_t* bytes) {
  if (!bytes) return fail(s ? s->ctx : nullptr, PR_EINVAL, "pr_snapshot_bound: bytes is NULL");
  if (!s) return fail(nullptr, PR_EINVAL, "pr_snapshot_bound: snapshot is NULL");
  *bytes = s->bound;
  return PR_OK;
}

int pr_snapshot_pack_dev(pr_snapshot* s, void* d_blob, int64_t blob_capacity, int64_t* d_info) {
  if (int rc = blob_check("pr_snapshot_pack_dev", s, d_blob, blob_capacity, d_info)) return rc;
  PR_CHECK_HIP(s->ctx, hipSetDevice(pr::ctx_device(s->ctx)));
  pr::launch_snapshot_pack(pr::ctx_stream(s->ctx), s->v, d_blob, blob_capacity, reinterpret_cast<long long*>(d_info));
  PR_CHECK_HIP(s->ctx, hipGetLastError());
  return PR_OK;
}

int pr_snapshot_unpack_dev(pr_snapshot* s, const void* d_blob, int64_t blob_bytes, int64_t* d_info) {
  if (int rc = blob_check("pr_snapshot_unpack_dev", s, d_blob, blob_bytes, d_info)) return rc;
  PR_CHECK_HIP(s->ctx, hipSetDevice(pr::ctx_device(s->ctx)));
  pr::launch_snapshot_unpack(pr::ctx_stream(s->ctx), s->v, d_blob, blob_bytes, reinterpret_cast<long long*>(d_info));
  PR_CHECK_HIP(s->ctx, hipGetLastError());
  return PR_OK;
}

int pr_snapshot_save(pr_snapshot* s, const char* path) {
  pr_ctx* ctx = s ? s->ctx : nullptr;
  if (!path || !path[0]) return fail(ctx, PR_EINVAL, "pr_snapshot_save: path is NULL or empty");
  if (!s) return fail(nullptr, PR_EINVAL, "pr_snapshot_save: snapshot is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  void* d_stage = nullptr;
  PR_CHECK_HIP(ctx, hipMalloc(&d_stage, (size_t)s->bound));
  long long info[4] = {0, 0, 0, 0};
  pr::Transfer t(ctx);
  t.run([&] { return pr_snapshot_pack_dev(s, d_stage, s->bound, reinterpret_cast<int64_t*>(s->stage_info)); });
  t.down(info, s->stage_info, sizeof info);
  int rc = t.finish(ctx, "pr_snapshot_save");                    // the one synchronising read of info
  char* host = nullptr;
  if (rc == PR_OK && (info[2] != 0 || info[0] < pr::SNAPSHOT_HEADER_BYTES || info[0] > s->bound))
    rc = fail(ctx, PR_EHIP, "pr_snapshot_save: the pack reported %lld bytes, flags %lld", info[0], info[2]);
  if (rc == PR_OK) {
    host = static_cast<char*>(malloc((size_t)info[0]));
    if (!host) rc = fail(ctx, PR_ENOMEM, "out of host memory");
  }
  if (rc == PR_OK) {
    const hipError_t e = hipMemcpy(host, d_stage, (size_t)info[0], hipMemcpyDeviceToHost);      // exactly the bytes written
    if (e != hipSuccess) rc = fail(ctx, pr::hip_code(e), "pr_snapshot_save: %s", hipGetErrorString(e));
  }
  (void)hipFree(d_stage);
  if (rc == PR_OK) {
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) rc = fail(ctx, PR_EIO, "pr_snapshot_save: cannot open %s for writing", tmp.c_str());
    else {
      const bool wrote = fwrite(host, 1, (size_t)info[0], f) == (size_t)info[0];
      const bool closed = fclose(f) == 0;
      if (!wrote || !closed) { remove(tmp.c_str()); rc = fail(ctx, PR_EIO, "pr_snapshot_save: writing %s failed", tmp.c_str()); }
      else if (rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); rc = fail(ctx, PR_EIO, "pr_snapshot_save: cannot rename %s to %s", tmp.c_str(), path); }
    }
  }
  free(host);
  return rc;
}

int pr_snapshot_load(pr_snapshot* s, const char* path, int64_t* info) {
  pr_ctx* ctx = s ? s->ctx : nullptr;
  if (!path || !path[0]) return fail(ctx, PR_EINVAL, "pr_snapshot_load: path is NULL or empty");
  if (!info) return fail(ctx, PR_EINVAL, "pr_snapshot_load: info is NULL");
  // the file is read and its table checked on the host: none of these refusals touches a device
  FILE* f = fopen(path, "rb");
  if (!f) return fail(ctx, PR_EIO, "pr_snapshot_load: cannot open %s", path);
  long long size = -1;
  if (fseek(f, 0, SEEK_END) == 0) size = ftell(f);
  if (size < 0 || fseek(f, 0, SEEK_SET) != 0) { fclose(f); return fail(ctx, PR_EIO, "pr_snapshot_load: cannot size %s", path); }
  if (size < pr::SNAPSHOT_HEADER_BYTES) { fclose(f); return fail(ctx, PR_EINVAL, "pr_snapshot_load: %s is shorter than a header (%lld bytes)", path, size); }
  char* host = static_cast<char*>(malloc((size_t)size));
  if (!host) { fclose(f); return fail(ctx, PR_ENOMEM, "out of host memory"); }
  const bool got = fread(host, 1, (size_t)size, f) == (size_t)size;
  fclose(f);
  int rc = PR_OK;
  if (!got) rc = fail(ctx, PR_EIO, "pr_snapshot_load: reading %s failed", path);
  if (rc == PR_OK) {
    long long h[8];
    memcpy(h, host, sizeof h);
    const long long nsec = h[2];
    if (nsec < 0 || nsec > pr::SNAPSHOT_MAX_SECTIONS || pr::SNAPSHOT_HEADER_BYTES + pr::SNAPSHOT_ENTRY_BYTES * nsec > size)
      rc = fail(ctx, PR_EINVAL, "pr_snapshot_load: %s is cut inside its header (%lld sections in %lld bytes)", path, nsec, size);
    for (long long k = 0; rc == PR_OK && k < nsec; k++) {
      long long e[16];
      memcpy(e, host + pr::SNAPSHOT_HEADER_BYTES + pr::SNAPSHOT_ENTRY_BYTES * k, sizeof e);
      if (e[5] < 0 || e[6] < 0 || e[5] > size || e[6] > size - e[5])
        rc = fail(ctx, PR_EINVAL, "pr_snapshot_load: section %lld of %s points outside the file", k, path);
    }
  }
  if (rc == PR_OK && !s) rc = fail(nullptr, PR_EINVAL, "pr_snapshot_load: snapshot is NULL");
  void* d_stage = nullptr;
  if (rc == PR_OK) {
    hipError_t e = hipSetDevice(pr::ctx_device(ctx));
    if (e == hipSuccess) e = hipMalloc(&d_stage, (size_t)size);
    if (e == hipSuccess) e = hipMemcpy(d_stage, host, (size_t)size, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(ctx, pr::hip_code(e), "pr_snapshot_load: staging %lld bytes: %s", size, hipGetErrorString(e));
  }
  if (rc == PR_OK) {
    pr::Transfer t(ctx);
    t.run([&] { return pr_snapshot_unpack_dev(s, d_stage, size, reinterpret_cast<int64_t*>(s->stage_info)); });
    t.down(info, s->stage_info, 4 * sizeof(int64_t));
    rc = t.finish(ctx, "pr_snapshot_load");
  }
  if (d_stage) { if (s) (void)hipStreamSynchronize(pr::ctx_stream(ctx)); (void)hipFree(d_stage); }
  free(host);
  return rc;
}

}  // extern "C"
