// bow.cpp — host side of BoW generation: the DBoW2 vocabulary (TemplatedVocabulary.h:1338-1424 loadFromTextFile, a binary side-car,
// creation from arrays), its BFS device layout uploaded once per context, the grow-only scratch, and the pr_bow_* entry points.  The
// kernels are in bow_gen.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/place_recognition.h"
#include "host_common.hpp"
#include "kernels.hpp"

namespace pr {
void host_set_error(const std::string& msg);     // host_io.cpp
}

struct pr_bow_vocab {
  int32_t k = 0, L = 0, scoring = 0, weighting = 0;
  int64_t n_words = 0;
  uint64_t serial = 0;                           // identifies the vocabulary in the contexts' device caches (never reused)
  std::vector<int32_t> parent;                   // [n] node arrays, node 0 = root
  std::vector<uint8_t> is_leaf;
  std::vector<uint8_t> desc;                     // [n][32]
  std::vector<double> weight;
  std::vector<int32_t> word;                     // word id of a leaf-flagged node, 0 otherwise (Node(): word_id(0))
};

namespace {

std::atomic<uint64_t> g_serial{1};
constexpr char BIN_MAGIC[8] = {'P', 'R', 'B', 'O', 'W', '1', 0, 0};

int herr(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int herr(int code, const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  pr::host_set_error(b);
  return code;
}

using pr::fail;

int check_header(int32_t k, int32_t L, int32_t scoring, int32_t weighting) {   // :1360-1364
  if (k < 0 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3)
    return herr(PR_EINVAL, "BoW vocabulary: header k=%d L=%d scoring=%d weighting=%d outside 0 <= k <= 20, 1 <= L <= 10, scoring 0..5, "
                "weighting 0..3", k, L, scoring, weighting);
  return PR_OK;
}

// word ids in node order for the leaf-flagged nodes (:1407-1414)
void assign_words(pr_bow_vocab* v) {
  const int64_t n = (int64_t)v->parent.size();
  v->word.assign(n, 0);
  v->n_words = 0;
  for (int64_t i = 1; i < n; i++)
    if (v->is_leaf[i]) v->word[i] = (int32_t)v->n_words++;
}

pr_bow_vocab* new_vocab(int32_t k, int32_t L, int32_t scoring, int32_t weighting, int64_t n) {
  pr_bow_vocab* v = new pr_bow_vocab;
  v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting;
  v->serial = g_serial.fetch_add(1);
  v->parent.assign(n, -1);
  v->is_leaf.assign(n, 0);
  v->desc.assign((size_t)n * 32, 0);
  v->weight.assign(n, 0.0);
  return v;
}

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// one whitespace-separated token of [p, e): returns false at the end of the line
bool next_token(const char*& p, const char* e, const char*& t0, const char*& t1) {
  while (p < e && is_space(*p)) p++;
  if (p == e) return false;
  t0 = p;
  while (p < e && !is_space(*p)) p++;
  t1 = p;
  return true;
}

bool parse_int(const char* t0, const char* t1, long long& out) {   // istream >> int: optional sign, decimal digits
  if (t0 < t1 && *t0 == '+') t0++;
  auto r = std::from_chars(t0, t1, out);
  return r.ec == std::errc() && r.ptr == t1;
}

// istream >> double is strtod's correctly rounded conversion; tokens strtod would read but istream would not (hex, inf, nan) are refused
bool parse_double(const char* t0, const char* t1, double& out) {
  for (const char* c = t0; c < t1; c++)
    if (!((*c >= '0' && *c <= '9') || *c == '.' || *c == 'e' || *c == 'E' || *c == '+' || *c == '-')) return false;
  char buf[128];
  const size_t len = (size_t)(t1 - t0);
  if (len == 0 || len >= sizeof buf) return false;
  memcpy(buf, t0, len);
  buf[len] = 0;
  char* end = nullptr;
  errno = 0;
  out = strtod(buf, &end);
  return end == buf + len && std::isfinite(out);
}

int load_text(const char* path, const std::string& data, pr_bow_vocab** out) {
  const char* p = data.data();
  const char* const end = p + data.size();
  const char* eol = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
  if (!eol) eol = end;
  long long h[4];
  const char *t0, *t1;
  const char* q = p;
  for (int i = 0; i < 4; i++)
    if (!next_token(q, eol, t0, t1) || !parse_int(t0, t1, h[i]))
      return herr(PR_EINVAL, "%s: line 1: expected the header `k L scoring weighting`", path);
  for (long long x : h)
    if (x < -(1LL << 31) || x >= (1LL << 31)) return herr(PR_EINVAL, "%s: line 1: header value out of range", path);
  if (int rc = check_header((int32_t)h[0], (int32_t)h[1], (int32_t)h[2], (int32_t)h[3])) return rc;
  // count the node lines first (non-empty ones) so that the arrays are sized once
  int64_t lines = 0;
  for (const char* s = eol; s < end;) {
    const char* s0 = s + 1;
    const char* e = s0 < end ? static_cast<const char*>(memchr(s0, '\n', (size_t)(end - s0))) : nullptr;
    if (!e) e = end;
    const char* c = s0;
    while (c < e && is_space(*c)) c++;
    if (c < e) lines++;
    s = e;
  }
  if (lines >= (1LL << 31) - 1) return herr(PR_EINVAL, "%s: too many nodes (%lld)", path, (long long)lines);
  pr_bow_vocab* v = new_vocab((int32_t)h[0], (int32_t)h[1], (int32_t)h[2], (int32_t)h[3], lines + 1);
  int64_t nid = 1;
  long long lineno = 1;
  for (const char* s = eol; s < end;) {
    const char* s0 = s + 1;
    lineno++;
    const char* e = s0 < end ? static_cast<const char*>(memchr(s0, '\n', (size_t)(end - s0))) : nullptr;
    if (!e) e = end;
    s = e;
    const char* c = s0;
    if (!next_token(c, e, t0, t1)) continue;   // an empty line: skipped (the reference would append a node with undefined bytes)
    c = s0;
    const char* tok[35][2];
    int got = 0;
    while (got < 35 && next_token(c, e, tok[got][0], tok[got][1])) got++;
    if (got < 35) {
      delete v;
      return herr(PR_EINVAL, "%s: line %lld: %d tokens, a node line holds 35 (parent isLeaf 32 bytes weight)", path, lineno, got);
    }
    long long vals[34];
    double w = 0.0;
    for (int i = 0; i < 35; i++)
      if (!(i < 34 ? parse_int(tok[i][0], tok[i][1], vals[i]) : parse_double(tok[i][0], tok[i][1], w))) {
        delete v;
        return herr(PR_EINVAL, "%s: line %lld: token %d `%.*s` is not a number", path, lineno, i + 1,
                    (int)std::min<ptrdiff_t>(tok[i][1] - tok[i][0], 40), tok[i][0]);
      }
    if (vals[0] < 0 || vals[0] >= nid) {
      delete v;
      return herr(PR_EINVAL, "%s: line %lld: parent %lld of node %lld is not an earlier node", path, lineno, vals[0], (long long)nid);
    }
    v->parent[nid] = (int32_t)vals[0];
    v->is_leaf[nid] = vals[1] > 0;
    for (int b = 0; b < 32; b++) v->desc[(size_t)nid * 32 + b] = (uint8_t)vals[2 + b];   // (unsigned char)n (FORB.cpp:120-131)
    v->weight[nid] = w;
    nid++;
  }
  assign_words(v);
  *out = v;
  return PR_OK;
}

struct BinHeader {
  char magic[8];
  int32_t k, L, scoring, weighting;
  int64_t n_nodes;
};

int check_nodes(const char* where, int64_t n, const int32_t* parent) {
  for (int64_t i = 1; i < n; i++)
    if (parent[i] < 0 || parent[i] >= i)
      return herr(PR_EINVAL, "%s: parent %d of node %lld is not an earlier node", where, parent[i], (long long)i);
  return PR_OK;
}

int load_bin(const char* path, const std::string& data, pr_bow_vocab** out) {
  BinHeader h;
  if (data.size() < sizeof h) return herr(PR_EIO, "%s: truncated PRBOW1 header", path);
  memcpy(&h, data.data(), sizeof h);
  if (int rc = check_header(h.k, h.L, h.scoring, h.weighting)) return rc;
  const int64_t n = h.n_nodes;
  if (n < 1 || n >= (1LL << 31)) return herr(PR_EINVAL, "%s: node count %lld", path, (long long)n);
  const size_t need = sizeof h + (size_t)n * (4 + 1 + 32 + 8);
  if (data.size() != need) return herr(PR_EIO, "%s: %zu bytes, a PRBOW1 file of %lld nodes has %zu", path, data.size(), (long long)n, need);
  pr_bow_vocab* v = new_vocab(h.k, h.L, h.scoring, h.weighting, n);
  const char* p = data.data() + sizeof h;
  memcpy(v->parent.data(), p, (size_t)n * 4); p += (size_t)n * 4;
  memcpy(v->is_leaf.data(), p, (size_t)n); p += n;
  memcpy(v->desc.data(), p, (size_t)n * 32); p += (size_t)n * 32;
  memcpy(v->weight.data(), p, (size_t)n * 8);
  v->parent[0] = -1;
  if (int rc = check_nodes(path, n, v->parent.data())) { delete v; return rc; }
  for (int64_t i = 0; i < n; i++) v->is_leaf[i] = i > 0 && v->is_leaf[i];
  assign_words(v);
  *out = v;
  return PR_OK;
}

// ------------------------------------------------------------------------------------------------------ device side
struct DevVocab {
  uint64_t serial = 0;
  int32_t n_words = 0;
  uint4* desc = nullptr;                         // [n][2] BFS order
  int2* child = nullptr;                         // [n] (first child, child count), BFS indices
  int* word = nullptr;                           // [n]
  double* weight = nullptr;                      // [n]
};

struct BowState {
  std::vector<DevVocab> vocabs;                  // one per vocabulary used on this context, kept until the context is destroyed
  int lanes = 4;                                 // lanes per descriptor of the descent (PR_BOW_LANES = 1, 2, 4, 8 or 16: experiments)
  int* node = nullptr;                           // [cap] scratch, grow-only
  double* wgt = nullptr;
  double* vals = nullptr;
  unsigned long long* gkeys = nullptr;           // [2 cap]
  int64_t cap = 0;
};

void free_scratch(BowState* st) {
  if (st->node) (void)hipFree(st->node);
  if (st->wgt) (void)hipFree(st->wgt);
  if (st->vals) (void)hipFree(st->vals);
  if (st->gkeys) (void)hipFree(st->gkeys);
  st->node = nullptr; st->wgt = nullptr; st->vals = nullptr; st->gkeys = nullptr;
  st->cap = 0;
}

BowState* state(pr_ctx* ctx) {
  void*& slot = pr::ctx_bow(ctx);
  if (!slot) {
    BowState* st = new BowState;
    if (const char* e = getenv("PR_BOW_LANES")) {
      const int g = atoi(e);
      if (g == 1 || g == 2 || g == 4 || g == 8 || g == 16) st->lanes = g;
    }
    slot = st;
  }
  return static_cast<BowState*>(slot);
}

// The vocabulary in BFS order (root first, each node's children contiguous in file order), uploaded on first use on this context (waits
// for the upload); recorded in the state only after the upload completed.
int device_vocab(pr_ctx* ctx, BowState* st, const pr_bow_vocab* v, const DevVocab** out) {
  for (const DevVocab& d : st->vocabs)
    if (d.serial == v->serial) { *out = &d; return PR_OK; }
  const int64_t n = (int64_t)v->parent.size();
  std::vector<int64_t> cstart(n + 1, 0);        // children of each node id, in file (= id) order
  for (int64_t i = 1; i < n; i++) cstart[v->parent[i] + 1]++;
  for (int64_t i = 0; i < n; i++) cstart[i + 1] += cstart[i];
  std::vector<int32_t> kids(n > 0 ? n - 1 : 0);
  {
    std::vector<int64_t> fill(cstart.begin(), cstart.end() - 1);
    for (int64_t i = 1; i < n; i++) kids[fill[v->parent[i]]++] = (int32_t)i;
  }
  std::vector<int32_t> order;                    // BFS position -> node id
  order.reserve(n);
  order.push_back(0);
  std::vector<int2> child(n);
  for (size_t b = 0; b < order.size(); b++) {
    const int32_t id = order[b];
    const int64_t c0 = cstart[id], c1 = cstart[id + 1];
    child[b] = make_int2((int)order.size(), (int)(c1 - c0));
    for (int64_t c = c0; c < c1; c++) order.push_back(kids[c]);
  }
  std::vector<uint8_t> desc((size_t)n * 32);
  std::vector<int> word(n);
  std::vector<double> weight(n);
  for (int64_t b = 0; b < n; b++) {
    const int32_t id = order[b];
    memcpy(&desc[(size_t)b * 32], &v->desc[(size_t)id * 32], 32);
    word[b] = v->word[id];
    weight[b] = v->weight[id];
  }
  hipStream_t s = pr::ctx_stream(ctx);
  DevVocab d;
  d.serial = v->serial;
  d.n_words = (int32_t)v->n_words;
  hipError_t e = hipMalloc(&d.desc, desc.size());
  if (e == hipSuccess) e = hipMalloc(&d.child, (size_t)n * sizeof(int2));
  if (e == hipSuccess) e = hipMalloc(&d.word, (size_t)n * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&d.weight, (size_t)n * sizeof(double));
  if (e == hipSuccess) e = hipMemcpyAsync(d.desc, desc.data(), desc.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d.child, child.data(), (size_t)n * sizeof(int2), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d.word, word.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d.weight, weight.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    if (d.desc) (void)hipFree(d.desc);
    if (d.child) (void)hipFree(d.child);
    if (d.word) (void)hipFree(d.word);
    if (d.weight) (void)hipFree(d.weight);
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "BoW vocabulary upload failed: %s", hipGetErrorString(e));
  }
  st->vocabs.push_back(d);
  *out = &st->vocabs.back();
  return PR_OK;
}

int check_args(pr_ctx* ctx, const char* fn, const pr_bow_vocab* vocab, const void* desc, const int64_t* offs, int32_t N, int32_t cols,
               const double* out) {
  if (!ctx) return fail(ctx, PR_EINVAL, "%s: ctx is NULL", fn);
  if (!vocab) return fail(ctx, PR_EINVAL, "%s: vocab is NULL", fn);
  if (N < 0) return fail(ctx, PR_EINVAL, "%s: N = %d", fn, N);
  if (cols < 1) return fail(ctx, PR_EINVAL, "%s: cols = %d (at least 1)", fn, cols);
  if (N > 0 && (!offs || !out)) return fail(ctx, PR_EINVAL, "%s: offs / out is NULL", fn);
  (void)desc;
  return PR_OK;
}

}  // namespace

namespace pr {
void bow_release(void* p) {
  BowState* st = static_cast<BowState*>(p);
  if (!st) return;
  for (DevVocab& d : st->vocabs) {
    (void)hipFree(d.desc);
    (void)hipFree(d.child);
    (void)hipFree(d.word);
    (void)hipFree(d.weight);
  }
  free_scratch(st);
  delete st;
}
}  // namespace pr

extern "C" {

int pr_bow_vocab_load(const char* path, pr_bow_vocab** out) {
  if (!path || !out) return herr(PR_EINVAL, "pr_bow_vocab_load: path / out is NULL");
  *out = nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) return herr(PR_EIO, "cannot open %s", path);
  std::string data;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.append(buf, got);
  const bool bad = ferror(f);
  fclose(f);
  if (bad) return herr(PR_EIO, "cannot read %s", path);
  try {
    if (data.size() >= 8 && memcmp(data.data(), BIN_MAGIC, 8) == 0) return load_bin(path, data, out);
    return load_text(path, data, out);
  } catch (const std::bad_alloc&) {
    return herr(PR_ENOMEM, "%s: out of host memory", path);
  }
}

int pr_bow_vocab_save_bin(const pr_bow_vocab* v, const char* path) {
  if (!v || !path) return herr(PR_EINVAL, "pr_bow_vocab_save_bin: vocab / path is NULL");
  FILE* f = fopen(path, "wb");
  if (!f) return herr(PR_EIO, "cannot open %s for writing", path);
  BinHeader h;
  memcpy(h.magic, BIN_MAGIC, 8);
  h.k = v->k; h.L = v->L; h.scoring = v->scoring; h.weighting = v->weighting;
  h.n_nodes = (int64_t)v->parent.size();
  const size_t n = v->parent.size();
  bool ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(v->parent.data(), 4, n, f) == n && fwrite(v->is_leaf.data(), 1, n, f) == n &&
            fwrite(v->desc.data(), 32, n, f) == n && fwrite(v->weight.data(), 8, n, f) == n;
  ok = (fclose(f) == 0) && ok;
  return ok ? PR_OK : herr(PR_EIO, "cannot write %s", path);
}

int pr_bow_vocab_create(int32_t k, int32_t L, int32_t scoring, int32_t weighting, int64_t n_nodes, const int32_t* parent,
                        const uint8_t* is_leaf, const uint8_t* desc, const double* weight, pr_bow_vocab** out) {
  if (!out) return herr(PR_EINVAL, "pr_bow_vocab_create: out is NULL");
  *out = nullptr;
  if (int rc = check_header(k, L, scoring, weighting)) return rc;
  if (n_nodes < 1 || n_nodes >= (1LL << 31)) return herr(PR_EINVAL, "pr_bow_vocab_create: n_nodes = %lld (the root included)", (long long)n_nodes);
  if (n_nodes > 1 && (!parent || !is_leaf || !desc || !weight)) return herr(PR_EINVAL, "pr_bow_vocab_create: a node array is NULL");
  if (n_nodes > 1)
    if (int rc = check_nodes("pr_bow_vocab_create", n_nodes, parent)) return rc;
  pr_bow_vocab* v;
  try {
    v = new_vocab(k, L, scoring, weighting, n_nodes);
  } catch (const std::bad_alloc&) {
    return herr(PR_ENOMEM, "pr_bow_vocab_create: out of host memory");
  }
  for (int64_t i = 1; i < n_nodes; i++) {
    v->parent[i] = parent[i];
    v->is_leaf[i] = is_leaf[i] > 0;
    memcpy(&v->desc[(size_t)i * 32], desc + (size_t)i * 32, 32);
    v->weight[i] = weight[i];
  }
  assign_words(v);
  *out = v;
  return PR_OK;
}

int pr_bow_vocab_info(const pr_bow_vocab* v, int32_t* info, int64_t* n_nodes, int64_t* n_words) {
  if (!v) return herr(PR_EINVAL, "pr_bow_vocab_info: vocab is NULL");
  if (info) { info[0] = v->k; info[1] = v->L; info[2] = v->scoring; info[3] = v->weighting; }
  if (n_nodes) *n_nodes = (int64_t)v->parent.size();
  if (n_words) *n_words = v->n_words;
  return PR_OK;
}

int pr_bow_vocab_export(const pr_bow_vocab* v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight) {
  if (!v) return herr(PR_EINVAL, "pr_bow_vocab_export: vocab is NULL");
  const size_t n = v->parent.size();
  if (parent) memcpy(parent, v->parent.data(), n * 4);
  if (is_leaf) memcpy(is_leaf, v->is_leaf.data(), n);
  if (desc) memcpy(desc, v->desc.data(), n * 32);
  if (weight) memcpy(weight, v->weight.data(), n * 8);
  return PR_OK;
}

void pr_bow_vocab_destroy(pr_bow_vocab* v) { delete v; }

}  // extern "C"

namespace {

// the device form; flag: the device word set when a row has more than cols words
int generate_dev(pr_ctx* ctx, const pr_bow_vocab* vocab, const uint8_t* desc, int64_t n_desc, const int64_t* offs, int32_t N, int32_t cols,
                 double* out, int32_t* n_words, int32_t* feat_words, int* flag) {
  if (n_desc < 0 || n_desc >= (1LL << 31)) return fail(ctx, PR_EINVAL, "pr_bow_generate_dev: n_desc = %lld", (long long)n_desc);
  if (n_desc > 0 && !desc) return fail(ctx, PR_EINVAL, "pr_bow_generate_dev: desc is NULL");
  if (reinterpret_cast<uintptr_t>(desc) % 16) return fail(ctx, PR_EINVAL, "pr_bow_generate_dev: desc must be 16-byte aligned");
  if (N == 0 && n_desc == 0) return PR_OK;
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  BowState* st = state(ctx);
  hipStream_t s = pr::ctx_stream(ctx);
  if (vocab->n_words == 0) {                     // transform returns an empty vector at once (:1135-1138)
    if (feat_words) pr::launch_bow_fill_words(s, feat_words, n_desc, -1);
    pr::launch_bow_aggregate(s, offs, N, n_desc, nullptr, nullptr, nullptr, vocab->weighting, vocab->scoring, cols, nullptr, nullptr,
                             nullptr, out, n_words, flag);
    PR_CHECK_HIP(ctx, hipGetLastError());
    return PR_OK;
  }
  const DevVocab* dv = nullptr;
  if (int rc = device_vocab(ctx, st, vocab, &dv)) return rc;
  if (n_desc > st->cap) {                        // grow-only: a later call of at most this size allocates nothing
    if (st->node) {
      PR_CHECK_HIP(ctx, hipStreamSynchronize(s));
      free_scratch(st);
    }
    hipError_t e = hipMalloc(&st->node, (size_t)n_desc * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&st->wgt, (size_t)n_desc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&st->vals, (size_t)n_desc * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&st->gkeys, (size_t)n_desc * 2 * sizeof(unsigned long long));
    if (e != hipSuccess) {
      free_scratch(st);
      return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_bow_generate_dev: scratch: %s", hipGetErrorString(e));
    }
    st->cap = n_desc;
  }
  pr::launch_bow_descend(s, desc, n_desc, dv->desc, dv->child, dv->word, st->lanes, st->node, feat_words);
  pr::launch_bow_aggregate(s, offs, N, n_desc, st->node, dv->word, dv->weight, vocab->weighting, vocab->scoring, cols, st->wgt, st->vals,
                           st->gkeys, out, n_words, flag);
  PR_CHECK_HIP(ctx, hipGetLastError());
  return PR_OK;
}

}  // namespace

extern "C" {

int pr_bow_generate_dev(pr_ctx* ctx, const pr_bow_vocab* vocab, const uint8_t* desc, int64_t n_desc, const int64_t* offs, int32_t N,
                        int32_t cols, double* out, int32_t* n_words, int32_t* feat_words) {
  if (int rc = check_args(ctx, "pr_bow_generate_dev", vocab, desc, offs, N, cols, out)) return rc;
  return generate_dev(ctx, vocab, desc, n_desc, offs, N, cols, out, n_words, feat_words, pr::ctx_bow_flag(ctx));
}

int pr_bow_generate(pr_ctx* ctx, const pr_bow_vocab* vocab, const uint8_t* desc, const int64_t* offs, int32_t N, int32_t cols,
                    double* out, int32_t* n_words) {
  if (int rc = check_args(ctx, "pr_bow_generate", vocab, desc, offs, N, cols, out)) return rc;
  if (N == 0) return PR_OK;
  if (offs[0] != 0) return fail(ctx, PR_EINVAL, "pr_bow_generate: offs[0] = %lld (expected 0)", (long long)offs[0]);
  for (int32_t i = 0; i < N; i++)
    if (offs[i + 1] < offs[i]) return fail(ctx, PR_EINVAL, "pr_bow_generate: offs is not ascending at image %d", i);
  const int64_t F = offs[N];
  if (F >= (1LL << 31)) return fail(ctx, PR_EINVAL, "pr_bow_generate: %lld descriptors in one call (at most 2^31 - 1)", (long long)F);
  if (F > 0 && !desc) return fail(ctx, PR_EINVAL, "pr_bow_generate: desc is NULL");
  PR_CHECK_HIP(ctx, hipSetDevice(pr::ctx_device(ctx)));
  hipStream_t s = pr::ctx_stream(ctx);
  const size_t out_bytes = (size_t)2 * N * cols * sizeof(double);
  uint8_t* ddesc = nullptr;
  int64_t* doffs = nullptr;
  double* dout = nullptr;
  int32_t* dcnt = nullptr;
  auto release = [&]() {
    (void)hipStreamSynchronize(s);
    if (ddesc) (void)hipFree(ddesc);
    if (doffs) (void)hipFree(doffs);
    if (dout) (void)hipFree(dout);
    if (dcnt) (void)hipFree(dcnt);
  };
  hipError_t e = hipMalloc(&ddesc, (size_t)(F > 0 ? F : 1) * 32);
  if (e == hipSuccess) e = hipMalloc(&doffs, (size_t)(N + 1) * sizeof(int64_t));
  if (e == hipSuccess) e = hipMalloc(&dout, out_bytes);
  if (e == hipSuccess) e = hipMalloc(&dcnt, (size_t)(N + 1) * sizeof(int32_t));   // + the truncation word of this call (not a warning: the error below)
  if (e == hipSuccess && F > 0) e = hipMemcpyAsync(ddesc, desc, (size_t)F * 32, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(doffs, offs, (size_t)(N + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    release();
    return fail(ctx, e == hipErrorOutOfMemory ? PR_ENOMEM : PR_EHIP, "pr_bow_generate: %s", hipGetErrorString(e));
  }
  int rc = generate_dev(ctx, vocab, ddesc, F, doffs, N, cols, dout, dcnt, nullptr, dcnt + N);
  std::vector<int32_t> cnt(N);
  if (rc == PR_OK) {
    e = hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), dcnt, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(ctx, PR_EHIP, "pr_bow_generate: %s", hipGetErrorString(e));
  }
  release();
  if (rc) return rc;
  if (n_words) memcpy(n_words, cnt.data(), (size_t)N * sizeof(int32_t));
  for (int32_t i = 0; i < N; i++)
    if (cnt[i] > cols)
      return fail(ctx, PR_EINVAL, "pr_bow_generate: image %d has %d distinct words, more than cols = %d (its row would be cut)", i, cnt[i], cols);
  return PR_OK;
}

}  // extern "C"
