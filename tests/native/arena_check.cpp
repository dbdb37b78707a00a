// arena_check.cpp — host-only check of pr::Arena (csrc/arena.hpp), the one layout rule behind every pr_*_scratch_bytes.
//   arena_check                    the rule itself: take(0), take(1), take(16), take(17), a sequence against its hand formula, alignment
//                                  and order of the offsets; prints "arena ok" and the number of checks
//   arena_check gate EC G          the total of pr_gate's parts as the public header lists them (EC = edge_capacity, G = max_gap + 1)
//   arena_check mapgrow MCP        the total of pr_mapgrow's parts as the public header lists them
// The two totals are compared with the library's pr_gate_scratch_bytes / pr_mapgrow_scratch_bytes by tests/test_arena.py.
#include "arena.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int checks = 0, failed = 0;
#define CHECK(c) do { checks++; if (!(c)) { failed++; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static size_t r16(size_t n) { return (n + 15) / 16 * 16; }

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "gate")) {
    const size_t EC = strtoull(argv[2], nullptr, 10), G = strtoull(argv[3], nullptr, 10);
    pr::Arena a;
    for (size_t bytes : {288 * EC, 8 * EC, 4 * EC, 4 * EC, 4 * EC, 4 * EC, 4 * EC, 8 * G, 8 * G, (size_t)16, EC, 4 * EC, 4 * EC, (size_t)16}) a.take(bytes);
    printf("%zu\n", a.total);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "mapgrow")) {
    const size_t m = strtoull(argv[2], nullptr, 10), nblk = (m + 255) / 256;
    pr::Arena a;
    for (size_t bytes : {(size_t)64, 4 * m, 8 * nblk, (size_t)96, (size_t)16, (size_t)32, 648 * m, 108 * m, 108 * m}) a.take(bytes);
    printf("%zu\n", a.total);
    return 0;
  }
  {
    pr::Arena a;
    CHECK(a.total == 0);
    CHECK(a.take(0) == 0 && a.total == 0);          // nothing taken, nothing added
    CHECK(a.take(1) == 0 && a.total == 16);
    CHECK(a.take(16) == 16 && a.total == 32);
    CHECK(a.take(17) == 32 && a.total == 64);
    CHECK(a.take(0) == 64 && a.total == 64);
  }
  {
    // a sequence of every size class around the boundaries: the total is the sum of the rounded sizes, each offset the sum before it
    std::vector<size_t> sizes;
    for (size_t s = 1; s <= 67; s++) sizes.push_back(s);
    for (size_t s : {(size_t)255, (size_t)256, (size_t)257, (size_t)4095, (size_t)4096, (size_t)4097, ((size_t)1 << 32) - 1, ((size_t)1 << 32) + 1,
                     ((size_t)1 << 40) + 15})
      sizes.push_back(s);
    pr::Arena a;
    size_t want = 0, last = 0;
    bool first = true;
    for (size_t s : sizes) {
      const size_t o = a.take(s);
      CHECK(o == want);
      CHECK(o % 16 == 0);
      CHECK(first || o > last);                     // strictly ordered: no two non-empty parts share an offset
      CHECK(a.total >= o + s);                      // the part lies inside the allocation
      first = false;
      last = o;
      want += r16(s);
    }
    CHECK(a.total == want && a.total % 16 == 0);
  }
  {
    double block[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    CHECK(pr::at<double>(block, 16) == block + 2);
    CHECK(pr::at<char>(block, 0) == reinterpret_cast<char*>(block));
  }
  if (failed) return 1;
  printf("arena ok, %d checks\n", checks);
  return 0;
}
