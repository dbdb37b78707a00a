// Writes the GIST generator's host-built tables (so_dso_place_recognition_amd/csrc/gist_tables.hpp) as raw little-endian float32:
//   argv[1]: the whitening circulant, 266 x 266 (the valid part of the [272][272] upload)
//   argv[2]: the Gabor bank for orientations argv[3..] (one count per scale), [sum][256][256]
// Built and run by tests/test_gist_tables.py (host code only).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../so_dso_place_recognition_amd/csrc/gist_tables.hpp"

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s circ.f32 gabor.f32 or1 [or2 ...]\n", argv[0]); return 1; }
  using namespace pr::gist;
  const std::vector<float> C = circulant();
  FILE* f = fopen(argv[1], "wb");
  if (!f) return 2;
  for (int i = 0; i < GP; i++) fwrite(&C[(size_t)i * LD], sizeof(float), GP, f);
  fclose(f);
  std::vector<int> orients;
  for (int a = 3; a < argc; a++) orients.push_back(atoi(argv[a]));
  const std::vector<float> G = gabor_table((int)orients.size(), orients.data());
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(G.data(), sizeof(float), G.size(), f);
  fclose(f);
  return 0;
}
