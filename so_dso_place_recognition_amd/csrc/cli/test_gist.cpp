// test_gist — drop-in for GIST/src/test_gist.cpp:23-101.  Same parameters (_incoming_id_file:=, _gist_file:=) except the ROS bag:
// _bag:= / _img_topic:= become _images:=LIST, a text file whose line i is the path of frame i (message i of the topic) as an 8-bit
// binary PGM (P5; relative paths are taken from the list's directory).  Frames are selected by the incoming ids exactly as the bag
// loop does (:61-71), every selected frame must be 256 x 256 (GIST::extract's resize and crop are the caller's), and
// the output file is written as the reference writes it: `val << " "` per value at default ostream precision, std::endl per row.
#include <chrono>
#include <cstdint>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/place_recognition.h"
#include "cli_common.hpp"

namespace {

bool read_pgm(const std::string& path, std::vector<uint8_t>& px, int& w, int& h, std::string& err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { err = "cannot open " + path; return false; }
  auto token = [&f](std::string& t) {
    t.clear();
    int c;
    while ((c = f.get()) != EOF) {
      if (c == '#') { while ((c = f.get()) != EOF && c != '\n') {} continue; }
      if (isspace(c)) { if (!t.empty()) return true; continue; }
      t.push_back((char)c);
    }
    return !t.empty();
  };
  std::string magic, sw, sh, smax;
  if (!token(magic) || magic != "P5" || !token(sw) || !token(sh) || !token(smax)) { err = path + ": not a binary PGM (P5)"; return false; }
  w = atoi(sw.c_str()); h = atoi(sh.c_str());
  const int maxval = atoi(smax.c_str());
  if (w <= 0 || h <= 0 || maxval <= 0 || maxval > 255) { err = path + ": not an 8-bit PGM"; return false; }
  px.resize((size_t)w * h);
  f.read(reinterpret_cast<char*>(px.data()), (std::streamsize)px.size());   // the single whitespace after maxval was consumed by token()
  if ((size_t)f.gcount() != px.size()) { err = path + ": truncated"; return false; }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  Params prm(argc, argv);
  std::string incoming_id_file, images, gist_file;
  if (!prm.get("incoming_id_file", incoming_id_file) || !prm.get("images", images) || !prm.get("gist_file", gist_file)) {
    printf("Fail to get params, exit.\n");        // test_gist.cpp:29-31
    return 1;
  }
  std::vector<int> incoming_id_vec;
  if (incoming_id_file != "") {
    std::ifstream infile(incoming_id_file);
    int iid;
    while (infile >> iid) incoming_id_vec.push_back(iid);
  }
  std::vector<std::string> frames;
  {
    std::ifstream lf(images);
    if (!lf) { fprintf(stderr, "cannot open %s\n", images.c_str()); return 2; }
    const size_t slash = images.find_last_of('/');
    const std::string dir = slash == std::string::npos ? "" : images.substr(0, slash + 1);
    std::string line;
    while (std::getline(lf, line)) {
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
      if (line.empty()) continue;
      frames.push_back(line[0] == '/' ? line : dir + line);
    }
  }
  // the bag loop's selection (:61-71): frame img_i is taken when it reaches the next incoming id
  std::vector<uint8_t> px;
  int32_t n = 0;
  size_t id_i = 0;
  for (size_t img_i = 0; img_i < frames.size(); img_i++) {
    if (incoming_id_file != "") {
      if (id_i >= incoming_id_vec.size()) break;
      if (incoming_id_vec[id_i] > (int)img_i) continue;
      id_i++;
    }
    std::vector<uint8_t> one;
    int w = 0, h = 0;
    std::string err;
    if (!read_pgm(frames[img_i], one, w, h, err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    if (w != 256 || h != 256) {
      fprintf(stderr, "%s is %d x %d: GIST::extract resizes and centre-crops to 256 x 256 first; do that before (INTEGRATION.md)\n",
              frames[img_i].c_str(), w, h);
      return 2;
    }
    px.insert(px.end(), one.begin(), one.end());
    n++;
  }
  const int32_t orients[4] = {8, 8, 8, 8};          // DEFAULT_PARAMS{false, 256, 256, 4, 4, {8, 8, 8, 8}} (:57)
  const int D = pr_gist_signature_size(4, 4, orients);
  pr_ctx* ctx = nullptr;
  int rc = pr_create((int)prm.num("device", 0), &ctx);
  if (rc != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(nullptr)); return 3; }
  std::vector<float> result((size_t)n * D);
  const auto t0 = std::chrono::steady_clock::now();
  rc = pr_gist_generate(ctx, px.data(), PR_U8, n, 256, 256, 4, 4, orients, result.data());
  const float total_time = (float)std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc != PR_OK) { fprintf(stderr, "generate failed: %s\n", pr_last_error(ctx)); pr_destroy(ctx); return 4; }
  pr_destroy(ctx);
  std::ofstream outfile(gist_file);
  for (int32_t i = 0; i < n; i++) {
    for (int k = 0; k < D; k++) outfile << result[(size_t)i * D + k] << " ";   // :89-92
    outfile << std::endl;
  }
  std::cout << std::endl << "GIST average time: " << 1000.0 * total_time / incoming_id_vec.size() << "ms" << std::endl;   // :94-96
  outfile.close();
  return outfile.fail() ? 5 : 0;
}
