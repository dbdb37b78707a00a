// test_bow — drop-in for BoW/test_bow.cpp:101-166.  Same parameters (_voc_file:=, _incoming_id_file:=, _output_file:=) except the ROS
// bag: _bag:= / _img_topic:= become _descriptors:=LIST, a text file whose line i is the path of message i's ORB descriptors, raw n x 32
// bytes (the data of the cv::Mat ORBextractor returns; relative paths are taken from the list's directory).  ORB extraction is the
// caller's.  _voc_file:= is ORBvoc-style text or its binary side-car (pr_bow_vocab_save_bin).  Frames are selected by the incoming ids
// exactly as the bag loop does (:57-71), and the output file is written as :146-163 writes it: per image a row of word ids and a row of
// values (default ostream precision), each entry followed by " ", padded with "-1 " to 4000 entries (an image with more words gets a
// longer row), std::endl per row.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/place_recognition.h"
#include "cli_common.hpp"

namespace {

bool read_desc(const std::string& path, std::vector<uint8_t>& out, int64_t& n, std::string& err) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) { err = "cannot open " + path; return false; }
  const std::streamoff size = f.tellg();
  if (size < 0 || size % 32) { err = path + ": not n x 32 bytes of ORB descriptors"; return false; }
  f.seekg(0);
  const size_t at = out.size();
  out.resize(at + (size_t)size);
  f.read(reinterpret_cast<char*>(out.data() + at), size);
  if (f.gcount() != size) { err = path + ": truncated"; return false; }
  n = size / 32;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  Params prm(argc, argv);
  std::string voc_file, id, descriptors, output_file;
  if (!prm.get("voc_file", voc_file) || !prm.get("incoming_id_file", id) || !prm.get("descriptors", descriptors) ||
      !prm.get("output_file", output_file)) {
    printf("Fail to get params, exit.\n");        // test_bow.cpp:105-112
    return 1;
  }
  std::cout << std::endl << "Loading ORB Vocabulary from " << voc_file << ". This could take a while..." << std::endl;
  pr_bow_vocab* voc = nullptr;
  if (pr_bow_vocab_load(voc_file.c_str(), &voc) != PR_OK) { fprintf(stderr, "%s\n", pr_host_last_error()); return 2; }
  std::cout << "Vocabulary loaded!" << std::endl << std::endl;

  std::vector<int> incoming_id_vec;               // :35-41
  {
    std::ifstream infile(id);
    int iid;
    while (infile >> iid) incoming_id_vec.push_back(iid);
  }
  std::vector<std::string> frames;
  {
    std::ifstream lf(descriptors);
    if (!lf) { fprintf(stderr, "cannot open %s\n", descriptors.c_str()); pr_bow_vocab_destroy(voc); return 2; }
    const size_t slash = descriptors.find_last_of('/');
    const std::string dir = slash == std::string::npos ? "" : descriptors.substr(0, slash + 1);
    std::string line;
    while (std::getline(lf, line)) {
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
      if (line.empty()) continue;
      frames.push_back(line[0] == '/' ? line : dir + line);
    }
  }
  // the bag loop's selection (:57-71): message img_i is taken when it reaches the next incoming id
  std::vector<uint8_t> desc;
  std::vector<int64_t> offs(1, 0);
  int64_t most = 0;
  size_t id_i = 0;
  for (size_t img_i = 0; img_i < frames.size(); img_i++) {
    if (id_i >= incoming_id_vec.size()) break;
    if (incoming_id_vec[id_i] > (int)img_i) continue;
    id_i++;
    int64_t n = 0;
    std::string err;
    if (!read_desc(frames[img_i], desc, n, err)) { fprintf(stderr, "%s\n", err.c_str()); pr_bow_vocab_destroy(voc); return 2; }
    offs.push_back(offs.back() + n);
    most = std::max(most, n);
  }
  const int32_t N = (int32_t)offs.size() - 1;
  const int32_t cols = (int32_t)std::max<int64_t>(4000, most);   // an image has at most as many words as descriptors
  pr_ctx* ctx = nullptr;
  int rc = pr_create((int)prm.num("device", 0), &ctx);
  if (rc != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(nullptr)); pr_bow_vocab_destroy(voc); return 3; }
  std::vector<double> rows((size_t)2 * N * cols);
  std::vector<int32_t> nw(N);
  const auto t0 = std::chrono::steady_clock::now();
  rc = pr_bow_generate(ctx, voc, desc.data(), offs.data(), N, cols, rows.data(), nw.data());
  const float ttOpt = (float)std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc != PR_OK) { fprintf(stderr, "generate failed: %s\n", pr_last_error(ctx)); pr_destroy(ctx); pr_bow_vocab_destroy(voc); return 4; }
  pr_destroy(ctx);
  pr_bow_vocab_destroy(voc);
  std::cout << std::endl << "BoW vector transform time: " << 1000.0 * ttOpt / N << "ms" << std::endl;   // :142-144

  std::ofstream outfile(output_file);             // :146-163
  for (int32_t i = 0; i < N; i++) {
    const double* ids = rows.data() + (size_t)2 * i * cols;
    const double* vals = ids + cols;
    for (int32_t r = 0; r < nw[i]; r++) outfile << (unsigned int)ids[r] << " ";
    for (int32_t r = nw[i]; r < 4000; r++) outfile << "-1 ";
    outfile << std::endl;
    for (int32_t r = 0; r < nw[i]; r++) outfile << vals[r] << " ";
    for (int32_t r = nw[i]; r < 4000; r++) outfile << "-1 ";
    outfile << std::endl;
  }
  printf("Saved to %s\n", output_file.c_str());
  outfile.close();
  return outfile.fail() ? 5 : 0;
}
