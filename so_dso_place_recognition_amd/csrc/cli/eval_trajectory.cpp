// eval_trajectory — a pose file against ground truth through pr_trajeval: one line per metric on stdout.
//   _poses:=FILE     rows of 12 numbers (world to camera [R | t], row-major) or 13 (a frame id in front, as poses_history_file.txt)
//   _gt:=FILE        rows of 12 numbers (_gt_kind:=w2c or c2w, KITTI's gt.txt rows) or 3 (_gt_kind:=positions); row i belongs to pose i
//   _gt_kind:=c2w  _align:=sim3 (none | first | se3 | sim3)  _deltas:=1,10  _lengths:=100,200,..,800  _step:=1  _device:=0
// Exit status: 0, 1 for a file that cannot be used, 2 for a refusal of the library (its message on stderr), 3 without a device.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <fstream>
#include <sstream>
#include <vector>

#include "../../../include/place_recognition.h"
#include "cli_common.hpp"

static bool read_rows(const std::string& path, std::vector<double>& v, int& cols, int& rows) {
  std::ifstream f(path);
  if (!f) return false;
  std::string line;
  cols = 0; rows = 0;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    double x;
    int c = 0;
    while (ss >> x) { v.push_back(x); c++; }
    if (c == 0) continue;
    if (cols == 0) cols = c;
    if (c != cols) return false;
    rows++;
  }
  return rows > 0;
}

static int pick(const std::string& s, const char* const* names, int count) {
  for (int k = 0; k < count; k++)
    if (s == names[k]) return k;
  return -1;
}

template <class T>
static std::vector<T> list_of(const std::string& s) {
  std::vector<T> out;
  std::stringstream ss(s);
  std::string tok;
  while (std::getline(ss, tok, ',')) out.push_back((T)atof(tok.c_str()));
  return out;
}

int main(int argc, char** argv) {
  Params prm(argc, argv);
  std::string poses_file, gt_file, gt_kind = "c2w", align = "sim3", deltas_s = "1,10", lengths_s = "100,200,300,400,500,600,700,800";
  if (!prm.get("poses", poses_file) || !prm.get("gt", gt_file)) {
    fprintf(stderr, "usage: eval_trajectory _poses:=FILE _gt:=FILE [_gt_kind:=w2c|c2w|positions] [_align:=none|first|se3|sim3] [_deltas:=1,10] "
                    "[_lengths:=100,..] [_step:=1]\n");
    return 1;
  }
  prm.get("gt_kind", gt_kind); prm.get("align", align); prm.get("deltas", deltas_s); prm.get("lengths", lengths_s);
  static const char* const KINDS[] = {"w2c", "c2w", "positions"};
  static const char* const ALIGNS[] = {"none", "first", "se3", "sim3"};
  std::vector<double> pv, gv;
  int pc, pr_rows, gc, gr;
  if (!read_rows(poses_file, pv, pc, pr_rows) || (pc != 12 && pc != 13)) { fprintf(stderr, "eval_trajectory: %s: rows of 12 or 13 numbers expected\n", poses_file.c_str()); return 1; }
  if (!read_rows(gt_file, gv, gc, gr) || (gc != 12 && gc != 3)) { fprintf(stderr, "eval_trajectory: %s: rows of 12 or 3 numbers expected\n", gt_file.c_str()); return 1; }
  if (pr_rows != gr) { fprintf(stderr, "eval_trajectory: %d poses but %d ground-truth rows (rows are matched by index)\n", pr_rows, gr); return 1; }
  const int n = pr_rows;
  std::vector<double> est((size_t)n * 12);
  for (int i = 0; i < n; i++)
    for (int c = 0; c < 12; c++) est[(size_t)i * 12 + c] = pv[(size_t)i * pc + (pc - 12) + c];
  const bool pos = gt_kind == "positions";
  std::vector<int32_t> deltas = pos ? std::vector<int32_t>() : list_of<int32_t>(deltas_s);
  std::vector<double> lengths = pos ? std::vector<double>() : list_of<double>(lengths_s);
  pr_trajeval_params p;
  p.node_capacity = n; p.batch = 1; p.align = pick(align, ALIGNS, 4); p.gt_kind = pick(gt_kind, KINDS, 3);
  p.n_deltas = (int32_t)deltas.size(); p.n_lengths = (int32_t)lengths.size(); p.step = (int32_t)prm.num("step", 1); p.edge_capacity = 0;
  p.rot_thr = 0.0; p.trans_thr = 0.0;
  if ((gc == 3) != pos) { fprintf(stderr, "eval_trajectory: %s has %d columns, which does not fit _gt_kind:=%s\n", gt_file.c_str(), gc, gt_kind.c_str()); return 1; }
  pr_trajeval* te = nullptr;
  if (pr_trajeval_scratch_bytes(&p) == 0) {                      // a refusal that needs no device: the library's own text
    pr_trajeval_create(nullptr, &p, deltas.data(), lengths.data(), &te);
    fprintf(stderr, "%s\n", pr_last_error(nullptr));
    return 2;
  }
  pr_ctx* ctx = nullptr;
  if (pr_create((int)prm.num("device", 0), &ctx) != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(nullptr)); return 3; }
  if (pr_trajeval_create(ctx, &p, deltas.data(), lengths.data(), &te) != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(ctx)); return 2; }
  double *d_est = nullptr, *d_gt = nullptr;
  int32_t* d_n = nullptr;
  const int32_t state[4] = {n, 0, 0, 0};
  if (hipMalloc(&d_est, est.size() * 8) != hipSuccess || hipMalloc(&d_gt, gv.size() * 8) != hipSuccess || hipMalloc(&d_n, 16) != hipSuccess ||
      hipMemcpy(d_est, est.data(), est.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_gt, gv.data(), gv.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_n, state, 16, hipMemcpyHostToDevice) != hipSuccess) {
    fprintf(stderr, "eval_trajectory: device memory: %s\n", hipGetErrorString(hipGetLastError()));
    return 3;
  }
  const int K = p.n_deltas, L = p.n_lengths;
  std::vector<double> ate(PR_TRAJ_ATE_STATS), rpe((size_t)PR_TRAJ_RPE_STATS * (K > 0 ? K : 1)), seg((size_t)PR_TRAJ_SEG_STATS * (L + 1));
  pr_trajeval_out o;
  memset(&o, 0, sizeof o);
  o.ate = ate.data(); o.rpe = K > 0 ? rpe.data() : nullptr; o.seg = L > 0 ? seg.data() : nullptr;
  if (pr_trajeval_run(te, d_est, d_n, d_gt, nullptr, nullptr, &o) != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(ctx)); return 2; }
  printf("rows %d used %.0f align %s gt_kind %s flags %.0f\n", n, ate[0], align.c_str(), gt_kind.c_str(), ate[19]);
  printf("ate rmse %.17g mean %.17g max %.17g argmax %.0f\n", ate[2], ate[3], ate[4], ate[5]);
  printf("align s %.17g t %.17g %.17g %.17g\n", ate[6], ate[16], ate[17], ate[18]);
  for (int k = 0; k < K; k++) {
    const double* r = rpe.data() + (size_t)k * PR_TRAJ_RPE_STATS;
    printf("rpe delta %d pairs %.0f trans_rmse %.17g trans_mean %.17g trans_max %.17g rot_rmse %.17g rot_mean %.17g rot_max %.17g\n", deltas[k], r[0],
           r[1], r[2], r[3], r[4], r[5], r[6]);
  }
  for (int l = 0; l <= L && L > 0; l++) {
    const double* s = seg.data() + (size_t)l * PR_TRAJ_SEG_STATS;
    if (l < L) printf("seg length %.17g", lengths[l]);
    else printf("seg all");
    printf(" segments %.0f t_err %.17g r_err %.17g ratio %.17g\n", s[0], s[1], s[2], s[3]);
  }
  pr_trajeval_destroy(te);
  (void)hipFree(d_est); (void)hipFree(d_gt); (void)hipFree(d_n);
  pr_destroy(ctx);
  return 0;
}
