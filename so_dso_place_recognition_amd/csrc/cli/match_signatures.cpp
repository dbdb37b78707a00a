// match_signatures — executable counterpart of match_signatures/run_test.m:25-57 (the reference runs it from MATLAB:
// test_kitti.m:18-28).  Options mirror run_test's arguments:
//   --type sc|m2dp|delight|gist|bow --hist1 F --hist2 F [--mask_width W=0] [--p_weight 2] [--topk K=1] [--one_based 0|1] --out F
//   [--devices 0,1,...]               hist2 row-sharded over these GPUs (pr_group: RCCL all-gathers between the kernels; sc | m2dp)
//   [--gt1 F --gt2 F --loop_diff L]   positions of the signatures (text matrices, one row per signature): the evaluation half of
//                                     run_test (run_test.m:3-22, :58-85) - prints `AUC = ...` and `top_recall = ...`
//   [--eval_device 1]                 that evaluation on the GPU (pr_precision_recall_gpu) instead of the host loops; the same printed lines
//   [--exact_statistics 0|1]          every query answered from its exact fp64 row (scores = the reference's doubles to rounding).  Default: 1
//                                     with --gt1 / --gt2 - the sweep ranks the QUERIES by score (run_test.m:58), and two queries whose scores
//                                     agree to 1e-5 must not change places -, else 0
//   [--online 1]                      the causal form of the same match (what a running SLAM front end asks: SC/test_sc.cpp:40-56 produces one row per
//                                     keyframe): row t of hist1 is matched against rows 0 .. t - mask_width of hist1 ITSELF (hist2 is not read; the
//                                     mask of run_test.m:47-53 restricted to the past), then joins the database - resident on the GPU and grown IN
//                                     PLACE (pr_group_set_database_growable / pr_group_append_database), one pr_group_match_topk per keyframe.
//                                     Rows with fewer than two candidates come out as -1 NaN.  sc | m2dp; --devices optional (default: device 0)
//   [--align_out F]                   the best-aligning variant of every returned pair (pr_match_align, one device whatever --devices; with --online
//                                     the indices are rows of hist1): one line per query, K groups "v_ch0 v_ch1", -1 where there is none.  SC: structure,
//                                     intensity, v = 2 shift + mirror (processSC.m:24-27); M2DP: count, intensity, v = 4 a + b (processM2DP.m:18);
//                                     DELIGHT: the octant permutation (processDELIGHT.m:2-5) and -1.  sc | m2dp | delight
//   [--icp_out F --poses1 F --pts1 F [--poses2 F --pts2 F]]   refine and verify every returned pair (--type sc|delight): the clouds of hist1 (and
//                                     of hist2 for a cross match; with --online or without --poses2 they are hist1's) come from the pose / point
//                                     files through pr_pts_preprocess_gpu (--lidarRange 45; the down-sampling of the type's generator: voxel for
//                                     sc, polar for delight), the seed from pr_match_align + pr_sc_relative_pose / pr_relative_pose,
//                                     the refinement from pr_icp_pairs (--icp_max_corr 1 --icp_max_iter 30 --icp_tol_rmse 1e-6 --icp_tol_fitness
//                                     1e-6 --icp_min_inliers 3).  One line per (query, candidate): "query match status iters fitness rmse" and
//                                     the 12 numbers of [R | t] row by row (status: PR_ICP_*; match -1 / status 4 where there is no pair)
//   [--icp_hyp 2]                     (--type sc) also refine the intensity channel's variant where it differs from the structure channel's and
//                                     keep the better result (larger fitness, then smaller rmse, among status converged / max_iter; DESIGN.md
//                                     4.12); the line then ends with the kept hypothesis "hyp" (0 | 1)
//   [--seq_len L --seq_vel "1,-1,0.75,-0.75"]   sequence matching (sc | m2dp | delight): hist1's rows are consecutive keyframes of a
//                                     drive; the scores are summed along L lags of DB trajectories of the listed velocities (rows of DB per query
//                                     row; negative: a reverse traversal; default "1,-1") and the K smallest means are returned
//                                     (pr_match_topk_seq_f64).  Refused together with --online, --icp_out, --align_out or --devices
//   [--icp_search brute|grid]         the correspondence search of the refinement (pr_set_icp_search; default: the context's mode, i.e. brute
//                                     force unless PR_ICP_SEARCH says otherwise).  grid: the exact uniform-grid search
// Output: one line per query: K pairs "index score" (0-based indices unless --one_based 1), and the reference's
// console lines `type` / `tm` (ms per query, run_test.m:42-44).  Scores are doubles, as MATLAB holds them.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../../include/place_recognition.h"
#include "cli_common.hpp"
#include "../pose_seed.hpp"

int main(int argc, char** argv) {
  Params prm(argc, argv);
  std::string type, h1f, h2f, outf;
  if (!prm.get("type", type) || !prm.get("hist1", h1f) || !prm.get("hist2", h2f) || !prm.get("out", outf) ||
      (type != "sc" && type != "m2dp" && type != "delight" && type != "gist" && type != "bow")) {
    printf("usage: match_signatures --type sc|m2dp|delight|gist|bow --hist1 F --hist2 F [--mask_width W] [--p_weight 2] [--topk K] [--one_based 0|1] --out F [--align_out F]\n");
    return 1;
  }
  const int t = type == "sc" ? PR_TYPE_SC : type == "m2dp" ? PR_TYPE_M2DP : type == "delight" ? PR_TYPE_DELIGHT : type == "gist" ? PR_TYPE_GIST : PR_TYPE_BOW;
  const bool cols_type = t == PR_TYPE_GIST || t == PR_TYPE_BOW;        // no fixed signature length
  std::string alignf;
  const bool want_align = prm.get("align_out", alignf);
  if (want_align && cols_type) { fprintf(stderr, "--align_out needs --type sc|m2dp|delight (gist / bow signatures have no variants)\n"); return 1; }
  std::string icpf;
  const bool want_icp = prm.get("icp_out", icpf);
  if (want_icp) {
    std::string a, b;
    // (m2dp has a seed too - pr_relative_pose(PR_POSE_M2DP) - but the executable keeps refusing it for now)
    if ((t != PR_TYPE_SC && t != PR_TYPE_DELIGHT) || !prm.get("poses1", a) || !prm.get("pts1", b)) { fprintf(stderr, "--icp_out needs --type sc|delight and --poses1 / --pts1\n"); return 1; }
    const int hyp = (int)prm.num("icp_hyp", 1);
    if (hyp != 1 && !(hyp == 2 && t == PR_TYPE_SC)) { fprintf(stderr, "--icp_out: --icp_hyp is 1, or 2 with --type sc (DELIGHT has one variant per pair)\n"); return 1; }
  }
  std::string icp_search;
  const bool has_icp_search = prm.get("icp_search", icp_search);
  if (has_icp_search && icp_search != "brute" && icp_search != "grid") { fprintf(stderr, "--icp_search is brute or grid, not %s\n", icp_search.c_str()); return 1; }
  // --seq_len L [--seq_vel "1,-1,..."]: the sequence form; the step table is api.seq_steps' (sign(v) floor(|v| l + 0.5), identical rows dropped)
  const int seq_len = (int)prm.num("seq_len", 0);
  std::vector<int32_t> seq_steps;
  int seq_V = 0;
  if (seq_len != 0) {
    std::string a;
    if (prm.num("online", 0) != 0 || want_icp || want_align || prm.get("devices", a)) {
      fprintf(stderr, "--seq_len (sequence matching, one device, whole drive) cannot be combined with --online, --icp_out, --align_out or --devices\n");
      return 1;
    }
    if (cols_type) { fprintf(stderr, "--seq_len needs --type sc|m2dp|delight\n"); return 1; }
    if (seq_len < 1 || seq_len > PR_SEQ_MAX_L) { fprintf(stderr, "--seq_len is 1 .. %d, not %d\n", PR_SEQ_MAX_L, seq_len); return 1; }
    std::string vels = "1,-1";
    (void)prm.get("seq_vel", vels);
    for (size_t p = 0; p < vels.size();) {
      char* end = nullptr;
      const double v = strtod(vels.c_str() + p, &end);
      if (end == vels.c_str() + p || !std::isfinite(v)) { fprintf(stderr, "--seq_vel is a comma-separated list of numbers, not %s\n", vels.c_str()); return 1; }
      std::vector<int32_t> row(seq_len);
      for (int l = 0; l < seq_len; l++) row[l] = (int32_t)((v > 0 ? 1 : v < 0 ? -1 : 0) * std::floor(std::fabs(v) * l + 0.5));
      if (std::abs(row[seq_len - 1]) > PR_SEQ_MAX_STEP) { fprintf(stderr, "--seq_vel: velocity %g reaches beyond %d rows within %d lags\n", v, PR_SEQ_MAX_STEP, seq_len); return 1; }
      bool dup = false;
      for (int u = 0; u < seq_V && !dup; u++) dup = std::equal(row.begin(), row.end(), seq_steps.begin() + (size_t)u * seq_len);
      if (!dup) { seq_steps.insert(seq_steps.end(), row.begin(), row.end()); seq_V++; }
      p = (size_t)(end - vels.c_str());
      if (p < vels.size() && vels[p] != ',') { fprintf(stderr, "--seq_vel is a comma-separated list of numbers, not %s\n", vels.c_str()); return 1; }
      p++;
    }
    if (seq_V < 1 || seq_V > PR_SEQ_MAX_V) { fprintf(stderr, "--seq_vel holds 1 .. %d distinct velocities\n", PR_SEQ_MAX_V); return 1; }
  }
  const int div = t == PR_TYPE_SC ? 1 : t == PR_TYPE_M2DP ? 4 : t == PR_TYPE_DELIGHT ? 16 : t == PR_TYPE_BOW ? 2 : 1;
  int64_t width = t == PR_TYPE_SC ? PR_SC_SIG_LEN : (t == PR_TYPE_M2DP ? PR_M2DP_SIG_LEN : PR_DELIGHT_SIG_LEN);
  double *h1 = nullptr, *h2 = nullptr;
  int64_t r1, c1, r2, c2;
  auto rd = [](const std::string& f, double** o, int64_t* r, int64_t* c) {
    const bool bin = f.size() > 4 && f.compare(f.size() - 4, 4, ".bin") == 0;
    return bin ? pr_read_signatures_bin(f.c_str(), o, r, c) : pr_read_signatures(f.c_str(), o, r, c);
  };
  if (rd(h1f, &h1, &r1, &c1) != PR_OK || rd(h2f, &h2, &r2, &c2) != PR_OK) {
    fprintf(stderr, "%s\n", pr_host_last_error());
    return 2;
  }
  if (cols_type) width = c1;
  if (c1 != width || c2 != width || r1 % div || r2 % div) { fprintf(stderr, "signature files must be [%d*m x %ld]\n", div, (long)width); return 2; }
  const int32_t m = (int32_t)(r1 / div), n = (int32_t)(r2 / div), k = (int32_t)prm.num("topk", 1);
  std::vector<int32_t> idx((size_t)m * k);
  std::vector<double> score((size_t)m * k);
  std::vector<float> score32;
  pr_ctx* ctx = nullptr;
  std::string devs;
  std::vector<int32_t> dev_ids;
  if (prm.get("devices", devs)) {
    for (size_t p = 0; p < devs.size();) { dev_ids.push_back(atoi(devs.c_str() + p)); p = devs.find(',', p); if (p == std::string::npos) break; p++; }
    if (dev_ids.empty() || (t != PR_TYPE_SC && t != PR_TYPE_M2DP)) { fprintf(stderr, "--devices needs a device list and --type sc|m2dp\n"); return 1; }
  }
  // one context for the single-device call; with --devices the group owns one context per shard and this one is not needed
  if (dev_ids.empty() && pr_create((int)prm.num("device", 0), &ctx) != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(nullptr)); return 3; }
  pr_group* grp = nullptr;
  if (!dev_ids.empty()) {
    if (pr_group_create(dev_ids.data(), (int32_t)dev_ids.size(), &grp) != PR_OK) { fprintf(stderr, "%s\n", pr_group_last_error(nullptr)); return 3; }
    if (pr_group_set_database(grp, t, h2, n) != PR_OK) { fprintf(stderr, "%s\n", pr_group_last_error(grp)); return 4; }
    printf("devices = %d (%s)\n", (int)dev_ids.size(), pr_group_uses_rccl(grp) ? "RCCL" : "copies");
  }
  {
    std::string a, b;
    const bool exact = prm.num("exact_statistics", (prm.get("gt1", a) && prm.get("gt2", b)) ? 1.0 : 0.0) != 0.0;
    if (exact && ctx) (void)pr_set_exact_statistics(ctx, 1);
    if (exact && grp) (void)pr_group_set_exact_statistics(grp, 1);
  }
  const bool online = prm.num("online", 0) != 0;
  if (online && t != PR_TYPE_SC && t != PR_TYPE_M2DP) { fprintf(stderr, "--online needs --type sc|m2dp\n"); return 1; }
  if (online && !grp) {                                                  // the growing database lives in a pr_group (one device unless --devices)
    const int32_t d0 = (int32_t)prm.num("device", 0);
    if (pr_group_create(&d0, 1, &grp) != PR_OK) { fprintf(stderr, "%s\n", pr_group_last_error(nullptr)); return 3; }
  }
  const auto t0 = std::chrono::steady_clock::now();
  int rc;
  if (online) {
    const int32_t mask = (int32_t)prm.num("mask_width", 0), lag = mask > 1 ? mask - 1 : 0;
    const size_t rowd = (size_t)div * (size_t)width;                    // doubles per signature
    int32_t have = 0;                                                   // rows of hist1 in the database: rows 0 .. have - 1
    rc = PR_OK;
    for (int32_t q = 0; q < m && rc == PR_OK; q++) {
      const int32_t want = q - lag;                                     // rows the mask admits for keyframe q: 0 .. q - lag - 1
      if (want >= 2 && have == 0) {                                     // two rows: the first database (N - 1 standard deviation)
        rc = pr_group_set_database_growable(grp, t, h1, 2, m);
        have = 2;
      }
      if (rc == PR_OK && have > 0 && want > have) { rc = pr_group_append_database(grp, h1 + (size_t)have * rowd, want - have); have = want; }
      if (rc != PR_OK) break;
      if (have < 2) { for (int32_t j = 0; j < k; j++) { idx[(size_t)q * k + j] = -1; score[(size_t)q * k + j] = NAN; } continue; }
      rc = pr_group_match_topk(grp, h1 + (size_t)q * rowd, 1, 0, prm.num("p_weight", 2.0), k, idx.data() + (size_t)q * k, score.data() + (size_t)q * k);
    }
    if (rc != PR_OK) { fprintf(stderr, "online match failed (%d): %s\n", rc, pr_group_last_error(grp)); return 4; }
    printf("online = 1 (database rows at the end: %d)\n", (int)pr_group_database_rows(grp));
  } else if (grp) {
    rc = pr_group_match_topk(grp, h1, m, (int32_t)prm.num("mask_width", 0), prm.num("p_weight", 2.0), k, idx.data(), score.data());
    if (rc != PR_OK) { fprintf(stderr, "match failed (%d): %s\n", rc, pr_group_last_error(grp)); return 4; }
  } else if (seq_len) {
    std::vector<int32_t> vel((size_t)m * k);
    rc = pr_match_topk_seq_f64(ctx, t, h1, m, h2, n, (int32_t)prm.num("mask_width", 0), prm.num("p_weight", 2.0), k, seq_steps.data(), seq_V, seq_len,
                               idx.data(), score.data(), vel.data());
    printf("seq_len = %d\nseq_velocities = %d\n", seq_len, seq_V);
  } else if (cols_type) {
    score32.resize(score.size());
    rc = pr_match_topk_cols(ctx, t, h1, m, h2, n, (int32_t)width, (int32_t)prm.num("mask_width", 0), k, idx.data(), score32.data());
    for (size_t i = 0; i < score.size(); i++) score[i] = (double)score32[i];
  } else {
    rc = pr_match_topk_f64(ctx, t, h1, m, h2, n, (int32_t)prm.num("mask_width", 0), prm.num("p_weight", 2.0), k, idx.data(), score.data());
  }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc != PR_OK) { fprintf(stderr, "match failed (%d): %s\n", rc, pr_last_error(ctx)); pr_destroy(ctx); return 4; }
  printf("type = %s\ntm = %g\n", type.c_str(), m ? 1000.0 * secs / m : 0.0);
  const int warn = grp ? pr_group_take_warnings(grp) : pr_take_warnings(ctx);
  if (warn > 0 && (warn & PR_WARN_F16_FALLBACK)) printf("note: some queries were recomputed in split-f16 (PR_SC_ARITH_F16 margin check)\n");
  if (warn > 0 && (warn & PR_WARN_ORDER_RESOLVED)) printf("note: some queries were answered with fp64 row statistics (order check, pr_order_resolve_dev)\n");
  if (warn > 0 && (warn & PR_WARN_NAN_ROWS)) printf("warning: zero-norm signature rows never match (NaN in MATLAB, processSC.m:16,19)\n");
  std::string g1f, g2f;
  if (prm.get("gt1", g1f) && prm.get("gt2", g2f)) {   // run_test.m:3-22, 58-85
    double *g1 = nullptr, *g2 = nullptr;
    int64_t gr1, gc1, gr2, gc2;
    if (rd(g1f, &g1, &gr1, &gc1) != PR_OK || rd(g2f, &g2, &gr2, &gc2) != PR_OK) { fprintf(stderr, "%s\n", pr_host_last_error()); pr_destroy(ctx); return 2; }
    if (gr1 != m || gr2 != n || gc1 != gc2) { fprintf(stderr, "gt files must hold one row per signature (%d / %d rows, same columns)\n", m, n); pr_destroy(ctx); return 2; }
    std::vector<double> v((size_t)m);
    std::vector<int32_t> bi((size_t)m);
    for (int32_t i = 0; i < m; i++) { v[i] = score[(size_t)i * k]; bi[i] = idx[(size_t)i * k]; }
    double auc = 0, tr = 0;
    int32_t nd = 0;
    if (prm.num("eval_device", 0) != 0) {
      if (!ctx && pr_create(dev_ids.empty() ? (int)prm.num("device", 0) : dev_ids[0], &ctx) != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(nullptr)); return 3; }
      if (pr_precision_recall_gpu(ctx, v.data(), bi.data(), m, g1, g2, n, (int32_t)gc1, prm.num("loop_diff", 10.0), (int32_t)prm.num("mask_width", 0),
                                  &auc, &tr, nullptr, nullptr, nullptr, &nd, nullptr, nullptr) != PR_OK) {
        fprintf(stderr, "%s\n", pr_last_error(ctx)); pr_destroy(ctx); return 4;
      }
    } else
    if (pr_precision_recall(v.data(), bi.data(), m, g1, g2, n, (int32_t)gc1, prm.num("loop_diff", 10.0), (int32_t)prm.num("mask_width", 0), &auc, &tr,
                            nullptr, &nd) != PR_OK) { fprintf(stderr, "%s\n", pr_host_last_error()); pr_destroy(ctx); return 4; }
    printf("AUC = %.9g\ntop_recall = %.9g\nlp_detected = %d\n", auc, tr, nd);
    pr_free(g1); pr_free(g2);
  }
  if (want_align) {   // the variants of the returned pairs, on one device (the online form matched hist1 against its own earlier rows)
    if (!ctx && pr_create(dev_ids.empty() ? (int)prm.num("device", 0) : dev_ids[0], &ctx) != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(nullptr)); return 3; }
    std::vector<int32_t> var((size_t)m * k * 2);
    std::vector<double> vd((size_t)m * k * 2);
    if (pr_match_align(ctx, t, h1, m, online ? h1 : h2, online ? m : n, k, idx.data(), var.data(), vd.data()) != PR_OK) {
      fprintf(stderr, "alignment failed: %s\n", pr_last_error(ctx)); pr_destroy(ctx); return 4;
    }
    FILE* fa = fopen(alignf.c_str(), "w");
    if (!fa) { fprintf(stderr, "cannot write %s\n", alignf.c_str()); pr_destroy(ctx); return 5; }
    for (int32_t i = 0; i < m; i++) {
      for (int32_t j = 0; j < k; j++) fprintf(fa, "%s%d %d", j ? " " : "", var[((size_t)i * k + j) * 2], var[((size_t)i * k + j) * 2 + 1]);
      fputc('\n', fa);
    }
    fclose(fa);
  }
  if (want_icp) {   // seed (pr_match_align + pr_sc_relative_pose / pr_relative_pose) and ICP refinement of every returned pair, on one device
    if (!ctx && pr_create(dev_ids.empty() ? (int)prm.num("device", 0) : dev_ids[0], &ctx) != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(nullptr)); return 3; }
    std::string p1, s1, p2, s2;
    prm.get("poses1", p1); prm.get("pts1", s1);
    const bool two = !online && prm.get("poses2", p2) && prm.get("pts2", s2);
    pr_clouds *cl1 = nullptr, *cl2 = nullptr;
    const double range = prm.num("lidarRange", 45.0);
    const int polar = t == PR_TYPE_DELIGHT ? 1 : 0;                      // the down-sampling of the type's generator (generate_main.hpp)
    const int H = (int)prm.num("icp_hyp", 1);
    if (pr_pts_preprocess_gpu(ctx, p1.c_str(), s1.c_str(), nullptr, range, polar, 0, &cl1) != PR_OK ||
        (two && pr_pts_preprocess_gpu(ctx, p2.c_str(), s2.c_str(), nullptr, range, polar, 0, &cl2) != PR_OK)) {
      fprintf(stderr, "pre-stage failed: %s\n", pr_last_error(ctx)); pr_destroy(ctx); return 4;
    }
    if (!two) cl2 = cl1;
    const int32_t nd = online ? m : n;
    if (pr_clouds_count(cl1) != m || pr_clouds_count(cl2) != nd) {
      fprintf(stderr, "the pose / point files give %ld / %ld clouds for %d / %d signatures\n", (long)pr_clouds_count(cl1), (long)pr_clouds_count(cl2), m, nd);
      pr_destroy(ctx); return 2;
    }
    std::vector<int32_t> var((size_t)m * k * 2);
    std::vector<double> vd((size_t)m * k * 2);
    if (pr_match_align(ctx, t, h1, m, online ? h1 : h2, nd, k, idx.data(), var.data(), vd.data()) != PR_OK) {
      fprintf(stderr, "alignment failed: %s\n", pr_last_error(ctx)); pr_destroy(ctx); return 4;
    }
    auto frames_of = [&](pr_clouds* cl, int32_t N, std::vector<double>& f) {      // PCA frames of the resident clouds, to the host
      f.assign((size_t)N * 16, 0.0);
      if (N == 0 || !pr_clouds_dev_xyz(cl)) return true;
      double* d = nullptr;
      if (hipMalloc(&d, (size_t)N * 16 * 8) != hipSuccess) return false;
      bool ok = pr_cloud_frames_dev(ctx, pr_clouds_dev_xyz(cl), pr_clouds_dev_inten(cl), pr_clouds_dev_offs(cl), N, d) == PR_OK && pr_sync(ctx) == PR_OK &&
                hipMemcpy(f.data(), d, (size_t)N * 16 * 8, hipMemcpyDeviceToHost) == hipSuccess;
      (void)hipFree(d);
      return ok;
    };
    std::vector<double> f1, f2;
    if (!frames_of(cl1, m, f1) || !frames_of(cl2, nd, f2)) { fprintf(stderr, "frames failed: %s\n", pr_last_error(ctx)); pr_destroy(ctx); return 4; }
    const size_t c = (size_t)m * k, slots = c * H;                       // slot e * H + h: hypothesis h of pair e
    std::vector<int32_t> src(slots, -1), dst(slots, -1);
    std::vector<double> T0(slots * 12, 0.0), T(slots * 12, 0.0);
    for (size_t e = 0; e < c; e++)
      for (int h = 0; h < H; h++) {
        const size_t o = e * H + h;
        T0[o * 12] = T0[o * 12 + 5] = T0[o * 12 + 10] = 1.0;
        const int32_t q = (int32_t)(e / k), b = idx[e], v = var[e * 2 + h];
        if (b < 0 || b >= nd || v < 0 || (h > 0 && v == var[e * 2])) continue;
        const double *fq = f1.data() + (size_t)q * 16, *fb = f2.data() + (size_t)b * 16;
        const int rc_seed = t == PR_TYPE_SC ? pr_sc_relative_pose(fq, fb, &v, 1, T0.data() + o * 12) : pr_relative_pose(PR_POSE_DELIGHT, fq, fb, &v, 1, T0.data() + o * 12);
        if (rc_seed != PR_OK) continue;   // (a cloud of fewer than 3 points)
        src[o] = q; dst[o] = b;
      }
    std::vector<pr_icp_stats> stats(slots);
    if (has_icp_search && pr_set_icp_search(ctx, icp_search == "grid" ? PR_ICP_SEARCH_GRID : PR_ICP_SEARCH_BRUTE) != PR_OK) {
      fprintf(stderr, "%s\n", pr_last_error(ctx)); pr_destroy(ctx); return 4;
    }
    if (pr_icp_pairs(ctx, pr_clouds_xyz(cl1), pr_clouds_offs(cl1), m, pr_clouds_xyz(cl2), pr_clouds_offs(cl2), nd, src.data(), dst.data(), (int32_t)slots,
                     T0.data(), (int32_t)prm.num("icp_max_iter", 30), prm.num("icp_max_corr", 1.0), prm.num("icp_tol_rmse", 1e-6),
                     prm.num("icp_tol_fitness", 1e-6), (int32_t)prm.num("icp_min_inliers", 3), T.data(), stats.data()) != PR_OK) {
      fprintf(stderr, "refinement failed: %s\n", pr_last_error(ctx)); pr_destroy(ctx); return 4;
    }
    FILE* fi = fopen(icpf.c_str(), "w");
    if (!fi) { fprintf(stderr, "cannot write %s\n", icpf.c_str()); pr_destroy(ctx); return 5; }
    for (size_t e = 0; e < c; e++) {
      const int kept = pr::pose_select(stats.data() + e * H, H, PR_ICP_CONVERGED, PR_ICP_MAX_ITER);    // the rule of verify_select_kernel
      const size_t o = e * H + (kept < 0 ? 0 : kept);
      fprintf(fi, "%d %d %d %d %.17g %.17g", (int)(e / k), dst[o], stats[o].status, stats[o].iters, stats[o].fitness, stats[o].rmse);
      for (int a = 0; a < 12; a++) fprintf(fi, " %.17g", T[o * 12 + a]);
      if (H == 2) fprintf(fi, " %d", kept < 0 ? 0 : kept);
      fputc('\n', fi);
    }
    fclose(fi);
    if (two) pr_clouds_free(cl2);
    pr_clouds_free(cl1);
  }
  FILE* f = fopen(outf.c_str(), "w");
  if (!f) { fprintf(stderr, "cannot write %s\n", outf.c_str()); pr_destroy(ctx); return 5; }
  const int base = prm.num("one_based", 0) != 0 ? 1 : 0;
  for (int32_t i = 0; i < m; i++) {
    for (int32_t j = 0; j < k; j++) fprintf(f, "%s%d %.17g", j ? " " : "", idx[(size_t)i * k + j] < 0 ? -1 : idx[(size_t)i * k + j] + base, score[(size_t)i * k + j]);
    fputc('\n', f);
  }
  fclose(f);
  pr_free(h1); pr_free(h2);
  pr_group_destroy(grp);
  pr_destroy(ctx);
  return 0;
}
