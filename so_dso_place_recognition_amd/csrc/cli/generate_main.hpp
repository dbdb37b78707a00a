// generate_main.hpp — shared body of test_sc / test_m2dp (SC/test_sc.cpp:12-69, M2DP/test_m2dp.cpp:13-89):
// same parameters, same exit code / message when one is missing, same console lines, same output files.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../../include/place_recognition.h"
#include "../records.hpp"
#include "cli_common.hpp"

// --stream 1: the files are parsed, then replayed keyframe by keyframe through a pr_window (the online pre-stage), and every row is
// generated from the cloud and frame that push left in HBM (pr_*_generate_frames_dev, N = 1).  Same signature file and id file, byte
// for byte, as the default run.  Returns 0, or the exit code of the failing phase; sig holds the rows, ids the emitted pose ids.
inline int generate_stream(pr_ctx* ctx, int kind, const std::string& poses_file, const std::string& pts_file, const std::string& idf,
                           double lidarRange, std::vector<double>& sig, int32_t& N, double& gen_secs) {
  const bool m2dp = kind == 1, delight = kind == 2;
  std::vector<pr_rec::PoseRec> poses;
  pr_rec::History h;
  pr_rec::read_records(poses_file.c_str(), pts_file.c_str(), poses, h);
  FILE* f = fopen(idf.c_str(), "w");
  if (!f) { fprintf(stderr, "pts_preprocess failed: cannot write %s\n", idf.c_str()); return 2; }
  // the cursor rule (pts_preprocess.h:196-200): pose p takes points while id <= pose id
  std::vector<size_t> cut(poses.size() + 1, 0);
  size_t cursor = 0, most = 1;
  for (size_t p = 0; p < poses.size(); p++) {
    while (cursor < h.id.size() && h.id[cursor] <= poses[p].id) cursor++;
    cut[p + 1] = cursor;
    most = std::max(most, cut[p + 1] - cut[p]);
  }
  const int32_t cap = (int32_t)std::max<size_t>(cursor, 1);
  const size_t rows1 = delight ? 16 : (m2dp ? 4 : 1), cols = delight ? PR_DELIGHT_SIG_LEN : (m2dp ? PR_M2DP_SIG_LEN : PR_SC_SIG_LEN);
  pr_window* win = nullptr;
  if (pr_window_create(ctx, lidarRange, (m2dp || delight) ? 1 : 0, cap, (int32_t)most, cap, &win) != PR_OK) {
    fprintf(stderr, "pts_preprocess failed: %s\n", pr_last_error(ctx)); fclose(f); return 2;
  }
  hipStream_t st = (hipStream_t)pr_stream(ctx);
  double *d_pose = nullptr, *d_xyz = nullptr, *d_oxyz = nullptr, *d_frame = nullptr, *d_sig = nullptr;
  float *d_int = nullptr, *d_oint = nullptr;
  int32_t *d_n = nullptr, *d_info = nullptr;
  int64_t* d_offs = nullptr;
  bool ok = hipMalloc(&d_pose, 12 * 8) == hipSuccess && hipMalloc(&d_xyz, most * 24) == hipSuccess && hipMalloc(&d_int, most * 4) == hipSuccess &&
            hipMalloc(&d_n, 4) == hipSuccess && hipMalloc(&d_oxyz, (size_t)cap * 24) == hipSuccess && hipMalloc(&d_oint, (size_t)cap * 4) == hipSuccess &&
            hipMalloc(&d_offs, 16) == hipSuccess && hipMalloc(&d_frame, 16 * 8) == hipSuccess && hipMalloc(&d_info, 16) == hipSuccess &&
            hipMalloc(&d_sig, rows1 * cols * 8) == hipSuccess;
  int code = ok ? 0 : 2;
  if (!ok) fprintf(stderr, "pts_preprocess failed: out of device memory\n");
  N = 0;
  gen_secs = 0.0;
  for (size_t p = 0; p < poses.size() && code == 0; p++) {
    const int32_t n = (int32_t)(cut[p + 1] - cut[p]);
    int32_t info[4] = {0, 0, 0, 0};
    ok = hipMemcpyAsync(d_pose, poses[p].w, 12 * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d_n, &n, 4, hipMemcpyHostToDevice, st) == hipSuccess &&
         (n == 0 || (hipMemcpyAsync(d_xyz, &h.xyz[3 * cut[p]], (size_t)n * 24, hipMemcpyHostToDevice, st) == hipSuccess &&
                     hipMemcpyAsync(d_int, &h.it[cut[p]], (size_t)n * 4, hipMemcpyHostToDevice, st) == hipSuccess)) &&
         pr_window_push_dev(win, d_pose, d_xyz, d_int, d_n, (int32_t)most, d_oxyz, d_oint, d_offs, d_frame, d_info) == PR_OK &&
         hipMemcpyAsync(info, d_info, 16, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) { fprintf(stderr, "pts_preprocess failed: %s\n", pr_last_error(ctx)); code = 2; break; }
    if (!info[0]) continue;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = delight ? pr_delight_generate_frames_dev(ctx, d_oxyz, d_oint, d_offs, 1, d_frame, d_sig)
             : m2dp  ? pr_m2dp_generate_frames_dev(ctx, d_oxyz, d_oint, d_offs, 1, lidarRange, d_frame, 1, d_sig)
                     : pr_sc_generate_frames_dev(ctx, d_oxyz, d_oint, d_offs, 1, lidarRange, d_frame, 1, d_sig);
    if (rc == PR_OK) rc = pr_sync(ctx);
    sig.resize(sig.size() + rows1 * cols);
    if (rc != PR_OK || hipMemcpy(&sig[(size_t)N * rows1 * cols], d_sig, rows1 * cols * 8, hipMemcpyDeviceToHost) != hipSuccess) {
      fprintf(stderr, "generate failed: %s\n", pr_last_error(ctx)); code = 4; break;
    }
    gen_secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(f, "%d\n", poses[p].id);                                                  // :215
    N++;
  }
  fclose(f);
  pr_window_destroy(win);
  for (void* q : {(void*)d_pose, (void*)d_xyz, (void*)d_int, (void*)d_n, (void*)d_oxyz, (void*)d_oint, (void*)d_offs, (void*)d_frame, (void*)d_info,
                  (void*)d_sig})
    if (q) (void)hipFree(q);
  return code;
}

// kind: 0 = SC (test_sc.cpp), 1 = M2DP (test_m2dp.cpp), 2 = DELIGHT (DELIGHT/test_delight.cpp:12-68)
inline int generate_main(int argc, char** argv, int kind) {
  Params prm(argc, argv);
  const bool m2dp = kind == 1, delight = kind == 2;
  const char* out_name = delight ? "delight_file" : (m2dp ? "m2dp_file" : "sc_file");
  std::string poses, pts, outf, idf;
  if (!prm.get("poses_history_file", poses) || !prm.get("pts_history_file", pts) || !prm.get(out_name, outf) ||
      !prm.get("incoming_id_file", idf)) {
    printf("Fail to get params, exit.\n");            // test_sc.cpp:23-24
    return 1;
  }
  const double lidarRange = prm.num("lidarRange", 45.0);   // :27-28
  pr_clouds* clouds = nullptr;
  pr_ctx* ctx = nullptr;
  // PR_CLI_TIMING=1: wall time of each phase on stderr (the console lines of the reference stay as they are)
  const bool timing = getenv("PR_CLI_TIMING") != nullptr;
  auto tp = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    const auto now = std::chrono::steady_clock::now();
    if (timing) fprintf(stderr, "[timing] %-28s %8.3f s\n", what, std::chrono::duration<double>(now - tp).count());
    tp = now;
  };
  int rc = pr_create((int)prm.num("device", 0), &ctx);
  if (rc != PR_OK) { fprintf(stderr, "%s\n", pr_last_error(nullptr)); return 3; }
  lap("create context");
  // pts_preprocess on the device by default (the same clouds bit for bit, 9-20x less wall time end to end);
  // _gpu_prestage:=0 runs the host restatement of utils/pts_preprocess.h instead
  const bool gpu_pre = prm.num("gpu_prestage", 1.0) != 0.0;
  if (prm.num("stream", 0.0) != 0.0) {
    std::vector<double> sig;
    int32_t N = 0;
    double secs = 0.0;
    if (int code = generate_stream(ctx, kind, poses, pts, idf, lidarRange, sig, N, secs)) { pr_destroy(ctx); return code; }
    lap("read + pre-stage + generate (stream)");
    const size_t cols = delight ? PR_DELIGHT_SIG_LEN : (m2dp ? PR_M2DP_SIG_LEN : PR_SC_SIG_LEN), rows = sig.size() / cols;
    printProgress(N ? 1.0 : 0.0);
    printf("\n%s average time: %gms\n", delight ? "DELIGHT" : (m2dp ? "M2DP" : "SC"), N ? 1000.0 * secs / N : 0.0);
    const bool bin = outf.size() > 4 && outf.compare(outf.size() - 4, 4, ".bin") == 0;
    rc = bin ? pr_write_signatures_bin(outf.c_str(), sig.data(), (int64_t)rows, (int64_t)cols, PR_F64)
             : pr_write_signatures(outf.c_str(), sig.data(), (int64_t)rows, (int64_t)cols);
    if (rc != PR_OK) fprintf(stderr, "%s\n", pr_host_last_error());
    pr_destroy(ctx);
    return rc == PR_OK ? 0 : 5;
  }
  rc = gpu_pre ? pr_pts_preprocess_gpu(ctx, poses.c_str(), pts.c_str(), idf.c_str(), lidarRange, (m2dp || delight) ? 1 : 0, 1, &clouds)
               : pr_pts_preprocess(poses.c_str(), pts.c_str(), idf.c_str(), lidarRange, (m2dp || delight) ? 1 : 0, 1, &clouds);
  if (rc != PR_OK) {
    fprintf(stderr, "pts_preprocess failed: %s\n", gpu_pre ? pr_last_error(ctx) : pr_host_last_error());
    pr_destroy(ctx);
    return 2;
  }
  lap(gpu_pre ? "read + pre-stage (gpu)" : "read + pre-stage (host)");
  const int32_t N = (int32_t)pr_clouds_count(clouds);
  const size_t rows = delight ? (size_t)16 * N : (m2dp ? (size_t)4 * N : (size_t)N);
  const size_t cols = delight ? PR_DELIGHT_SIG_LEN : (m2dp ? PR_M2DP_SIG_LEN : PR_SC_SIG_LEN);
  std::vector<double> sig(rows * cols);
  const auto t0 = std::chrono::steady_clock::now();
  // (clouds the GPU pre-stage left in HBM are binned there with the frames it emitted; host-made clouds are uploaded and take both passes)
  rc = pr_generate_clouds(ctx, delight ? PR_TYPE_DELIGHT : (m2dp ? PR_TYPE_M2DP : PR_TYPE_SC), clouds, lidarRange, sig.data());
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc != PR_OK) { fprintf(stderr, "generate failed: %s\n", pr_last_error(ctx)); pr_destroy(ctx); pr_clouds_free(clouds); return 4; }
  lap("generate (incl. copies)");
  if (m2dp && (pr_take_warnings(ctx) & PR_WARN_M2DP_SVD)) {    // rows whose leading singular pair is not unique (may differ from the reference's, N6)
    std::vector<int32_t> rws(1024);
    int32_t cnt = 0;
    if (pr_m2dp_svd_rows(ctx, rws.data(), (int32_t)rws.size(), &cnt) == PR_OK) {
      fprintf(stderr, "warning: leading singular pair not unique in %d row(s):", cnt);
      for (int i = 0; i < cnt && i < (int)rws.size(); i++) fprintf(stderr, " %d", rws[i]);
      fprintf(stderr, "\n");
    }
  }
  printProgress(N ? 1.0 : 0.0);
  printf("\n%s average time: %gms\n", delight ? "DELIGHT" : (m2dp ? "M2DP" : "SC"), N ? 1000.0 * secs / N : 0.0);   // test_sc.cpp:58-61
  const bool bin = outf.size() > 4 && outf.compare(outf.size() - 4, 4, ".bin") == 0;
  rc = bin ? pr_write_signatures_bin(outf.c_str(), sig.data(), (int64_t)rows, (int64_t)cols, PR_F64)
           : pr_write_signatures(outf.c_str(), sig.data(), (int64_t)rows, (int64_t)cols);   // :63-66
  if (rc != PR_OK) fprintf(stderr, "%s\n", pr_host_last_error());
  lap(bin ? "write signatures (.bin)" : "write signatures (text)");
  pr_destroy(ctx);
  pr_clouds_free(clouds);
  return rc == PR_OK ? 0 : 5;
}
