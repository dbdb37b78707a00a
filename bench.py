#!/usr/bin/env python3
"""bench.py — headline benchmark of the place-recognition hot path on MI355X.

Metric (BASELINE.json): queries/sec over a 100k-signature DB, top-1 index parity.
Workload (`config.workload`): Scan-Context 20x60 matching, m = 4096 synthetic queries planted on an
n = 100 000-signature synthetic DB (SURVEY.md §8-d "metric config"), mask_width 0, p_weight 2, k = 1.
One step = the whole match path on inputs already resident in HBM as f64 signatures:
    pack queries (L2-normalise + sector rfft) -> pack DB shard -> all-pairs SC distance (both channels)
    -> per-row moments -> [all-gather moments] -> z-score fusion + mask + top-1 -> [all-gather + merge]
i.e. run_test.m:25-57.  With N > 1 GPUs the SAME 100k DB is row-sharded over the ranks (strong scaling,
SURVEY.md §8-e); queries are replicated.  value = queries of all steps / max-over-ranks wall time.

A plain run does only what `value` needs: it sets up, warms up, times the steps, writes --dump-outputs and prints the JSON line.
Everything below (all outside the timed region) runs with --full only.

`extra` (outside the timed region, N = 1 only): the secondary workloads of BASELINE.json measured in the same run - M2DP matching
over a 50k-signature DB (config 3), SC generation from 50 000-point clouds (config 2), and the fp32-MFMA arithmetic of the SC matcher.

Extra objects on the JSON line: `roofline` (the dominant kernel - sc_match_e_kernel, split-f16 MFMA, by default;
sc_match_kernel, fp32 MFMA, with --sc-arith f32 - timed live with HIP events on the stream it runs on; algorithmic
FLOPs = 23 856 fp32 FLOP per (query, entry) pair = 71 568 f16 FLOP in the split form; since round 4 the binary intensity
channel of the synthetic signatures - SC/SC.cpp:67-72 writes 0 / 1 there - takes a launch of its own with one f16 product per term and
exact integer rounding, so the dominant kernel is the split-f16 launch of the structure channel: 35 784 f16 FLOP per
pair, timed by the library's own events around that launch, pr_set_kernel_timing), `cpu_baseline` (the CPU oracle =
a port of the reference, timed on this host's cores on a bounded query sample at N = 1), `parity` (GPU top-1 vs
that oracle on the sample and vs the planted ground truth on all queries).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic FLOP per (query, entry) pair of the formulation sc_match.hip runs, per channel:
#   stage 1: 29 frequencies x 4 real K=20 dots (160) + 2 real-only frequencies x 1 dot (40)            = 4 720
#   stage 2: {fwd, mir} x ( E: 31 shifts x 31 freqs + O: 29 shifts x 29 freqs ) x 2 FLOP               = 7 208
FLOP_PER_PAIR = 2 * (29 * 160 + 2 * 40 + 2 * 2 * (31 * 31 + 29 * 29))    # 23 856
MFMA_F32_PEAK_TFLOPS = 157.3             # MI355X_MICROARCH.md: Peak FP32 (matrix)
# split-f16 arithmetic (sc_match_h.hip): the same formulation with every fp32 product carried as three f16 products
# (hi*hi + hi*lo + lo*hi, fp32 accumulate) on the f16 matrix cores
FLOP_PER_PAIR_F16X2 = 3 * FLOP_PER_PAIR  # 71 568
MFMA_F16_PEAK_TFLOPS = 2500.0            # MI355X_MICROARCH.md: BF16/F16 ~2.5 PF dense


class HipEvents:
    """HIP events on an arbitrary hipStream_t (torch.cuda.Event only sees torch's own streams)."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def create(self):
        e = C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(e)) == 0
        return e

    def record(self, e, stream):
        assert self.hip.hipEventRecord(e, C.c_void_p(stream)) == 0

    def elapsed_ms(self, a, b):
        assert self.hip.hipEventSynchronize(b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
        return ms.value


def blas_baseline(q_host, db_host, S):
    """The reference matcher in its own shape (processSC.m:15-33 + run_test.m:38-41, 57): rows / L2 norm, per query and channel ONE dense
    dgemm `sig_i (120 x 1200) * hist2' (1200 x n)` on the host's multithreaded BLAS (numpy -> OpenBLAS), column minimum, 2:1 z-score fusion,
    arg-min.  Returns (seconds, top-1 indices, threads BLAS reports)."""
    import numpy as np
    try:
        from threadpoolctl import threadpool_info
        nthr = max([p.get("num_threads", 1) for p in threadpool_info() if p.get("user_api") == "blas"] or [1])
    except Exception:
        nthr = None
    s, r = np.meshgrid(np.arange(60), np.arange(20), indexing="ij")              # flattened bin = sector * 20 + ring (SC.cpp:39)
    V = np.empty((120, 1200), np.int64)
    for k0 in range(60):
        V[k0] = (((k0 + s) % 60) * 20 + r).reshape(-1)                            # processSC.m:40 forward rotation
        V[60 + k0] = (((k0 - s) % 60) * 20 + r).reshape(-1)                       # processSC.m:42 mirrored rotation
    t0 = time.perf_counter()
    h2t = []
    for c in range(2):
        x = db_host[:, 1200 * c: 1200 * (c + 1)]
        h2t.append(np.ascontiguousarray((x / np.sqrt((x * x).sum(1, keepdims=True))).T))     # processSC.m:18-20
    top1 = np.empty(S, np.int64)
    for i in range(S):
        f = 0.0
        for c in range(2):
            row = q_host[i, 1200 * c: 1200 * (c + 1)]
            row = row / np.sqrt((row * row).sum())                                # processSC.m:15-17
            d = ((1.0 - row[V] @ h2t[c]) / 2.0).min(0)                            # processSC.m:30-32
            f = f + (2.0 if c == 0 else 1.0) * (d - d.mean()) / d.std(ddof=1)     # run_test.m:38-41
        top1[i] = int(np.argmin(f))                                               # run_test.m:57
    return time.perf_counter() - t0, top1, nthr


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, **arrays):
    """--dump-outputs: what the timed path handed its caller in the last timed step, one float64 DIR/<name>.npy per array (DB row
    indices are exact in float64).  The inputs are seeded, so two builds run with the same arguments can be compared file for file.
    All arrays share their first axis (one row per query); above DUMP_LIMIT_BYTES a fixed, seeded sample of rows is kept, and the
    query numbers of that sample go to DIR/rows.npy."""
    import numpy as np
    out = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    m = len(next(iter(out.values())))
    row_bytes = sum(a.nbytes for a in out.values()) // max(m, 1)
    budget = DUMP_LIMIT_BYTES - 4096                     # room for the .npy headers
    if row_bytes * m > budget:
        rows = np.sort(np.random.default_rng(0).choice(m, budget // (row_bytes + 8), replace=False))
        out = {k: a[rows] for k, a in out.items()}
        out["rows"] = rows.astype(np.float64)
    os.makedirs(d, exist_ok=True)
    for k, a in out.items():
        np.save(os.path.join(d, k + ".npy"), a)


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks here (torch.distributed.run, one rank per GPU,
    rendezvous on 127.0.0.1 at a free port) with the same command line.  The ranks inherit stdout / stderr, so rank 0's single JSON line is
    this command's JSON line; the exit code is the launcher's."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")               # dmabuf IPC: what RCCL needs between processes on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // args.gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)


def via_group(args):
    """--via-group: the same metric through the C ABI's own sharding (pr_group: one process drives all GPUs, RCCL in-process).  The call takes
    HOST query buffers (it is the drop-in form of run_test.m:25-57), so the 39 MB of queries cross PCIe in every step: reported as its own
    line, never as the headline value."""
    import numpy as np
    from so_dso_place_recognition_amd import synth
    from so_dso_place_recognition_amd.api import Group
    n, m = args.db, args.queries
    db = synth.sc_database(45, n)
    q, planted = synth.sc_queries(46, np.empty((0, 2400)), m, db_first=0, n_global=n, db_seed=45)
    g = Group(list(range(args.gpus)))
    g.set_database("sc", db)
    for _ in range(args.warmup):
        g.match_topk(q, 0, 2.0, 1)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        idx, sc = g.match_topk(q, 0, 2.0, 1)
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, idx=idx, score=sc)
    out = {"metric": "queries/sec over 100k-signature DB (SC 20x60, z-score fusion, top-1), through pr_group (C ABI, host query buffers)",
           "value": m * args.steps / dt, "unit": "queries/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f16x2 (fp32 carried as f16 hi + lo, fp32 accumulate)", "data": "synthetic"}
    if args.full:
        g.set_timing(True)                                         # one more step with events between the phases on every shard's stream
        g.match_topk(q, 0, 2.0, 1)
        per_rank = []
        for r, ph in enumerate(g.last_timing()):
            coll_ms = sum(v for kk, v in ph.items() if kk.startswith("all_gather"))
            rows = n * (r + 1) // args.gpus - n * r // args.gpus
            per_rank.append({"rank": r, "db_rows": rows, "shard_fraction": rows / n, "phases_ms": ph, "collective_ms": coll_ms,
                             "compute_ms": sum(ph.values()) - coll_ms, "matcher_ns_per_pair": 1e6 * ph["distances"] / (m * rows)})
        g.set_timing(False)
        out.update({"collective": {"backend": "rccl (in-process, ncclCommInitAll)" if g.uses_rccl else "device copies", "world": args.gpus,
                                   "rccl_ranks_seen": g.rccl_ranks, "exchange_selftest": "passed at pr_group_create" if args.gpus > 1 else None},
                    "per_rank": per_rank, "flagged_queries_last_step": g.last_flagged})
    out["config"] = {"workload": "sc_match_100k", "db_signatures": n, "queries_per_step": m, "via": "pr_group_match_topk",
                     "uses_rccl": g.uses_rccl, "note": "DB packed once (pr_group_set_database); queries host -> every GPU per step"}
    if args.full:
        out["parity"] = {"planted_top1_correct": int((idx[:, 0] == planted).sum()), "queries": m}
    print(json.dumps(out), flush=True)
    g.close()


def kitti_shape(dev, ev, args, with_cpu):
    """The reference's own operating point (match_signatures/test_kitti.m:19-20: mask_width 100, loop_diff 10 m; KITTI seq00 = 3475 keyframes,
    run_test.m:25-57 matches the sequence against itself): m = n = 3475 SC signatures GENERATED from a synthetic drive - two laps of a
    circuit, consecutive clouds nearly equal, three stretches where the vehicle stands still (clusters of near-copies: what the containment
    check of the matcher exists for) - matched by one Matcher step, with the number of queries the checks hand to the exact fp64 rows, the
    same call as a captured hipGraph (chained resolution passes: no 64-query cap, no warning), run_test.m's precision / recall figures, and
    the oracle's FULL chain (pr_ref_match_topk: all 3475 x 3475 x 120 variants in fp64, not a sample) timed on this host's cores beside it."""
    import numpy as np
    import torch
    from so_dso_place_recognition_amd import _lib, api, eval as pr_eval, synth
    from so_dso_place_recognition_amd.api import Context
    from so_dso_place_recognition_amd.matcher import Matcher
    N, MASK, LOOP = 3475, 100, 10.0
    stops = ((400, 60), (1500, 40), (2600, 80))
    cur = int(torch.cuda.current_stream(dev).cuda_stream)
    t0 = time.perf_counter()
    xyz, it, offs, lap, pos = synth.drive_clouds_torch(N, 6000, 5, stops=stops, device=dev, positions=True)
    draw_s = time.perf_counter() - t0
    ctx = Context(dev.index, stream=cur)
    t0 = time.perf_counter()
    sig_h = api.sc_generate(xyz, it, offs, ctx=ctx)                       # [N, 2400] f64 (host buffers in, host buffer out: the CLI's path)
    gen_s = time.perf_counter() - t0
    sig = torch.from_numpy(sig_h).to(dev)
    mt = Matcher("sc", N, N, ctx=ctx)

    def step(**kw):
        mt.pack_database(sig)
        return mt.match(sig, MASK, 2.0, 1, **kw)
    step(); step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        idx, sc = step()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / 5
    idx_h, sc_h = idx.cpu().numpy()[:, 0].copy(), sc.cpu().numpy()[:, 0].copy()
    warn = mt.take_warnings()
    # phases of one more step (events on the stream), the flagged count of the same call without the resolution
    marks = []

    def mark(name):
        e = ev.create(); ev.record(e, mt.ctx.stream); marks.append((name, e))
    mark("start"); mt.pack_database(sig); mark("pack(db)"); mt.match(sig, MASK, 2.0, 1, mark=mark); mark("end")
    torch.cuda.synchronize()
    phases = {}
    for (_, a), (name, b_) in zip(marks[:-1], marks[1:]):
        phases[name] = phases.get(name, 0.0) + ev.elapsed_ms(a, b_)
    mt.match(sig, MASK, 2.0, 1, exact_order=False)
    flagged = mt.flagged_count()
    out = {"note": "test_kitti.m:19-20's operating point on a synthetic drive of KITTI seq00's size: self-match m = n = 3475 generated SC signatures, "
                   "mask_width 100, loop_diff 10 m, k = 1; stops = standing-still stretches (first frame, frames)",
           "frames": N, "points_per_cloud": 6000, "stops": [list(s_) for s_ in stops], "lap_frames": int(lap), "mask_width": MASK, "loop_diff_m": LOOP,
           "drive_draw_s": draw_s, "sc_generate_s_host_buffers": gen_s,
           "ms_per_step": ms, "queries_per_s": N / (ms * 1e-3), "ms_per_query": ms / N,
           "queries_flagged_for_exact_rows": int(flagged), "phases_ms": phases, "exact_rows_ms": phases.get("exact rows (one shard)"),
           "warnings_after_the_steps": int(warn), "order_unresolved_warning": bool(warn & _lib.WARN_ORDER_UNRESOLVED)}
    auc, top_recall, lp = pr_eval.precision_recall(sc_h, idx_h, pos, pos, LOOP, MASK)[:3]
    out.update({"auc": float(auc), "top_recall": float(top_recall), "loops_detected_at_full_precision": int(len(lp))})
    # the same call with fp64 row statistics for every query (what api.run_test uses for the sweep: every score the reference's double)
    mx = Matcher("sc", N, N, ctx=Context(dev.index, exact_statistics=True, stream=cur))
    mx.pack_database(sig)
    mx.match(sig, MASK, 2.0, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xi, xs = mx.match(sig, MASK, 2.0, 1)
    torch.cuda.synchronize()
    out["ms_per_step_exact_statistics_every_query"] = 1e3 * (time.perf_counter() - t0)
    xi_h, xs_h = xi.cpu().numpy()[:, 0].copy(), xs.cpu().numpy()[:, 0].copy()
    mx.close()
    xauc, xtr, xlp = pr_eval.precision_recall(xs_h, xi_h, pos, pos, LOOP, MASK)[:3]
    out.update({"auc_exact_statistics": float(xauc), "top_recall_exact_statistics": float(xtr), "top1_equal_default_vs_exact_statistics": bool((xi_h == idx_h).all())})
    try:    # the same call as ONE captured hipGraph: 3475 > 64 queries -> ceil(m / 64) resolution passes chained on the stream, no read-back
        mg = Matcher.on_new_stream("sc", N, N, device=dev.index)
        with torch.cuda.stream(mg.stream):
            mg.pack_database(sig)
        cap = mg.capture(sig.clone(), MASK, 2.0, 1)
        for _ in range(2):
            cap.run()
        t0 = time.perf_counter()
        for _ in range(5):
            cap.run()
        gms = 1e3 * (time.perf_counter() - t0) / 5
        gw = mg.take_warnings()
        out["hipgraph_replay"] = {"ms_per_replay": gms, "resolution_passes_chained": (N + 63) // 64, "warnings": int(gw),
                                  "order_unresolved_warning": bool(gw & _lib.WARN_ORDER_UNRESOLVED), "order_resolved_warning": bool(gw & _lib.WARN_ORDER_RESOLVED),
                                  "top1_equal_stepwise": bool((cap.idx.cpu().numpy()[:, 0] == idx_h).all()),
                                  "max_abs_score_diff_vs_stepwise": float(np.abs(cap.score.cpu().numpy()[:, 0] - sc_h).max())}
        mg.close()
    except Exception as e:
        out["hipgraph_replay"] = {"error": repr(e)[:300]}
    mt.close()
    if with_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib                                           # the checker: CPU port of the reference (after every timed GPU region)
        cores = os.cpu_count() or 1
        C.CDLL("libgomp.so.1").omp_set_num_threads(cores)
        t0 = time.perf_counter()
        rc, oidx, osc = oracle_lib.match_topk(0, sig_h, sig_h, MASK, 2.0, 1)
        cdt = time.perf_counter() - t0
        o = oracle_lib.precision_recall(osc[:, 0], oidx[:, 0], pos, pos, LOOP, MASK)
        err = np.abs(sc_h - osc[:, 0])
        fin = np.isfinite(osc[:, 0])
        out["cpu_chain"] = {"kind": "port", "what": "oracle/pr_ref.cpp pr_ref_match_topk: the whole 3475 x 3475 self-match (processSC.m:15-33 dense 120-variant fp64 + "
                                    "run_test.m:38-57), un-sampled", "threads": cores, "seconds": cdt, "queries_per_s": N / cdt,
                            "ms_per_query": 1e3 * cdt / N, "gpu_step_speedup": cdt / (ms * 1e-3),
                            "top1_equal": bool((oidx[:, 0] == idx_h).all()), "top1_equal_exact_statistics": bool((oidx[:, 0] == xi_h).all()),
                            "max_abs_score_err": float(err[fin].max()), "max_abs_score_err_exact_statistics": float(np.abs(xs_h - osc[:, 0])[fin].max()),
                            "oracle_auc": o["auc"], "oracle_top_recall": o["top_recall"],
                            "auc_equal": bool(o["auc"] == float(auc)), "top_recall_equal": bool(o["top_recall"] == float(top_recall)),
                            "auc_equal_exact_statistics": bool(o["auc"] == float(xauc)), "top_recall_equal_exact_statistics": bool(o["top_recall"] == float(xtr))}
    return out


def extra_workloads(dev, ev, args):
    """Secondary workloads of BASELINE.json, measured after (outside) the timed region on the same GPU."""
    import numpy as np
    import torch
    from so_dso_place_recognition_amd import synth
    from so_dso_place_recognition_amd.api import Context
    from so_dso_place_recognition_amd.matcher import Matcher
    P = lambda t: C.c_void_p(t.data_ptr())
    out = {}
    cur = int(torch.cuda.current_stream(dev).cuda_stream)

    def timed(ctx, fn, reps=3):
        ts = []
        for _ in range(reps + 1):
            a, b = ev.create(), ev.create()
            ev.record(a, ctx.stream); fn(); ev.record(b, ctx.stream)
            ts.append(ev.elapsed_ms(a, b))
        return float(np.mean(ts[1:]))

    # config 3: M2DP 192-d x 2 channels, 4 x 4 sign variants, 50k-signature DB, 4096 queries
    n, m = 50_000, 4096
    db = synth.m2dp_database_torch(43, n, device=dev)
    q_h, planted = synth.m2dp_queries(44, db.cpu().numpy(), m)
    q = torch.from_numpy(q_h).to(dev)
    mt = Matcher("m2dp", m, n, ctx=Context(dev.index, stream=cur))
    pair = [ev.create(), ev.create()]
    kms = []

    def m2_step():
        mt.pack_database(db)
        mt.pre_distances = lambda: ev.record(pair[0], mt.ctx.stream)
        mt.post_distances = lambda: ev.record(pair[1], mt.ctx.stream)
        return mt.match(q, 0, 2.0, 1)
    m2_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        idx, _ = m2_step()
        kms.append(ev.elapsed_ms(pair[0], pair[1]))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 5
    f16 = mt.ctx.sc_arith == "f16x2"
    fpp = 12288 * (3 if f16 else 1)
    k = float(np.mean(kms))
    out["m2dp_match_50k"] = {"queries_per_s": m / dt, "ms_per_step": 1e3 * dt, "kernel": "m2dp_match_h_kernel" if f16 else "m2dp_match_kernel",
                             "ms_per_launch": k, "flop_per_pair": fpp, "achieved_TFLOPs": m * n * fpp / (k * 1e-3) / 1e12,
                             "frac_of_mfma_peak": m * n * fpp / (k * 1e-3) / 1e12 / (MFMA_F16_PEAK_TFLOPS if f16 else MFMA_F32_PEAK_TFLOPS),
                             "planted_top1_correct": int((idx.cpu().numpy()[:, 0] == planted).sum()), "queries": m,
                             # what a loop of nothing but v_mfma_f32_32x32x16_f16 sustains with split-f16-like operands on this chip (power-limited
                             # clock): tools/ubench/mfma_power.hip, profiles/r06_mfma_power_box{A,B}.txt - a committed measurement, DESIGN.md section 4
                             "sustained_mfma_ceiling_frac_of_peak": 0.67 if f16 else None,
                             "frac_of_sustained_mfma_ceiling": (m * n * fpp / (k * 1e-3) / 1e12 / (0.67 * MFMA_F16_PEAK_TFLOPS)) if f16 else None}
    mt.close(); del db, q, mt
    torch.cuda.empty_cache()
    # config 2: SC / M2DP generation from 50 000-point clouds resident in HBM
    N, PTS = 1024, 50_000
    xyz, it, offs = synth.scene_clouds_torch(42, N, PTS, device=dev)
    ctx = Context(dev.index, stream=cur)
    sig = torch.empty((N, 2400), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ms = timed(ctx, lambda: ctx.check(ctx.lib.pr_sc_generate_dev(ctx.h, P(xyz), P(it), P(offs), N, 45.0, P(sig))))
    by = N * (28 * PTS + 19200)
    out["sc_generate_50k_pts"] = {"clouds": N, "points_per_cloud": PTS, "ms": ms, "clouds_per_s": N / (ms * 1e-3), "bound": "hbm",
                                  "algorithmic_bytes_per_cloud": 28 * PTS + 19200, "achieved_GBps": by / (ms * 1e-3) / 1e9,
                                  "frac_of_8TBps": by / (ms * 1e-3) / 8e12}
    # the same with the PCA frames supplied by the caller (what the GPU pre-stage leaves beside the clouds it emits): binning pass only
    fr = torch.empty((N, 16), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.pr_cloud_frames_dev(ctx.h, P(xyz), P(it), P(offs), N, P(fr)))        # frames + the float intensity averages
    ctx.sync()
    ms_chain = timed(ctx, lambda: ctx.check(ctx.lib.pr_sc_generate_frames_dev(ctx.h, P(xyz), P(it), P(offs), N, 45.0, P(fr), 0, P(sig))))
    ms = timed(ctx, lambda: ctx.check(ctx.lib.pr_sc_generate_frames_dev(ctx.h, P(xyz), P(it), P(offs), N, 45.0, P(fr), 1, P(sig))))
    out["sc_generate_50k_pts_frames_given"] = {"clouds": N, "points_per_cloud": PTS, "ms": ms, "clouds_per_s": N / (ms * 1e-3), "bound": "hbm",
                                               "algorithmic_bytes_per_cloud": 28 * PTS + 19200, "achieved_GBps": by / (ms * 1e-3) / 1e9,
                                               "frac_of_8TBps": by / (ms * 1e-3) / 8e12,
                                               "ms_when_the_call_computes_the_averages": ms_chain,
                                               "note": "pr_sc_generate_frames_dev with the frames AND float averages of pr_cloud_frames_dev / the GPU pre-stage: the "
                                                       "binning pass alone; without the averages their chain of dependent float adds runs beside it"}
    del fr
    Nm = 128
    sigm = torch.empty((4 * Nm, 384), dtype=torch.float64, device=dev)
    ms = timed(ctx, lambda: ctx.check(ctx.lib.pr_m2dp_generate_dev(ctx.h, P(xyz), P(it), P(offs), Nm, 45.0, P(sigm))), reps=2)
    # "report projections/s and % VALUBusy".  VALU lane-instructions per plane projection from the committed PMC passes of this command
    # (profiles/r06_final_derived.json: SQ_INSTS_VALU of m2dp_bin_kernel per launch of 256 clouds x 64 lanes / its projections), priced against the
    # chip's VALU issue peak: 1024 SIMDs x 16 lanes x 2.4 GHz = 39.3 T lane-instructions/s
    ipp = busy = None
    try:
        dk = json.load(open(os.path.join(ROOT, "profiles", "r06_final_derived.json")))["kernels"]
        e_ = next(v for kk, v in dk.items() if kk.startswith("m2dp_bin_kernel<16> @ 1048576"))
        ipp, busy = e_["insts_valu"] * 64.0 / (256.0 * PTS * 256.0), e_.get("valu_busy")
    except Exception:
        pass
    VALU_PEAK = 1024 * 16 * 2.4e9

    def m2gen(clouds, ms_):
        pps = clouds * 256 * PTS / (ms_ * 1e-3)
        return {"clouds": clouds, "points_per_cloud": PTS, "ms": ms_, "clouds_per_s": clouds / (ms_ * 1e-3), "plane_projections_per_s": pps,
                "bound": "valu (fp64 dots + polar classification), not HBM", "valu_lane_instructions_per_projection": ipp,
                "frac_of_valu_issue_peak": (pps * ipp / VALU_PEAK) if ipp else None, "valu_busy_of_m2dp_bin_kernel": busy,
                "frac_source": "profiles/r06_final_derived.json (a committed PMC measurement of one box, not a live counter); whole call = m2dp_bin + m2dp_svd + frames"}
    out["m2dp_generate_50k_pts"] = m2gen(Nm, ms)
    sigm = torch.empty((4 * N, 384), dtype=torch.float64, device=dev)
    ms = timed(ctx, lambda: ctx.check(ctx.lib.pr_m2dp_generate_dev(ctx.h, P(xyz), P(it), P(offs), N, 45.0, P(sigm))), reps=2)
    out["m2dp_generate_50k_pts_1024_clouds"] = m2gen(N, ms)
    ctx.close(); del xyz, it, offs, sig, sigm
    torch.cuda.empty_cache()
    # the fp32-MFMA arithmetic of the SC matcher on the metric workload (one launch)
    n, m = args.db, args.queries
    db = synth.sc_database_torch(45, n, device=dev)
    q_h, planted = synth.sc_queries(46, np.empty((0, 2400)), m, db_first=0, n_global=n, db_seed=45)
    q = torch.from_numpy(q_h).to(dev)
    mt = Matcher("sc", m, n, ctx=Context(dev.index, sc_arith="f32", stream=cur))
    mt.pack_database(db)
    kms = []
    mt.pre_distances = lambda: ev.record(pair[0], mt.ctx.stream)
    mt.post_distances = lambda: ev.record(pair[1], mt.ctx.stream)
    for _ in range(2):
        idx, _ = mt.match(q, 0, 2.0, 1)
        kms.append(ev.elapsed_ms(pair[0], pair[1]))
    k = kms[-1]
    out["sc_match_100k_f32_arith"] = {"kernel": "sc_match_kernel", "ms_per_launch": k, "flop_per_pair": FLOP_PER_PAIR,
                                      "achieved_TFLOPs": m * n * FLOP_PER_PAIR / (k * 1e-3) / 1e12,
                                      "frac_of_fp32_mfma_peak": m * n * FLOP_PER_PAIR / (k * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS,
                                      "planted_top1_correct": int((idx.cpu().numpy()[:, 0] == planted).sum()), "queries": m}
    mt.close()
    # the metric workload with the binary-channel path switched off (pr_set_sc_binary(ctx, 0): both channels in ONE split-f16 launch, the
    # default until the second session of round 4) - what a DB whose intensity channel is not binary costs, and the figure of earlier rounds
    mt = Matcher("sc", m, n, ctx=Context(dev.index, sc_arith="f16x2", sc_binary=False, stream=cur))
    mt.pre_distances = lambda: ev.record(pair[0], mt.ctx.stream)
    mt.post_distances = lambda: ev.record(pair[1], mt.ctx.stream)
    kms = []

    def split_step():
        mt.pack_database(db)
        return mt.match(q, 0, 2.0, 1)
    split_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        idx, _ = split_step()
        kms.append(ev.elapsed_ms(pair[0], pair[1]))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 4
    k = float(np.mean(kms))
    out["sc_match_100k_split_f16_both_channels"] = {"queries_per_s": m / dt, "ms_per_step": 1e3 * dt, "kernel": "sc_match_e_kernel<split-f16>, both channels",
                                                    "ms_per_launch": k, "flop_per_pair": FLOP_PER_PAIR_F16X2,
                                                    "frac_of_f16_mfma_peak": m * n * FLOP_PER_PAIR_F16X2 / (k * 1e-3) / 1e12 / MFMA_F16_PEAK_TFLOPS,
                                                    "planted_top1_correct": int((idx.cpu().numpy()[:, 0] == planted).sum()), "queries": m}
    mt.close()
    # PR_SC_ARITH_F16 (BASELINE config 5's "fp16 descriptors": one f16 per value, one MFMA per product) on the metric workload: whole steps
    # (pack(q) + pack(db) + distances + moments + select(k + 56) + fp64 re-evaluation + margin check + split-f16 fallback of flagged queries)
    mt = Matcher("sc", m, n, ctx=Context(dev.index, sc_arith="f16", stream=cur))
    mt.pre_distances = lambda: ev.record(pair[0], mt.ctx.stream)
    mt.post_distances = lambda: ev.record(pair[1], mt.ctx.stream)
    kms = []

    def f16_step():
        mt.pack_database(db)
        return mt.match(q, 0, 2.0, 1)
    f16_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        idx, _ = f16_step()
        kms.append(ev.elapsed_ms(pair[0], pair[1]))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 5
    k = float(np.mean(kms))
    out["sc_match_100k_f16_arith"] = {"queries_per_s": m / dt, "ms_per_step": 1e3 * dt, "kernel": "sc_match_e_kernel<single product>", "ms_per_launch": k,
                                      "flop_per_pair": FLOP_PER_PAIR, "achieved_TFLOPs": m * n * FLOP_PER_PAIR / (k * 1e-3) / 1e12,
                                      "frac_of_f16_mfma_peak": m * n * FLOP_PER_PAIR / (k * 1e-3) / 1e12 / MFMA_F16_PEAK_TFLOPS,
                                      "packed_db_bytes_per_entry": 2 * 2976, "queries_recomputed_in_split_f16": int(mt.f16_fallbacks),
                                      "planted_top1_correct": int((idx.cpu().numpy()[:, 0] == planted).sum()), "queries": m}
    # the same arithmetic at k = 5 (what the margin / order checks of the f16 pass hand to the split-f16 twin when the list reaches
    # into a row's dense part, and what that costs a step - the twin's DB pack is part of the first such step only)
    try:
        f16_step(); mt.match(q, 0, 2.0, 5); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            mt.pack_database(db)
            idx5, _ = mt.match(q, 0, 2.0, 5)
        torch.cuda.synchronize()
        out["sc_match_100k_f16_arith"]["k=5"] = {"ms_per_step": 1e3 * (time.perf_counter() - t0) / 3, "queries_recomputed_in_split_f16_per_step": int(mt.f16_fallbacks),
                                                  "planted_top1_correct": int((idx5.cpu().numpy()[:, 0] == planted).sum())}
    except Exception as e:
        out["sc_match_100k_f16_arith"]["k=5"] = {"error": repr(e)[:200]}
    mt.close(); del mt
    torch.cuda.empty_cache()
    # BASELINE config 5, one GPU's share: fused SC + M2DP scoring, 125 000 of the 1 M signatures (an 8-GPU shard), f16 descriptors
    from so_dso_place_recognition_amd.matcher import FusedMatcher
    ns = 125_000
    dbs = synth.sc_database_torch(71, ns, device=dev)
    dbm = synth.m2dp_database_torch(73, ns, device=dev)
    qs_h, pl5 = synth.sc_queries(72, np.empty((0, 2400)), m, db_first=0, n_global=ns, db_seed=71)
    qm_h = np.concatenate([synth.m2dp_queries(74 + 0 * i, synth.m2dp_database(73, 1, first=int(e)), 1)[0] for i, e in enumerate(pl5[:256])])
    qm_h = np.tile(qm_h, (m // 256, 1))                                          # M2DP queries: 256 planted rows repeated (timing only needs the shape)
    qs, qm = torch.from_numpy(qs_h).to(dev), torch.from_numpy(qm_h).to(dev)
    fm = FusedMatcher(m, ns, ctx=Context(dev.index, sc_arith="f16", stream=cur))
    pair2 = [ev.create(), ev.create()]
    fm.sc.pre_distances = lambda: ev.record(pair[0], fm.ctx.stream)
    fm.sc.post_distances = lambda: ev.record(pair[1], fm.ctx.stream)
    fm.m2.pre_distances = lambda: ev.record(pair2[0], fm.ctx.stream)
    fm.m2.post_distances = lambda: ev.record(pair2[1], fm.ctx.stream)

    def fused_step():
        fm.pack_database(dbs, dbm)
        return fm.match(qs, qm, 0, 2.0, 1)
    fused_step()
    torch.cuda.synchronize()
    ks, km = [], []
    t0 = time.perf_counter()
    for _ in range(5):
        idx, _ = fused_step()
        ks.append(ev.elapsed_ms(pair[0], pair[1])); km.append(ev.elapsed_ms(pair2[0], pair2[1]))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 5
    ks, km = float(np.mean(ks)), float(np.mean(km))
    out["fused_1m_shard_fp16"] = {"note": "BASELINE config 5, the per-GPU share of 1 M signatures over 8 GPUs: SC + M2DP, four z-scores, f16 descriptors, "
                                          "k + 56 candidates re-evaluated in fp64, margin check, split-f16 fallback",
                                  "db_rows": ns, "queries": m, "queries_per_s": m / dt, "ms_per_step": 1e3 * dt,
                                  "sc_kernel_ms": ks, "sc_frac_of_f16_mfma_peak": m * ns * FLOP_PER_PAIR / (ks * 1e-3) / 1e12 / MFMA_F16_PEAK_TFLOPS,
                                  "m2dp_kernel_ms": km, "m2dp_frac_of_f16_mfma_peak": m * ns * 12288 / (km * 1e-3) / 1e12 / MFMA_F16_PEAK_TFLOPS,
                                  "queries_recomputed_in_split_f16": int(fm.f16_fallbacks),
                                  "planted_top1_correct": int((idx.cpu().numpy()[:, 0] == pl5).sum())}
    fm.close(); del fm, dbs, dbm, qs, qm
    torch.cuda.empty_cache()
    # online use (one keyframe at a time against a resident, already packed DB): wall time per call, host launch overhead included.
    # The floor of such a call is one read of the packed DB image from HBM: 2 channels x ceil(n / 16) groups x 95 232 B (split-f16) or
    # 47 616 B (one f16 per value); frac_of_8TBps prices the WHOLE call (pack(q) .. re-evaluation, ~10 launches) against that read at 8 TB/s.
    lat = {}
    for arith_l, gbytes in (("f16x2", 95232), ("f16", 47616)):
        mt = Matcher("sc", 64, n, ctx=Context(dev.index, sc_arith=arith_l, stream=cur))
        mt.pack_database(db)
        img = 2 * ((n + 15) // 16) * gbytes
        for mq in (1, 8, 16, 32, 64):
            qq = q[:mq].contiguous()
            for _ in range(3):
                mt.match(qq, 0, 2.0, 1)
            torch.cuda.synchronize()
            if arith_l == "f16x2":      # the binary path reads the structure channel's image and the hi tiles - half - of the other
                stb = C.c_int32(0)
                mt.ctx.check(mt.lib.pr_sc_binary_state(mt.ctx.h, mt.q, mt.db, C.byref(stb)))
                img = ((n + 15) // 16) * (gbytes + (gbytes // 2 if stb.value == 1 else gbytes))
            t0 = time.perf_counter()
            for _ in range(20):
                idx, _ = mt.match(qq, 0, 2.0, 1)
                torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / 20
            lat[f"m={mq}" + ("" if arith_l == "f16x2" else " f16")] = {"ms_per_call": ms, "hbm_bytes": img, "frac_of_8TBps": img / (ms * 1e-3) / 8e12,
                                                                       "top1_correct": int((idx.cpu().numpy()[:, 0] == planted[:mq]).sum())}
        mt.close()
    out["sc_match_100k_latency"] = {"note": "pack(q) + distances + moments + select + fp64 re-evaluation (+ margin check in f16), DB resident and packed, "
                                            "synchronised per call; hbm_bytes = one read of the packed DB image (with a binary intensity channel: of its hi tiles only)", **lat}
    # the online LOOP (SC/test_sc.cpp:40-56 + run_test.m:57 per keyframe): the keyframe is matched against the DB so far, then appended
    # to it IN PLACE (pr_sigset_reserve / pr_sigset_append: capacity geometry, one pack kernel per row, statistics folded in) - until round 6 a
    # DB change was a full re-pack (1.1 ms at 100k) + re-upload
    try:
        mo = Matcher("sc", 8, n + 256, ctx=Context(dev.index, stream=cur))
        mo.reserve_database(db)
        fresh = synth.sc_database_torch(47, 64, device=dev)
        for i in range(4):
            mo.append_database(fresh[i:i + 1]); mo.match(q[i:i + 1].contiguous(), 0, 2.0, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(4, 24):
            mo.append_database(fresh[i:i + 1])
            torch.cuda.synchronize()
        app_ms = 1e3 * (time.perf_counter() - t0) / 20
        ok = 0
        t0 = time.perf_counter()
        for i in range(24, 44):
            idx, _ = mo.match(q[i:i + 1].contiguous(), 0, 2.0, 1)
            mo.append_database(fresh[i:i + 1])
            torch.cuda.synchronize()
            ok += int(idx.cpu().numpy()[0, 0] == planted[i])
        loop_ms = 1e3 * (time.perf_counter() - t0) / 20
        out["sc_online_loop"] = {"note": "per keyframe: match(1) against the resident 100k-signature DB, then append(1) in place (raw row + operand row), synchronised",
                                 "db_rows": int(mo.n), "ms_per_keyframe": loop_ms, "append_ms_synchronised": app_ms, "top1_correct": ok, "keyframes": 20}
        mo.close(); del mo, fresh
    except Exception as e:
        out["sc_online_loop"] = {"error": repr(e)[:300]}
    try:   # the same call replayed as one hipGraph
        mg = Matcher.on_new_stream("sc", 8, n, device=dev.index)
        with torch.cuda.stream(mg.stream):
            mg.pack_database(db)
        q1 = q[:1].clone()
        cap = mg.capture(q1, 0, 2.0, 1)
        for _ in range(3):
            cap.run()
        t0 = time.perf_counter()
        for _ in range(20):
            cap.run()
        ms = 1e3 * (time.perf_counter() - t0) / 20
        stb = C.c_int32(0)
        mg.ctx.check(mg.lib.pr_sc_binary_state(mg.ctx.h, mg.q, mg.db, C.byref(stb)))
        img = ((n + 15) // 16) * (95232 + (47616 if stb.value == 1 else 95232))
        out["sc_match_100k_latency"]["m=1 hipGraph replay"] = {"ms_per_call": ms, "hbm_bytes": img, "frac_of_8TBps": img / (ms * 1e-3) / 8e12,
                                                                "top1_correct": int((cap.idx.cpu().numpy()[:, 0] == planted[:1]).sum())}
        mg.close()
    except Exception as e:   # graph capture is an extra, never a reason to lose the bench line
        out["sc_match_100k_latency"]["m=1 hipGraph replay"] = {"error": repr(e)[:200]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--db", type=int, default=100_000, help="total DB signatures (sharded over the ranks)")
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what the headline figure does not need: roofline, parity, collective, "
                         "per_rank, cpu_baseline and extra (a plain run sets up, warms up, times the steps, dumps and prints the line)")
    ap.add_argument("--cpu-sample", type=int, default=-1, help="queries for the CPU baseline (-1: one per host core, <= 64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline and the oracle's entries of parity")
    ap.add_argument("--sc-arith", default=None, choices=["f16x2", "f32", "f16"],
                    help="SC matcher arithmetic (default: the library's, split-f16 MFMA; f32 = the fp32-MFMA kernel; f16 = one f16 product per term)")
    ap.add_argument("--via-group", action="store_true",
                    help="ONE process drives --gpus GPUs through pr_group (C ABI, in-process RCCL) instead of one torch.distributed rank per GPU")
    ap.add_argument("--force-exchange", action="store_true",
                    help="N = 1 only: run the two all-gathers (RCCL, one-rank group) and the device merge of the sharded protocol anyway")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the secondary workloads reported under `extra`")
    ap.add_argument("--no-kitti-shape", action="store_true", help="with --full: skip extra.kitti_shape (its drive sampler is ~70 000 torch launches: slow under rocprofv3 --pmc)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (gloo: several ranks on ONE GPU, tests only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the top-k indices and scores of the last timed step to DIR/idx.npy and DIR/score.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.via_group:
        return via_group(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args)

    import numpy as np
    import torch
    import torch.distributed as dist

    from so_dso_place_recognition_amd import synth
    from so_dso_place_recognition_amd.matcher import Matcher

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.backend == "gloo":
        local = 0                                              # all ranks share cuda:0
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    if args.backend == "nccl" and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py --gpus {world}: only {torch.cuda.device_count()} HIP device(s) visible (one rank per GPU)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if args.force_exchange and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)

    n, m = args.db, args.queries
    lo, hi = (n * rank) // world, (n * (rank + 1)) // world          # this rank's DB rows
    t0 = time.time()
    db = synth.sc_database_torch(45, hi - lo, first=lo, device=dev)   # f64 [n_local, 2400] drawn in HBM (== synth.sc_database bit for bit)
    db_host = db.cpu().numpy() if (args.full and rank == 0 and world == 1 and not args.no_cpu_baseline) else None
    q_host, planted = synth.sc_queries(46, np.empty((0, 2400)), m, db_first=0, n_global=n, db_seed=45)
    q = torch.from_numpy(q_host).to(dev)                              # f64 [m, 2400]
    gen_s = time.time() - t0

    from so_dso_place_recognition_amd.api import Context
    # the library context lives on torch's current stream: its kernels, torch's buffers and RCCL's collectives are ordered by
    # the stream, a step has no host synchronisation (pr_create_on_stream)
    mt = Matcher("sc", m, hi - lo, ctx=Context(local, sc_arith=args.sc_arith, stream=int(torch.cuda.current_stream(dev).cuda_stream)))
    arith = mt.ctx.sc_arith
    ev = HipEvents()
    evs = [(ev.create(), ev.create()) for _ in range(args.steps)]     # one pair per timed step, read after the timed region
    stream = mt.ctx.stream

    def step(pair):
        mt.pack_database(db)
        if pair is not None:   # the only launches between the two records are the matcher and the NaN fix-up, on the stream they run on
            mt.pre_distances = lambda: ev.record(pair[0], stream)
            mt.post_distances = lambda: ev.record(pair[1], stream)
        out = mt.match(q, 0, 2.0, 1, db_row0=lo, force_exchange=args.force_exchange)
        mt.pre_distances = mt.post_distances = None
        return out

    for _ in range(args.warmup):
        step(None)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        idx, score = step(evs[i])
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:   # now: the calls below reuse the matcher's output buffers
        dump_outputs(args.dump_outputs, idx=idx.cpu().numpy(), score=score.cpu().numpy())
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    # whether the steps took the binary path for the intensity channel: read from the packed sets' statistics, no launch
    st_bin = None
    if arith == "f16x2":
        st_bin = C.c_int32(0)
        mt.ctx.check(mt.lib.pr_sc_binary_state(mt.ctx.h, mt.q, mt.db, C.byref(st_bin)))
        st_bin = st_bin.value
    binary_path = st_bin == 1 and os.environ.get("PR_SC_KERNEL") != "h"     # (PR_SC_KERNEL=h: sc_match_h_kernel has no binary path)

    if args.full:
        kern_ms = [ev.elapsed_ms(a, b) for a, b in evs]
        # one more step, outside the timed region, with an event after every phase of the protocol on the stream everything runs on (the
        # library's kernels, torch's copies and RCCL's all-gathers share it): per-rank phase times, gathered to rank 0 below
        marks = []

        def mark(name):
            e = ev.create()
            ev.record(e, stream)
            marks.append((name, e))
        barrier()
        mark("start")
        mt.pack_database(db)
        mark("pack(db)")
        mt.match(q, 0, 2.0, 1, db_row0=lo, force_exchange=args.force_exchange, mark=mark)
        mark("end")
        torch.cuda.synchronize()
        phases = {}
        for (_, a), (name, b_) in zip(marks[:-1], marks[1:]):
            phases[name] = phases.get(name, 0.0) + ev.elapsed_ms(a, b_)
        coll_ms = sum(v for kk, v in phases.items() if kk.startswith("all_gather"))
        mine_rank = {"rank": rank, "db_rows": hi - lo, "shard_fraction": (hi - lo) / n, "phases_ms": phases, "collective_ms": coll_ms,
                     "compute_ms": sum(phases.values()) - coll_ms, "step_ms": ev.elapsed_ms(marks[0][1], marks[-1][1]),
                     "matcher_ns_per_pair": 1e6 * float(np.mean(kern_ms)) / (m * (hi - lo))}
        flagged = None
        if world == 1 and not args.force_exchange and arith != "f16":   # how many queries of a step the order / containment checks hand to the exact rows
            mt.match(q, 0, 2.0, 1, db_row0=lo, exact_order=False)
            flagged = mt.flagged_count()
        per_rank = [mine_rank]
        if world > 1:
            per_rank = [None] * world
            dist.all_gather_object(per_rank, mine_rank)
        # per-launch times of the matcher (pr_set_kernel_timing: the library's own events between its launches), outside the timed region
        launch_ms = None
        if arith == "f16x2":
            mt.ctx.kernel_timing(True)
            acc = []
            for _ in range(min(5, max(2, args.steps))):
                step(None)
                acc.append(mt.ctx.last_distance_timing())
            mt.ctx.kernel_timing(False)
            launch_ms = [float(np.mean([a[i] for a in acc])) for i in range(3)]

        idx_h = idx.cpu().numpy()[:, 0]
        score_h = score.cpu().numpy()[:, 0]
        planted_ok = int((idx_h == planted).sum())
        # what the communicator itself says (not argv): every rank contributes its rank through the group's own all-gather
        coll = {"backend": None, "world": 1, "rccl_ranks_seen": 0}
        if dist.is_available() and dist.is_initialized():
            on_dev = dist.get_backend() == "nccl"
            mine = torch.tensor([rank], dtype=torch.int32, device=dev if on_dev else "cpu")
            seen = torch.empty((dist.get_world_size(),), dtype=torch.int32, device=mine.device)
            dist.all_gather_into_tensor(seen, mine)
            coll = {"backend": "nccl (RCCL %s)" % ".".join(map(str, torch.cuda.nccl.version())) if on_dev else dist.get_backend(),
                    "world": dist.get_world_size(), "rccl_ranks_seen": len(set(seen.cpu().tolist())) if on_dev else 0}

    if rank == 0:
        out = {
            "metric": "queries/sec over 100k-signature DB (SC 20x60, z-score fusion, top-1)",
            "value": m * args.steps / dt, "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "ms_per_query": 1e3 * dt / (args.steps * m),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": {"f16x2": "f16x2 (fp32 carried as f16 hi + lo, fp32 accumulate)" + ("; binary intensity channel: one f16 product per term, rounded to its exact integer count" if binary_path else ""),
                      "f16": "f16 (one f16 per value, fp32 accumulate; exact top-k through fp64 re-evaluation)"}.get(arith, "f32"),
            "data": "synthetic",
            "config": {"workload": "sc_match_100k", "db_signatures": n, "queries_per_step": m, "descriptor": "SC 20x60 x 2 channels",
                       "mask_width": 0, "p_weight": 2.0, "k": 1, "db_rows_per_gpu": hi - lo,
                       "step": "pack(q)+pack(db)+distances+moments+select(k+8)+fp64 re-evaluation+order / containment checks+exact fp64 rows of flagged queries"
                               + ("+4 all_gathers+merge" if (world > 1 or args.force_exchange) else "")},
        }
        if args.full:
            kms = float(np.mean(kern_ms))
            pairs = m * (hi - lo)
            f16 = arith in ("f16x2", "f16")
            kname = {"h": "sc_match_h_kernel"}.get(os.environ.get("PR_SC_KERNEL", "e"), "sc_match_e_kernel") if f16 else "sc_match_kernel"
            if arith == "f16":
                kname = "sc_match_e_kernel<single product>"
            fpp, peak = (FLOP_PER_PAIR_F16X2 if arith == "f16x2" else FLOP_PER_PAIR, MFMA_F16_PEAK_TFLOPS) if f16 else (FLOP_PER_PAIR, MFMA_F32_PEAK_TFLOPS)
            kms_all = kms
            launches = None
            binary = launch_ms is not None and launch_ms[1] + launch_ms[2] > 0
            if binary:     # three launches: structure channel in split-f16 | intensity channel with one product per term + rounding | the same in split-f16
                # (one of the last two has left at once: the gate of DESIGN.md §4.0b).  The dominant kernel is the first one: one channel's FLOPs.
                fast = launch_ms[1] > launch_ms[2]
                kname = "sc_match_e_kernel<split-f16>, structure channel"
                fpp, kms = FLOP_PER_PAIR_F16X2 // 2, launch_ms[0]
                launches = [{"kernel": kname, "ms": launch_ms[0], "flop_per_pair": fpp, "frac": pairs * fpp / (launch_ms[0] * 1e-3) / 1e12 / peak},
                            {"kernel": "sc_match_e_kernel<single product on the hi halves + integer rounding>, intensity channel (binary)", "ms": launch_ms[1],
                             "flop_per_pair": FLOP_PER_PAIR // 2, "frac": (pairs * (FLOP_PER_PAIR // 2) / (launch_ms[1] * 1e-3) / 1e12 / peak) if fast else None},
                            {"kernel": "sc_match_e_kernel<split-f16>, intensity channel", "ms": launch_ms[2], "flop_per_pair": FLOP_PER_PAIR_F16X2 // 2,
                             "frac": None if fast else pairs * (FLOP_PER_PAIR_F16X2 // 2) / (launch_ms[2] * 1e-3) / 1e12 / peak}]
            ach = pairs * fpp / (kms * 1e-3) / 1e12
            traffic = None   # HBM bytes per launch from the committed PMC passes (FETCH_SIZE x2 on gfx950 + WRITE_SIZE)
            traffic_file = None
            for cand in (("r06_traffic.json", "r05_traffic.json", "r04b_traffic.json") if binary else ("r04_traffic.json", "r03_traffic.json")):   # the newest committed PMC passes of this command
                try:
                    tr = json.load(open(os.path.join(ROOT, "profiles", cand)))
                    if tr["workload"] == {"db": n, "queries": m, "n_gpus": world}:
                        traffic = next(v["hbm_bytes_per_launch"] for kk, v in tr.items() if kk.startswith(kname.split("<")[0]) and (arith != "f16") == ("<false" not in kk)
                                       and (not binary or v.get("launch") == "structure channel"))
                        traffic_file = cand
                        break
                except Exception:
                    pass
            out.update({
                "roofline": {"kernel": kname, "bound": "mfma", "achieved": ach, "peak": peak,
                             "unit": "TFLOP/s", "frac": ach / peak, "traffic": traffic,
                             "traffic_source": (f"profiles/{traffic_file}: rocprofv3 --pmc FETCH_SIZE (x2 on gfx950) + WRITE_SIZE passes of this command, per launch "
                                                "(a committed measurement of one box, not a live counter)" if traffic is not None else None),
                             "flop_per_pair": fpp, "pairs_per_launch": pairs, "ms_per_launch": kms,
                             "matcher_ms_per_step": kms_all, "launches": launches,
                             "binary_channel_state": st_bin,
                             # a loop of nothing but f16 MFMAs on split-f16-like operands sustains 0.66 - 0.68 of `peak` on this chip (it clocks against its
                             # power limit; zeros reach 0.98): tools/ubench/mfma_power.hip, profiles/r06_mfma_power_box{A,B}.txt (committed, not live)
                             "sustained_mfma_ceiling_frac_of_peak": 0.67 if f16 else None,
                             "frac_of_sustained_mfma_ceiling": (ach / peak / 0.67) if f16 else None,
                             # the same launch priced as the fp32 formulation it replaces (what an fp32-MFMA kernel would need)
                             "fp32_formulation_tflops": pairs * FLOP_PER_PAIR / (kms_all * 1e-3) / 1e12,
                             "fp32_formulation_frac_of_157.3": pairs * FLOP_PER_PAIR / (kms_all * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS,
                             "dense_equivalent_tflops": pairs * 576000 / (kms_all * 1e-3) / 1e12},
                "parity": {"planted_top1_correct": planted_ok, "queries": m, "queries_flagged_for_exact_rows": flagged},
                "collective": coll,
                # one instrumented step per rank (outside the timed region): where a step's time goes on every GPU - compute scales with
                # shard_fraction (compare matcher_ns_per_pair with the N = 1 line: the kernel's efficiency at the shard's size), the all-gathers do not
                "per_rank": per_rank,
            })
        out["setup_s"] = gen_s
        if args.full and world == 1 and not args.no_cpu_baseline:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import oracle_lib                                           # the checker: CPU port of the reference
            cores = os.cpu_count() or 1
            S = args.cpu_sample if args.cpu_sample > 0 else min(cores, 64)
            omp = C.CDLL("libgomp.so.1")
            omp.omp_set_num_threads(1)                                  # the reference itself is single-threaded (SC/test_sc.cpp:40-56, run_test.m)
            t0 = time.perf_counter()
            rc1, oidx1, osc1 = oracle_lib.match_topk(0, q_host[:1], db_host, 0, 2.0, 1)
            cdt1 = time.perf_counter() - t0
            omp.omp_set_num_threads(cores)
            t0 = time.perf_counter()
            rc, oidx, osc = oracle_lib.match_topk(0, q_host[:S], db_host, 0, 2.0, 1)
            cdt = time.perf_counter() - t0
            out["cpu_baseline"] = {"value": S / cdt, "unit": "queries/s", "cores": min(cores, S), "kind": "port", "nproc": cores,
                                   "value_1_thread": 1.0 / cdt1,
                                   "sample": f"{S} queries x full {n}-signature DB on {min(cores, S)} threads ({cdt:.1f} s) and 1 query on 1 thread "
                                             f"({cdt1:.1f} s), dense 120-variant fp64 (oracle/pr_ref.cpp)"}
            try:   # the reference matcher's own shape: one multithreaded dgemm per query and channel (processSC.m:30)
                bdt, btop, bthr = blas_baseline(q_host, db_host, S)
                out["cpu_baseline"]["blas"] = {"value": S / bdt, "unit": "queries/s", "threads": bthr, "top1_equal_oracle": bool((btop == oidx[:, 0]).all()),
                                               "tflops_fp64": S * 2 * 120 * 1200 * n * 2 / bdt / 1e12,
                                               "sample": f"{S} queries x full {n}-signature DB, numpy / OpenBLAS dgemm 120 x 1200 . 1200 x n per query and channel "
                                                         f"({bdt:.1f} s incl. the normalisation of hist2)"}
            except Exception as e:
                out["cpu_baseline"]["blas"] = {"error": repr(e)[:200]}
            err = np.abs(osc[:, 0] - score_h[:S])
            # the same sample with fp64 row statistics for every query (pr_set_exact_statistics; 2.3 ms per query, outside the timed region):
            # what is left of the score error when nothing of the fp32 pass enters the returned score
            mx = Matcher("sc", S, hi - lo, ctx=Context(local, sc_arith=args.sc_arith, exact_statistics=True,
                                                       stream=int(torch.cuda.current_stream(dev).cuda_stream)))
            mx.pack_database(db)
            xi, xs = mx.match(q[:S].contiguous(), 0, 2.0, 1, db_row0=lo)
            torch.cuda.synchronize()
            exact_err = float(np.abs(xs.cpu().numpy()[:, 0] - osc[:, 0]).max()) if S <= 64 and arith != "f16" else None
            exact_idx_ok = bool((xi.cpu().numpy()[:, 0] == oidx[:, 0]).all())
            mx.close()
            # up to which |z| the returned score is within a FLAT 1e-5 of the oracle's: the sample's planted matches sit at z ~ -160 where the fp32
            # pass's ~2e-7 relative sigma error is 3e-5 absolute; error model |err| <= c |z| with c fitted on the sample -> the |z| where it meets 1e-5
            zc = float((err / np.maximum(np.abs(osc[:, 0]), 1e-30)).max())
            out["parity"]["score_flat_1e5_up_to_z"] = (1e-5 / zc) if zc > 0 else None
            out["parity"].update({"oracle_queries": S, "oracle_top1_equal": bool((oidx[:, 0] == idx_h[:S]).all()),
                                  "oracle_max_abs_score_err": float(err.max()),
                                  "oracle_max_rel_score_err": float((err / np.abs(osc[:, 0])).max()),
                                  "oracle_max_abs_score_err_with_exact_statistics": exact_err,
                                  "oracle_top1_equal_with_exact_statistics": exact_idx_ok,
                                  "score_note": "planted matches sit at z ~ -160; the returned score is exact in the pair's distances (fp64 re-evaluation), "
                                                "its row statistics carry the fp32 pass's ~2e-7 relative error (DESIGN.md)"})
        if args.full and world == 1 and not args.no_extra:
            mt.close()
            del db, mt
            torch.cuda.empty_cache()
            out["extra"] = extra_workloads(dev, ev, args)
            try:
                if not args.no_kitti_shape:
                    out["extra"]["kitti_shape"] = kitti_shape(dev, ev, args, not args.no_cpu_baseline)
            except Exception as e:    # an extra, never a reason to lose the bench line
                out["extra"]["kitti_shape"] = {"error": repr(e)[:300]}
        print(json.dumps(out), flush=True)
    if world > 1 or args.force_exchange:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
