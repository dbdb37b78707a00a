#!/usr/bin/env python3
"""The ICP refinement (csrc/icp.hip) at two shapes: 64 pairs of 4096-point clouds (a batch of loop-closure candidates) and 1 pair of
50 000-point clouds (one dense pair), each with 30 forced iterations (tol_* = 0: every iteration runs its correspondence pass) plus the
final pass.  Clouds are drawn on the GPU: a box scene seen twice, the second view moved by 2 degrees and 0.3 m with 2 cm jitter.
Per shape one JSON line: ms per pr_icp_pairs_dev call (HIP events on the context's stream, median (min .. max) of --iters after two
warm-ups), one correspondence pass alone (pr_icp_nn_dev), point pairs per second of the call (31 passes) and the fraction of the non-FMA
fp64 vector rate: 9 fp64 lane-operations per pair (3 subtractions, 3 products, 2 sums, 1 compare; the three 32-bit selects issue on the
same port but are not counted) against 1024 SIMDs x 16 lanes x 2.4 GHz = 39.3 T/s, the figure DESIGN.md 4.10 uses.
--search brute|grid|both chooses the correspondence search (pr_set_icp_search), both in one process so that the clocks are
comparable.  Every line carries `search`; a grid line times one pass through pr_icp_nn_radius_dev (grid build + one probe), gives the
build's share of the call from a call with max_iter = 0 less one probe pass (`grid_build_ms`, `grid_build_frac`), checks that T and the
statistics equal the brute-force split path's bytes when both ran (`equals_brute_split`), and leaves out frac_of_fp64_vector_rate and the
pair rates: they count pairs the grid never forms.

    python tools/bench_icp.py [--iters 5] [--only 4096] [--search both] [--out profiles/icp/bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((64, 4096), (1, 50000))
PEAK = 1024 * 16 * 2.4e9
OPS_PER_PAIR = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", type=int, default=0, help="only the shape with this many points per cloud")
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--search", choices=("brute", "grid", "both"), default="brute")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from so_dso_place_recognition_amd import _lib, api
    from so_dso_place_recognition_amd.matcher import _stream_context
    ctx = _stream_context(0)
    lib = ctx.lib
    p = lambda t: C.c_void_p(t.data_ptr())
    lines = []
    for c, P in SHAPES:
        if a.only and P != a.only:
            continue
        g = torch.Generator(device="cuda"); g.manual_seed(c + P)
        base = (torch.rand((c, P, 3), generator=g, device="cuda", dtype=torch.float64) - 0.5) * torch.tensor([80.0, 6.0, 80.0], device="cuda")
        th = np.radians(2.0)
        R = torch.tensor([[np.cos(th), 0, -np.sin(th)], [0, 1, 0], [np.sin(th), 0, np.cos(th)]], device="cuda", dtype=torch.float64)
        xq = (base + 0.02 * torch.randn(base.shape, generator=g, device="cuda", dtype=torch.float64)).reshape(-1, 3).contiguous()
        xd = (base @ R.T + torch.tensor([0.3, 0.02, -0.2], device="cuda") + 0.02 * torch.randn(base.shape, generator=g, device="cuda", dtype=torch.float64))
        xd = xd.reshape(-1, 3).contiguous()
        offs = (torch.arange(c + 1, device="cuda", dtype=torch.int64) * P).contiguous()
        pair = torch.arange(c, device="cuda", dtype=torch.int32)
        T0 = torch.eye(3, 4, device="cuda", dtype=torch.float64).repeat(c, 1, 1).contiguous()
        T = torch.empty_like(T0); stats = torch.zeros((c, 32), dtype=torch.uint8, device="cuda")
        oo = torch.empty(c + 1, dtype=torch.int64, device="cuda"); nj = torch.empty(c * P, dtype=torch.int32, device="cuda")
        nd = torch.empty(c * P, dtype=torch.float64, device="cuda")
        def pairs_call(max_iter, T_out):
            return lambda: lib.pr_icp_pairs_dev(ctx.h, p(xq), p(offs), c, p(xd), p(offs), c, p(pair), p(pair), c, p(T0), P, P, max_iter, 1.0, 0.0, 0.0,
                                                3, p(T_out), p(stats))

        def timed(fn):
            ts = []
            for it in range(a.iters + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(fn())
                e1.record()
                e1.synchronize()
                if it >= 2:
                    ts.append(e0.elapsed_time(e1))
            return float(np.median(ts)), float(min(ts)), float(max(ts))

        split_bytes = None
        for search in (("brute", "grid") if a.search == "both" else (a.search,)):
            grid = search == "grid"
            ctx.check(lib.pr_set_icp_search(ctx.h, _lib.ICP_SEARCH_GRID if grid else _lib.ICP_SEARCH_BRUTE))
            calls = {"icp": pairs_call(a.max_iter, T)}
            if grid:
                calls["nn"] = lambda: lib.pr_icp_nn_radius_dev(ctx.h, p(xq), p(offs), c, p(xd), p(offs), c, p(pair), p(pair), c, p(T0), P, P, 1.0, p(oo),
                                                               p(nj), p(nd))
                calls["icp0"] = pairs_call(0, torch.empty_like(T0))              # init + build + one probe + one finish
            else:
                calls["nn"] = lambda: lib.pr_icp_nn_dev(ctx.h, p(xq), p(offs), c, p(xd), p(offs), c, p(pair), p(pair), c, p(T0), P, P, p(oo), p(nj), p(nd))
            ms = {name: timed(calls[name]) for name in ("nn", "icp0", "icp") if name in calls}      # "icp" last: T and stats are the full call's
            st = np.frombuffer(stats.cpu().numpy().tobytes(), api.ICP_STATS)
            passes = a.max_iter + 1
            line = dict(bench="icp", search=search, pairs=c, points=P, max_iter=a.max_iter, passes=passes, iters=a.iters, icp_ms=round(ms["icp"][0], 4),
                        icp_ms_min=round(ms["icp"][1], 4), icp_ms_max=round(ms["icp"][2], 4), nn_pass_ms=round(ms["nn"][0], 4))
            if grid:
                per_pass = (ms["icp"][0] - ms["icp0"][0]) / max(a.max_iter, 1)  # one probe + one finish
                build = max(ms["icp0"][0] - per_pass, 0.0)
                line.update(grid_build_ms=round(build, 4), grid_build_frac=round(build / ms["icp"][0], 4), grid_pass_ms=round(per_pass, 4))
                if split_bytes is not None:
                    line.update(equals_brute_split=bool(split_bytes == (T.cpu().numpy().tobytes(), stats.cpu().numpy().tobytes())))
            else:
                pairs = float(c) * P * P * passes
                rate = pairs / (ms["icp"][0] * 1e-3)
                line.update(point_pairs_per_s=round(rate, 1), nn_pass_point_pairs_per_s=round(float(c) * P * P / (ms["nn"][0] * 1e-3), 1),
                            frac_of_fp64_vector_rate=round(rate * OPS_PER_PAIR / PEAK, 4), ops_per_pair=OPS_PER_PAIR)
                if a.search == "both":                                           # the bytes the grid has to return: the split path's
                    ctx.check(lib.pr_set_icp_path(ctx.h, 2))
                    ctx.check(pairs_call(a.max_iter, T)())
                    ctx.check(lib.pr_set_icp_path(ctx.h, 0))
                    split_bytes = (T.cpu().numpy().tobytes(), stats.cpu().numpy().tobytes())
            line.update(status=sorted(set(st["status"].tolist())), iters_done=sorted(set(st["iters"].tolist())),
                        fitness_min=float(st["fitness"].min()), rmse_max=float(st["rmse"].max()))
            print(json.dumps(line), flush=True)
            lines.append(line)
        ctx.check(lib.pr_set_icp_search(ctx.h, _lib.ICP_SEARCH_BRUTE))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
