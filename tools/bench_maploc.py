#!/usr/bin/env python3
"""The map localiser (pr_maploc) on the two-lap map of tools/bench_worldmap.py (--keyframes x --points camera-frame
clouds along two laps of a 100 m circle), fused at cell 1.0 (about 0.5 M rows) and 0.2 (about 8 M rows) into a world map whose
out_capacity is the row count.  The method of DESIGN.md 4.15: wall time from the call to the end of a stream synchronise, median
(min .. max) of --iters after --warmup warm-ups, eager and as a graph replay.
  maploc_index    MapLocalizer.index_torch at both worlds
  maploc_refine   c = 1, 8, 64 sources of 4096 points (world rows of neighbouring keyframes, moved by 0.3 m and 1 degree), 30 forced
                  iterations (both tolerances 0), max_corr 0.9, against the cell-1.0 world: refine_torch, index_torch + refine_torch, one
                  pass (nn_torch), beside icp_refine_torch(search="grid") on the same one-cloud target in the same process - after the two
                  results were compared for equal bytes - with the scratch bytes of both (the existing call's from icp.cpp's plan).
The condition on record at c = 64: the median of index + refine (graph) is no larger than the existing call's (graph).

    python tools/bench_maploc.py [--iters 10] [--warmup 2] [--keyframes 3475] [--points 2500] [--out profiles/maploc/bench.jsonl]"""
import argparse
import json
import math
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SRC_PTS, ITERS_ICP, MAX_CORR = 4096, 30, 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keyframes", type=int, default=3475)
    ap.add_argument("--points", type=int, default=2500)
    ap.add_argument("--pairs", default="1,8,64")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import icp_grid_np
    from so_dso_place_recognition_amd import _lib, api
    from so_dso_place_recognition_amd.matcher import _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    lines = []
    st = torch.cuda.Stream()

    def timed(fn):
        t = []
        for r in range(a.warmup + a.iters):
            st.synchronize()
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            if r >= a.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        return dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)))

    def both(fn):
        """eager and as one captured graph replayed"""
        fn()
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            fn()
        res = dict(eager=timed(fn), graph=timed(g.replay))
        del g
        return res

    def emit(line):
        lines.append(dict(line, iters=a.iters, warmup=a.warmup, **box))
        print(json.dumps(lines[-1]), flush=True)

    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        K, M = a.keyframes, a.points
        gen = torch.Generator(device="cuda").manual_seed(7)
        th = torch.arange(K, dtype=torch.float64, device="cuda") * (4.0 * math.pi / K)
        c, s = torch.cos(th), torch.sin(th)
        centre = torch.stack([100.0 * c, 100.0 * s, torch.zeros_like(c)], 1)
        R = torch.zeros((K, 3, 3), dtype=torch.float64, device="cuda")       # world to camera: a turn about z by -theta
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = c, s, -s, c, 1.0
        t = -torch.bmm(R, centre.unsqueeze(-1)).squeeze(-1)
        kf = torch.cat([R, t.unsqueeze(-1)], 2).reshape(K, 12).contiguous()
        p = torch.rand((K * M, 3), dtype=torch.float64, device="cuda", generator=gen)
        p = (p * torch.tensor([90.0, 90.0, 8.0], dtype=torch.float64, device="cuda") - torch.tensor([45.0, 45.0, 2.0], dtype=torch.float64, device="cuda")).contiguous()
        inten = torch.rand(K * M, dtype=torch.float32, device="cuda", generator=gen)
        offs_d = torch.arange(K + 1, dtype=torch.int64, device="cuda") * M
        km = api.KeyframeMap(ctx, K, K * M, M, max_append=K)
        st.synchronize()
        km.append_torch(p, inten, offs_d, torch.zeros((K, 16), dtype=torch.float64, device="cuda"), poses=kf,
                        ids=torch.arange(K, dtype=torch.int32, device="cuda"))
        st.synchronize()
        del p, inten
        info = torch.zeros(4, dtype=torch.int64, device="cuda")
        for cell in (1.0, 0.2):
            probe = api.WorldMap(ctx, km, K * M)                               # a first fuse tells the row count; the world is then rebuilt at that capacity
            rows = int(probe.fuse_torch(cell=cell, min_count=1, keep="first").cpu()[0])
            probe.close(); del probe
            wm = api.WorldMap(ctx, km, rows)
            wm.fuse_torch(cell=cell, min_count=1, keep="first")
            pairs = [int(x) for x in a.pairs.split(",")] if cell == 1.0 else []
            ml = api.MapLocalizer(ctx, wm, cell, max(pairs + [1]), SRC_PTS if pairs else 0)
            ml.index_torch(info=info)
            st.synchronize()
            h = info.cpu().numpy()
            assert h.tolist() == [rows, rows, 0, 0], h
            T = 1 << max(6, math.ceil(math.log2(2 * rows)))
            ms_index = both(lambda: ml.index_torch(info=info))
            emit(dict(bench="maploc_index", cell=cell, rows=rows, table_slots=T, table_bytes=16 * T, ms=ms_index,
                      scratch_bytes=int(_lib.load().pr_maploc_scratch_bytes(rows, max(pairs + [1]), SRC_PTS if pairs else 0))))
            if pairs:
                wx, wrow = wm.xyz.cpu().numpy(), wm.row.cpu().numpy()
                rng = np.random.default_rng(11)
                cmax = max(pairs)
                clouds, T0 = [], np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (cmax, 1, 1))
                for i in range(cmax):
                    k0, w = int(rng.integers(0, max(1, K // 2 - 200))), 8
                    while True:
                        sel = np.nonzero((wrow >= k0) & (wrow < k0 + w))[0]
                        if len(sel) >= SRC_PTS:
                            break
                        w *= 2
                    q = wx[rng.permutation(sel)[:SRC_PTS]]
                    ang = np.deg2rad(1.0)
                    Rz = np.array([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1.0]])
                    mid = q.mean(0)
                    clouds.append((q - mid) @ Rz.T + mid + np.array([0.2, -0.2, 0.1]))          # 1 degree about the cloud's middle, 0.3 m
                xq = torch.from_numpy(np.vstack(clouds)).cuda()
                oq = torch.arange(cmax + 1, dtype=torch.int64, device="cuda") * SRC_PTS
                od = torch.tensor([0, rows], dtype=torch.int64, device="cuda")
                kw = dict(max_iter=ITERS_ICP, max_corr=MAX_CORR, tol_rmse=0.0, tol_fitness=0.0, min_inliers=3)
                for cp in pairs:
                    ps = torch.arange(cp, dtype=torch.int32, device="cuda")
                    pd = torch.zeros(cp, dtype=torch.int32, device="cuda")
                    t0 = torch.from_numpy(T0[:cp].copy()).cuda()
                    mine = ml.refine_torch(xq, oq, ps, t0, **kw)
                    theirs = api.icp_refine_torch(xq, oq, wm.xyz, od, ps, pd, t0, SRC_PTS, rows, ctx=ctx, search="grid", **kw)
                    st.synchronize()
                    equal = bool(torch.equal(mine[0], theirs[0]) and torch.equal(mine[1], theirs[1]))
                    stats = np.frombuffer(mine[1].cpu().numpy().tobytes(), api.ICP_STATS)
                    nn_out = ml.nn_torch(xq, oq, ps, t0, max_corr=MAX_CORR)
                    ms = dict(refine=both(lambda: ml.refine_torch(xq, oq, ps, t0, out=mine, **kw)),
                              index_and_refine=both(lambda: (ml.index_torch(info=info), ml.refine_torch(xq, oq, ps, t0, out=mine, **kw))),
                              one_pass=both(lambda: ml.nn_torch(xq, oq, ps, t0, max_corr=MAX_CORR, out=nn_out)),
                              existing_grid=both(lambda: api.icp_refine_torch(xq, oq, wm.xyz, od, ps, pd, t0, SRC_PTS, rows, ctx=ctx, out=theirs,
                                                                              search="grid", **kw)))
                    cells_, G = icp_grid_np.plan(cp, rows)
                    nch = (SRC_PTS + 255) // 256
                    existing_scratch = cp * (cells_ * 4 + rows * 4 + 48) + cp * SRC_PTS * 12 + cp * nch * 160 + cp * 20
                    emit(dict(bench="maploc_refine", cell=cell, rows=rows, pairs=cp, src_pts=SRC_PTS, icp_iters=ITERS_ICP, max_corr=MAX_CORR,
                              bytes_equal=equal, iters_done=[int(stats["iters"].min()), int(stats["iters"].max())],
                              fitness=[float(stats["fitness"].min()), float(stats["fitness"].max())], ms=ms,
                              ratio_existing_over_index_and_refine=ms["existing_grid"]["graph"]["median"] / ms["index_and_refine"]["graph"]["median"],
                              condition_holds=bool(ms["index_and_refine"]["graph"]["median"] <= ms["existing_grid"]["graph"]["median"]) if cp == 64 else None,
                              scratch_bytes=int(_lib.load().pr_maploc_scratch_bytes(rows, max(pairs), SRC_PTS)), existing_grid_cells_per_pair=cells_,
                              existing_scratch_bytes=existing_scratch))
            ml.close(); wm.close()
        km.close(); ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
