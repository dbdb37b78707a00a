#!/usr/bin/env python3
"""The plane-metric map localiser (pr_mapplane) on the two-lap map of tools/bench_worldmap.py (--keyframes x --points
camera-frame clouds along two laps of a 100 m circle), fused at cell 1.0 (about 0.5 M rows) and 0.2 (about 8 M rows) into a world map
whose out_capacity is the row count.  The method of DESIGN.md 4.15: wall time from the call to the end of a stream synchronise, median
(min .. max) of --iters after --warmup warm-ups, eager and as a graph replay.
  mapplane_normals  PlaneLocalizer.normals_torch at both worlds (radius 0.99 cell, min_nbrs 3, max_ratio 1.0: the map's clouds are
                    uniform in a box, so the planarity test is left open and every row with three neighbours gets a normal)
  mapplane_refine   c = 1, 8, 64 sources of 4096 points (world rows of neighbouring keyframes, moved by 0.3 m and 1 degree), 30 forced
                    iterations (both tolerances 0), max_corr 0.9, against the cell-1.0 world: PlaneLocalizer.refine_torch beside
                    MapLocalizer.refine_torch in the same process, with the ratio plane / point.  No threshold is attached.

    python tools/bench_mapplane.py [--iters 10] [--warmup 2] [--keyframes 3475] [--points 2500] [--out profiles/mapplane/bench.jsonl]"""
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

SRC_PTS, ITERS_ICP, MAX_CORR = 4096, 30, 0.9
NORMALS = dict(min_nbrs=3, max_ratio=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keyframes", type=int, default=3475)
    ap.add_argument("--points", type=int, default=2500)
    ap.add_argument("--pairs", default="1,8,64")
    ap.add_argument("--cells", default="1.0,0.2")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
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
        for cell in [float(x) for x in a.cells.split(",")]:
            probe = api.WorldMap(ctx, km, K * M)                               # a first fuse tells the row count; the world is then rebuilt at that capacity
            rows = int(probe.fuse_torch(cell=cell, min_count=1, keep="first").cpu()[0])
            probe.close(); del probe
            wm = api.WorldMap(ctx, km, rows)
            wm.fuse_torch(cell=cell, min_count=1, keep="first")
            pairs = [int(x) for x in a.pairs.split(",")] if cell == 1.0 else []
            ml = api.MapLocalizer(ctx, wm, cell, max(pairs + [1]), SRC_PTS if pairs else 0)
            pl = api.PlaneLocalizer(ctx, ml)
            ml.index_torch(info=info)
            st.synchronize()
            assert info.cpu().numpy().tolist() == [rows, rows, 0, 0]
            nout = pl.normals_torch(0.99 * cell, **NORMALS)
            st.synchronize()
            ni = nout[1].cpu().numpy()
            ms_normals = both(lambda: pl.normals_torch(0.99 * cell, out=nout, **NORMALS))
            emit(dict(bench="mapplane_normals", cell=cell, rows=rows, radius=0.99 * cell, valid_rows=int((ni > 0).sum()),
                      mean_neighbours=float(np.abs(ni).mean()), ms=ms_normals, bytes_written=28 * rows, **NORMALS,
                      scratch_bytes=int(_lib.load().pr_mapplane_scratch_bytes(max(pairs + [1]), SRC_PTS if pairs else 0))))
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
                kw = dict(max_iter=ITERS_ICP, max_corr=MAX_CORR, tol_rmse=0.0, tol_fitness=0.0)
                for cp in pairs:
                    ps = torch.arange(cp, dtype=torch.int32, device="cuda")
                    t0 = torch.from_numpy(T0[:cp].copy()).cuda()
                    plane = pl.refine_torch(xq, oq, ps, t0, nout[0], nout[1], min_inliers=6, **kw)
                    point = ml.refine_torch(xq, oq, ps, t0, min_inliers=3, **kw)
                    st.synchronize()
                    sp = np.frombuffer(plane[1].cpu().numpy().tobytes(), api.ICP_STATS)
                    sq = np.frombuffer(point[1].cpu().numpy().tobytes(), api.ICP_STATS)
                    ms = dict(plane=both(lambda: pl.refine_torch(xq, oq, ps, t0, nout[0], nout[1], min_inliers=6, out=plane, **kw)),
                              point=both(lambda: ml.refine_torch(xq, oq, ps, t0, min_inliers=3, out=point, **kw)))
                    emit(dict(bench="mapplane_refine", cell=cell, rows=rows, pairs=cp, src_pts=SRC_PTS, icp_iters=ITERS_ICP, max_corr=MAX_CORR,
                              plane_iters_done=[int(sp["iters"].min()), int(sp["iters"].max())], plane_status=sorted(set(sp["status"].tolist())),
                              point_iters_done=[int(sq["iters"].min()), int(sq["iters"].max())], point_status=sorted(set(sq["status"].tolist())),
                              fitness=[float(sp["fitness"].min()), float(sp["fitness"].max())], ms=ms,
                              ratio_plane_over_point_graph=ms["plane"]["graph"]["median"] / ms["point"]["graph"]["median"],
                              ratio_plane_over_point_eager=ms["plane"]["eager"]["median"] / ms["point"]["eager"]["median"]))
            pl.close(); ml.close(); wm.close()
        km.close(); ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
