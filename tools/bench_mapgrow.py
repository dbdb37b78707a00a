#!/usr/bin/env python3
"""The incremental world map (pr_mapgrow) beside the rebuild it replaces, on the two-lap map of tools/bench_worldmap.py
(--keyframes x --points camera-frame clouds along two laps of a 100 m circle) at cells 1.0 and 0.2; out_capacity is the row count at K.
The method of tools/bench_mapplane.py: wall time from the call to the end of a stream synchronise, median (min .. max) of --iters after
--warmup warm-ups, eager and as a graph replay.  For n = K and K / 8 keyframes and each repetition:
  untimed  MapGrower.rebuild_torch at n - 64 (fuse -> index -> normals -> sync)
  timed    64 consecutive keyframes, each `row += 1; extend_torch(row); normals_torch` (ONE captured graph replayed 64 times in the graph
           mode; the row counter is a device word), divided by 64
  timed    the rebuild at n - fuse_torch + index_torch + PlaneLocalizer.normals_torch, the existing calls - in the same process, alternating
bytes_equal: the five world arrays (rows written), state and both normal arrays after the 64 extends against that rebuild at n.
The last line states the three conditions of the measurement: bytes_equal everywhere, per-keyframe time below the rebuild's at both cells,
and the per-keyframe time at K not above the time at K / 8 by more than the recorded min .. max spread of the two.

    python tools/bench_mapgrow.py [--iters 10] [--warmup 2] [--keyframes 3475] [--points 2500] [--out profiles/mapgrow/bench.jsonl]"""
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

STEPS = 64
NORMALS = dict(min_nbrs=3, max_ratio=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keyframes", type=int, default=3475)
    ap.add_argument("--points", type=int, default=2500)
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
    stat = lambda t: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)))

    def emit(line):
        lines.append(dict(line, iters=a.iters, warmup=a.warmup, **box))
        print(json.dumps(lines[-1]), flush=True)

    def clock(fn):
        st.synchronize()
        t0 = time.perf_counter()
        fn()
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3

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
        I32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")
        ok_bytes, ok_faster, per_kf = True, True, {}
        for cell in [float(x) for x in a.cells.split(",")]:
            probe = api.WorldMap(ctx, km, K * M)                               # a first fuse tells the row count at K
            rows = int(probe.fuse_torch(cell=cell, min_count=1, keep="first").cpu()[0])
            probe.close(); del probe
            wm = api.WorldMap(ctx, km, rows)
            ml = api.MapLocalizer(ctx, wm, cell, 1, 0)
            pl = api.PlaneLocalizer(ctx, ml)
            mg = api.MapGrower(ctx, wm, ml)
            radius = 0.99 * cell
            nout = pl.normals_torch(radius, **NORMALS)
            finfo, iinfo, einfo = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(3))
            row = torch.zeros(1, dtype=torch.int32, device="cuda")
            for n in (K, max(K // 8, STEPS + 1)):
                n_t, start_t = I32(n), I32(n - STEPS)

                def rebuild():
                    wm.fuse_torch(n=n_t, cell=cell, min_count=1, keep="first", info=finfo)
                    ml.index_torch(info=iinfo)
                    pl.normals_torch(radius, out=nout, **NORMALS)

                def step():
                    row.add_(1)
                    mg.extend_torch(row, info=einfo)
                    mg.normals_torch(radius, NORMALS["min_nbrs"], NORMALS["max_ratio"], nout[0], nout[1])

                def prepare():
                    mg.rebuild_torch(pl, n=start_t, radius=radius, out=nout, infos=(finfo, iinfo), **NORMALS)
                    row.fill_(n - STEPS - 1)

                # the graphs: captured behind an untimed rebuild; the captured step is one keyframe
                prepare(); step(); rebuild()
                st.synchronize()
                g_step, g_rebuild = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                prepare()
                with torch.cuda.graph(g_step, stream=st):
                    step()
                with torch.cuda.graph(g_rebuild, stream=st):
                    rebuild()
                ms, equal, added = {}, None, None
                for mode, one, full in (("eager", step, rebuild), ("graph", g_step.replay, g_rebuild.replay)):
                    t_step, t_full = [], []
                    for r in range(a.warmup + a.iters):
                        prepare()
                        st.synchronize()
                        before = int(wm.state.cpu()[0])
                        dt = clock(lambda: [one() for _ in range(STEPS)]) / STEPS
                        if r == 0:                                             # the bytes after the 64 extends, kept for the rebuild below
                            st.synchronize()
                            assert int(einfo.cpu()[3]) == 0 and mg.count()[0] == n, (einfo.cpu(), mg.count())
                            grown = [getattr(wm, name).clone() for name in api.WorldMap.NAMES] + [nout[0].clone(), nout[1].clone()]
                            added = int(wm.state.cpu()[0]) - before
                        df = clock(full)
                        if r == 0:
                            Rn = int(wm.state.cpu()[0])
                            now = [getattr(wm, name) for name in api.WorldMap.NAMES] + [nout[0], nout[1]]
                            cut = lambda x, i: x if i >= 5 else x[:Rn]          # the five world arrays: the rows written
                            same = all(torch.equal(cut(x, i).contiguous().view(torch.uint8), cut(y, i).contiguous().view(torch.uint8))
                                       for i, (x, y) in enumerate(zip(grown, now)))
                            equal = same if equal is None else (equal and same)
                            del grown
                        if r >= a.warmup:
                            t_step.append(dt); t_full.append(df)
                    ms[mode] = dict(per_keyframe=stat(t_step), rebuild=stat(t_full),
                                    ratio_rebuild_over_keyframe=float(np.median(t_full) / np.median(t_step)))
                del g_step, g_rebuild
                st.synchronize()
                emit(dict(bench="mapgrow", cell=cell, keyframes=n, steps=STEPS, points_per_keyframe=M, out_capacity=rows, rows_at_n=Rn,
                          rows_added_by_the_steps=added, radius=radius, ms=ms, bytes_equal=bool(equal), **NORMALS,
                          scratch_bytes=int(_lib.load().pr_mapgrow_scratch_bytes(M))))
                ok_bytes = ok_bytes and bool(equal)
                ok_faster = ok_faster and all(ms[m]["per_keyframe"]["median"] < ms[m]["rebuild"]["median"] for m in ms)
                per_kf[(cell, n)] = ms
            mg.close(); pl.close(); ml.close(); wm.close()
        flat = True
        detail = []
        for cell in sorted({k[0] for k in per_kf}):
            big, small = per_kf[(cell, K)], per_kf[(cell, max(K // 8, STEPS + 1))]
            for m in ("eager", "graph"):
                b, s_ = big[m]["per_keyframe"], small[m]["per_keyframe"]
                spread = (b["max"] - b["min"]) + (s_["max"] - s_["min"])
                detail.append(dict(cell=cell, mode=m, at_K=b["median"], at_K_over_8=s_["median"], spread=spread))
                flat = flat and (b["median"] - s_["median"] <= spread)
        emit(dict(bench="mapgrow_conditions", bytes_equal=ok_bytes, per_keyframe_below_rebuild=ok_faster, cost_follows_the_cloud=flat, detail=detail))
        km.close(); ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
