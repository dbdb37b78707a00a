#!/usr/bin/env python3
"""The world map (pr_worldmap): WorldMap.fuse_torch beside what a caller composes from torch today, on two maps:
  seq07     the 140-pose KITTI seq07 drive of tools/bench_map.py (60 points per pose) through the GPU pre-stage: 110 keyframes, 240 k points
  two_lap   --keyframes x --points camera-frame clouds generated on the device along two laps of a 100 m circle (0.36 m between keyframes,
            points uniform in a 90 x 90 x 8 m box around the camera): neighbouring keyframes and the two laps overlap
each at --cells (default 0.2 and 1.0), min_count 1, keep first.  The method of DESIGN.md 4.15: wall time from the call to the end of a
stream synchronise, median of --iters after --warmup warm-ups, for
  hip_eager / hip_graph   fuse_torch, and one captured fuse_torch replayed
  torch                   the composition: read the point count back, searchsorted for the rows, gather the poses, batched matmul, floor,
                          pack the keys, torch.unique(return_inverse, return_counts), scatter_reduce(amin) for the first point of each
                          voxel, sort of the representatives, gathers of the five output rows
The torch rows are compared with the HIP rows before anything is timed (torch_rows_equal: same src, row and count; torch_max_abs_dxyz).  Each line
states ratio = torch / hip_graph (the condition on record: >= 1 on both maps) and the compulsory traffic of a fuse - 20 T bytes of table
cleared, 28 bytes read per point, 4 + 4 bytes of slot index written and read per point, 44 bytes written per row - per second of the
graph form beside the HBM rate the MI355X guide measures for a streaming copy (6.29 TB/s): a statement of distance from that bound, not
a claim - the table accesses are random 8-byte atomics, not streams.

    python tools/bench_worldmap.py [--iters 10] [--warmup 2] [--keyframes 3475] [--points 2500] [--cells 0.2,1.0] [--out profiles/worldmap/bench.jsonl]"""
import argparse
import json
import math
import os
import socket
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_COPY_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keyframes", type=int, default=3475)
    ap.add_argument("--points", type=int, default=2500)
    ap.add_argument("--cells", default="0.2,1.0")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import helpers
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    cells = [float(c) for c in a.cells.split(",")]
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
        return float(np.median(t))

    def torch_fuse(km, cell, min_count):
        """what a caller does today; returns (xyz, inten, src, row, count)"""
        n = int(km.state[0].item())                                      # the read-backs a caller cannot avoid
        P = int(km.offs[n].item())
        g = torch.arange(P, dtype=torch.int64, device="cuda")
        rows = torch.searchsorted(km.offs[:n + 1], g, right=True) - 1
        q = km.poses[rows].view(P, 3, 4)
        d = km.xyz[:P] - q[:, :, 3]
        w = torch.bmm(q[:, :, :3].transpose(1, 2), d.unsqueeze(-1)).squeeze(-1)
        c = torch.floor(w / cell).to(torch.int64) + (1 << 20)
        key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
        uniq, inv, counts = torch.unique(key, return_inverse=True, return_counts=True)
        first = torch.full((uniq.numel(),), P, dtype=torch.int64, device="cuda").scatter_reduce_(0, inv, g, "amin")
        ok = counts >= min_count
        src, order = torch.sort(first[ok])
        return w[src], km.inten[src], src, rows[src].to(torch.int32), counts[ok][order].to(torch.int32)

    def run(name, km, ctx):
        keyframes, points, flags = km.count()
        wm = api.WorldMap(ctx, km, points)
        info = torch.zeros(4, dtype=torch.int64, device="cuda")
        T = 1 << max(6, math.ceil(math.log2(2 * km.point_capacity)))
        for cell in cells:
            kw = dict(cell=cell, min_count=1, keep="first", info=info)
            wm.fuse_torch(**kw)
            st.synchronize()
            h = info.cpu().numpy()
            r = int(h[0])
            assert h[3] == 0 and h[2] == points, h
            ref = torch_fuse(km, cell, 1)
            st.synchronize()
            # (a point within the matmul's rounding of a cell boundary may fall on the other side: recorded, not asserted)
            same = ref[2].numel() == r and torch.equal(ref[2], wm.src[:r]) and torch.equal(ref[4], wm.count[:r]) and torch.equal(ref[3], wm.row[:r])
            dxyz = float((ref[0] - wm.xyz[:r]).abs().max()) if same and r else None
            del ref
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                wm.fuse_torch(**kw)
            ms = dict(hip_eager=timed(lambda: wm.fuse_torch(**kw)), hip_graph=timed(g.replay), torch=timed(lambda: torch_fuse(km, cell, 1)))
            del g
            traffic = 20 * T + 36 * points + 44 * r
            lines.append(dict(bench="worldmap_fuse", map=name, keyframes=keyframes, points=points, point_capacity=km.point_capacity, table_slots=T,
                              cell=cell, min_count=1, keep="first", rows=r, torch_rows_equal=bool(same), torch_max_abs_dxyz=dxyz, iters=a.iters, warmup=a.warmup, ms=ms,
                              ratio_torch_over_hip_graph=ms["torch"] / ms["hip_graph"], ratio_torch_over_hip_eager=ms["torch"] / ms["hip_eager"],
                              compulsory_bytes=traffic, tb_per_s_graph=traffic / (ms["hip_graph"] * 1e-3) / 1e12, hbm_copy_tb_per_s_guide=HBM_COPY_TBS,
                              **box))
            print(json.dumps(lines[-1]), flush=True)
        wm.close()

    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        # ---- seq07
        poses = os.path.join(ROOT, "tests", "golden", "kitti_seq07", "poses_history_file.txt")
        tmp = tempfile.mkdtemp()
        pts = os.path.join(tmp, "seq07_60.txt")
        helpers.write_synthetic_points(poses, pts, per_pose=60, max_poses=140)
        short = os.path.join(tmp, "seq07_60_poses.txt")
        open(short, "w").write("\n".join([l for l in open(poses).read().split("\n") if l.strip()][:140]) + "\n")
        pid, w, qid, _, _ = api.read_poses_points(short, pts)
        xyz, it, offs, ids = api.pts_preprocess(short, pts, None, 45.0, gpu=True, ctx=ctx)
        N = len(ids)
        kept = {int(i): k for k, i in enumerate(pid)}
        kf_poses = np.stack([w[kept[int(i)]].reshape(12) for i in ids])
        km = api.KeyframeMap(ctx, N, len(xyz), int(np.diff(offs).max()), max_append=N)
        km.append(xyz, it, offs, np.zeros((N, 16)), poses=kf_poses, ids=ids)
        run("seq07", km, ctx)
        km.close()
        # ---- two laps of a circle, generated on the device
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
        run("two_lap", km, ctx)
        km.close(); ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
