#!/usr/bin/env python3
"""The loop-closure log and the pose-graph relaxation (pr_posegraph).  Method as tools/bench_map.py: wall time from the
call to the end of a stream synchronisation, medians over --iters after --warmup warm-ups.  Recorded, not gated.
  posegraph_add    one add_torch of k = 2 slots per keyframe (both logged), microseconds, eager and as a graph replay
  posegraph_relax  relax_torch at --nodes node counts (default 140, 3475 and the capacity) with one closure per 20 nodes on a noisy
                   two-lap circle (tests/posegraph_np.py), milliseconds, eager and as a graph replay, at --outer / --inner; the first
                   and the last reported cost go into the record

    python tools/bench_graph.py [--iters 10] [--warmup 2] [--capacity 4096] [--nodes 140,3475] [--outer 5] [--inner 64]
                                [--out profiles/posegraph/bench.jsonl]"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--nodes", default="140,3475")
    ap.add_argument("--outer", type=int, default=5)
    ap.add_argument("--inner", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import posegraph_np as pg
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    counts = sorted({min(int(c), a.capacity) for c in a.nodes.split(",") if c} | {a.capacity})
    lines = []
    st = torch.cuda.Stream()

    def timed(fn):
        ts = []
        for i in range(a.warmup + a.iters):
            st.synchronize()
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            if i >= a.warmup:
                ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        ecap = a.capacity // 20 + 8
        g = api.PoseGraph(ctx, a.capacity, max(ecap, 2 * (a.warmup + a.iters) * 2 + 8), max_outer=a.outer, max_inner=a.inner)
        # ---- add: two accepted slots per keyframe
        idx = torch.tensor([[3, 5]], dtype=torch.int32, device="cuda")
        T = torch.from_numpy(np.tile(np.eye(4)[:3].reshape(1, 1, 3, 4), (1, 2, 1, 1))).cuda()
        acc = torch.ones((1, 2), dtype=torch.uint8, device="cuda")
        row = torch.tensor([9], dtype=torch.int32, device="cuda")
        info = torch.zeros(4, dtype=torch.int32, device="cuda")
        add = lambda: g.add_torch(idx, T, acc, row, 100.0, 10.0, info=info)
        add()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            add()
        for form, fn in (("eager", add), ("graph", graph.replay)):
            g.reset()
            med, lo, hi = timed(fn)
            lines.append(dict(bench="posegraph_add", form=form, k=2, us_median=med * 1e6, us_min=lo * 1e6, us_max=hi * 1e6, iters=a.iters, **box))
        del graph
        # ---- relax
        poses = torch.zeros((a.capacity, 12), dtype=torch.float64, device="cuda")
        nd = torch.zeros(4, dtype=torch.int32, device="cuda")
        out = torch.zeros((a.capacity, 12), dtype=torch.float64, device="cuda")
        rep = torch.zeros(a.outer + 2, dtype=torch.float64, device="cuda")
        prm = dict(outer=a.outer, inner=a.inner, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0)
        relax = lambda: g.relax_torch(poses, nd, out=out, report=rep, **prm)
        relax()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            relax()
        for n in counts:
            gt = pg.circle_truth(n, 2, radius=10.0 + n / 8.0)
            sc = min(1.0, 12.0 / n) ** 0.5
            poses.zero_()
            poses[:n] = torch.from_numpy(pg.noisy(gt, 7, rot=0.01 * sc, trans=0.05 * sc)).cuda()
            nd[0] = n
            g.reset()
            half, closures = n // 2, max(n // 20, 1)
            for a0 in np.linspace(0, half - 1, closures).astype(int):
                g.add([int(a0)], pg.measure(gt, int(a0), int(a0) + half), [1], int(a0) + half, 100.0, 10.0)
            for form, fn in (("eager", relax), ("graph", graph.replay)):
                med, lo, hi = timed(fn)
                r = rep.cpu().numpy()
                lines.append(dict(bench="posegraph_relax", form=form, nodes=n, closures=int(g.count()[0]), node_capacity=a.capacity, outer=a.outer,
                                  inner=a.inner, ms_median=med * 1e3, ms_min=lo * 1e3, ms_max=hi * 1e3, cost_first=float(r[0]),
                                  cost_last=float(r[a.outer]), edges_used=int(r[a.outer + 1]), iters=a.iters, **box))
        del graph
        g.close(); ctx.close()
    for l in lines:
        print(json.dumps(l))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
