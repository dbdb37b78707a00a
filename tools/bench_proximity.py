#!/usr/bin/env python3
"""The pose-proximity candidate search and the batch add of the closure log (pr_proximity, pr_posegraphb_add).  Method as
tools/bench_graph.py (4.15): wall time from the call to the end of a stream synchronisation, median (min .. max) over --iters after
--warmup warm-ups, eager and as a graph replay.  Recorded, not gated.
  search_dev   n = 140, 910, 3475 and 4096 keyframes of a noisy two-lap circle (tests/proximity_np.py) at node_capacity 4096, k = 4,
               stride = 10, radius 5 growing by 0.02 to 30, min_gap 50; query_capacity 4096 (a whole-map pass) and 1 (the newest keyframe)
  torch_fp64   context, not a gate: the unbucketed rule as a plain torch fp64 expression (cdist, mask, topk) on the same poses
  add_batch    pr_posegraphb_add_dev at c = 64 and 8192 slots into an empty log of 16384 edges

    python tools/bench_proximity.py [--iters 10] [--warmup 2] [--out profiles/proximity/bench.jsonl]"""
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
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import proximity_np as px
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    lines = []
    st = torch.cuda.Stream()
    NC, K = 4096, 4
    kw = dict(radius=5.0, growth=0.02, radius_max=30.0, min_gap=50, stride=10, k=K)

    def timed(fn):
        ts = []
        for i in range(a.warmup + a.iters):
            st.synchronize()
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            if i >= a.warmup:
                ts.append(time.perf_counter() - t0)
        return dict(ms_median=float(np.median(ts)) * 1e3, ms_min=float(min(ts)) * 1e3, ms_max=float(max(ts)) * 1e3)

    def record(**line):
        lines.append(dict(iters=a.iters, **line, **box))
        print(json.dumps(lines[-1]), flush=True)

    def torch_rule(poses, n, q0, mq):
        """the unbucketed rule (stride 1) in plain torch fp64: centres, cumsum path length, cdist, mask, topk"""
        P = poses[:n].view(n, 3, 4)
        cen = -torch.einsum("nji,nj->ni", P[:, :, :3], P[:, :, 3])
        s = torch.cat([cen.new_zeros(1), torch.cumsum((cen[1:] - cen[:-1]).norm(dim=1), 0)])
        q = torch.arange(q0, q0 + mq, device=poses.device)
        d = torch.cdist(cen[q], cen)
        rad = torch.clamp(kw["radius"] + kw["growth"] * (s[q, None] - s[None, :]), max=kw["radius_max"])
        ok = (d < rad) & (torch.arange(n, device=poses.device)[None, :] + kw["min_gap"] <= q[:, None])
        return torch.topk(torch.where(ok, d, torch.full_like(d, float("inf"))), min(K, n), dim=1, largest=False)

    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        for Q in (NC, 1):
            ps = api.ProximitySearch(ctx, NC, Q, K)
            for n in (140, 910, 3475, 4096):
                P_np = np.zeros((NC, 12))
                P_np[:n] = px.two_lap_circle(n, seed=3, radius=5.0 + n / 12.0, rot=0.0005, trans=0.01, flat=True)   # the second lap meets the first
                poses = torch.from_numpy(P_np).cuda()
                nd = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")
                q0, mq = (0, n) if Q > 1 else (n - 1, 1)
                qr = torch.tensor([q0, mq], dtype=torch.int32, device="cuda")
                out = ps.search_torch(poses, nd, qr, **kw)
                fn = lambda: ps.search_torch(poses, nd, qr, out=out, **kw)
                fn()
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st):
                    fn()
                for form, f in (("eager", fn), ("graph", graph.replay)):
                    t = timed(f)
                    info = out.info.cpu().numpy()
                    record(bench="search_dev", form=form, nodes=n, node_capacity=NC, query_capacity=Q, k=K, stride=kw["stride"], rows_searched=int(info[0]),
                           slots_filled=int(info[1]), scratch_bytes=ps.scratch_bytes(), **t)
                del graph
                t = timed(lambda: torch_rule(poses, n, q0, mq))
                record(bench="torch_fp64", form="eager", nodes=n, node_capacity=NC, query_capacity=Q, k=K, stride=1, **t)
            ps.close()
        EC = 16384
        g = api.PoseGraph(ctx, NC, EC)
        for c in (64, 8192):
            rng = np.random.default_rng(c)
            i = torch.from_numpy(rng.integers(0, 2000, c).astype(np.int32)).cuda()
            j = torch.from_numpy(rng.integers(2048, 4096, c).astype(np.int32)).cuda()
            T = torch.from_numpy(rng.normal(size=(c, 12))).cuda()
            acc = torch.from_numpy((rng.random(c) < 0.8).astype(np.uint8)).cuda()
            info = torch.zeros(4, dtype=torch.int32, device="cuda")

            def fn():
                g.reset()
                g.add_batch_torch(i, j, T, acc, None, 100.0, 10.0, info=info)
            fn()
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                fn()
            for form, f in (("eager", fn), ("graph", graph.replay)):
                t = timed(f)
                record(bench="add_batch", form=form, c=c, edge_capacity=EC, logged=int(info.cpu().numpy()[0]), **t)
            del graph
        g.close()
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
