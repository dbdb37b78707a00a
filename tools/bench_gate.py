#!/usr/bin/env python3
"""The closure consistency gate (pr_gate).  Method as tools/bench_graph.py: wall time from the call to the end of a stream
synchronisation, median (min .. max) over --iters after --warmup warm-ups, eager and as a graph replay.  Recorded, not gated.
  gate        run_torch at rounds = 1 and 8 over three logs on a noisy two-lap circle (tests/posegraph_np.py): the drive (3475 nodes, one
              closure per 20 nodes = 173, 4.17's timing case), 4096 edges and 65536 edges (4096 nodes; i on the first lap, j within 3 rows
              of i + n / 2, in the order of j as a drive logs them, one closure in twenty measured from a row 5 places off); the drive's
              closures are 20 apart in |di| + |dj|, so --max-gap must exceed that for any of them to be kept; valid / kept / flags go
              into the record
  relax       at the drive only: the same run's relax_torch of the gated log, eager and as a replay
  gate_relax  at the drive only: ONE graph of gate -> relax, so the gate's share of the replay is on record

    python tools/bench_gate.py [--iters 10] [--warmup 2] [--max-gap 64] [--min-support 2] [--outer 5] [--inner 64]
                               [--out profiles/gate/bench.jsonl]"""
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
    ap.add_argument("--max-gap", type=int, default=64)
    ap.add_argument("--min-support", type=int, default=2)
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
    lines = []
    st = torch.cuda.Stream()
    NC = 4096

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

    def log_of(name, n, gt):
        """(edge_ij, edge_Z) of the named log"""
        half = n // 2
        if name == "drive":
            i = np.linspace(0, half - 1, max(n // 20, 1)).astype(np.int64)
            j, src = i + half, i
        else:
            E = int(name)
            rng = np.random.default_rng(E)
            i = rng.integers(0, half, E)
            j = np.clip(i + half + rng.integers(-3, 4, E), half, n - 1)
            order = np.lexsort((i, j))                              # a log is written in the order of its query keyframes
            i, j = i[order], j[order]
            src = np.where(rng.integers(0, 20, E) == 0, np.minimum(i + 5, half - 1), i)
        P = pg.as34(gt)
        Z = pg.mul(P[src], pg.inv(P[j])).reshape(-1, 12)
        return np.stack([i, j], axis=1).astype(np.int32), Z

    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        for name, n, EC in (("drive", 3475, NC // 20 + 8), ("4096", NC, 4096), ("65536", NC, 65536)):
            gt = pg.circle_truth(n, 2, radius=10.0 + n / 8.0)
            sc = min(1.0, 12.0 / n) ** 0.5
            poses = torch.zeros((NC, 12), dtype=torch.float64, device="cuda")
            poses[:n] = torch.from_numpy(pg.noisy(gt, 7, rot=0.01 * sc, trans=0.05 * sc)).cuda()
            nd = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")
            ij, Z = log_of(name, n, gt)
            E = len(ij)
            src = api.PoseGraph(ctx, NC, EC, max_outer=a.outer, max_inner=a.inner)
            dst = api.PoseGraph(ctx, NC, EC, max_outer=a.outer, max_inner=a.inner)
            src.edge_ij[:E] = torch.from_numpy(ij).cuda(); src.edge_Z[:E] = torch.from_numpy(Z).cuda()
            src.edge_w[:E] = torch.tensor([100.0, 10.0], dtype=torch.float64, device="cuda")
            src.state[0] = E
            outs = dict(keep=torch.zeros(EC, dtype=torch.uint8, device="cuda"), support=torch.zeros(EC, dtype=torch.int32, device="cuda"),
                        map=torch.zeros(EC, dtype=torch.int32, device="cuda"), info=torch.zeros(4, dtype=torch.int32, device="cuda"))
            out = torch.zeros((NC, 12), dtype=torch.float64, device="cuda")
            rep = torch.zeros(a.outer + 2, dtype=torch.float64, device="cuda")
            prm = dict(outer=a.outer, inner=a.inner, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0)
            for rounds in (1, 8):
                gate = api.ClosureGate(ctx, src, dst, a.max_gap, a.min_support, rounds)
                run = lambda: gate.run_torch(poses, nd, **outs)
                relax = lambda: dst.relax_torch(poses, nd, out=out, report=rep, **prm)
                both = lambda: (run(), relax())
                todo = [("gate", run)] + ([("relax", relax), ("gate_relax", both)] if name == "drive" else [])
                for bench, fn in todo:
                    fn()
                    st.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=st):
                        fn()
                    for form, f in (("eager", fn), ("graph", graph.replay)):
                        t = timed(f)
                        info = outs["info"].cpu().numpy()
                        lines.append(dict(bench=bench, form=form, log=name, nodes=n, edges=E, edge_capacity=EC, node_capacity=NC, rounds=rounds,
                                          max_gap=a.max_gap, min_support=a.min_support, valid=int(info[0]), kept=int(info[1]), flags=int(info[3]),
                                          outer=a.outer, inner=a.inner, iters=a.iters, **t, **box))
                        print(json.dumps(lines[-1]), flush=True)
                    del graph
                gate.close()
            dst.close(); src.close()
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
