#!/usr/bin/env python3
"""The trajectory evaluation (pr_trajeval).  Method as tools/bench_graph.py (4.15): wall time from the call to the end of a
stream synchronisation, median (min .. max) over --iters after --warmup warm-ups, eager and as a graph replay.  Recorded, not gated.
  full     run_torch with everything on: SIM3 alignment, deltas (1, 10), lengths 100 .. 800 m, step 1, a closure log of n / 20 edges -
           n = 140 and 3475 keyframes of a noisy two-lap circle (tests/posegraph_np.py) at capacity 4096, B = 1 and 16 candidates
  ate      the same without deltas, lengths and log: the two launches every run has (prepare, alignment + ATE + prefixes)
The theta of every closure edge is also compared with the restatement's (tests/trajeval_np.py): `theta_ulps` is the largest difference in
units of the last place, on record for DESIGN.md's note on atan2.

    python tools/bench_trajeval.py [--iters 10] [--warmup 2] [--out profiles/trajeval/bench.jsonl]"""
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
    import posegraph_np as pg
    import trajeval_np as tn
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    lines = []
    st = torch.cuda.Stream()
    NC = 4096
    lengths = tuple(100.0 * k for k in range(1, 9))

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

    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        for n in (140, 3475):
            gt_np = np.zeros((NC, 12))
            gt_np[:n] = pg.circle_truth(n, 2, radius=10.0 + n / 8.0)
            gt_np[n:] = gt_np[0]
            EC = NC // 20 + 8
            E = max(n // 20, 1)
            half = n // 2
            i = np.linspace(0, half - 1, E).astype(np.int64)
            P = pg.as34(gt_np[:n])
            g = api.PoseGraph(ctx, NC, EC)
            eij, eZ = np.zeros((EC, 2), np.int32), np.zeros((EC, 12))
            eij[:E], eZ[:E] = np.stack([i, i + half], axis=1), pg.mul(P[i], pg.inv(P[i + half])).reshape(-1, 12)
            g.edge_ij.copy_(torch.from_numpy(eij).cuda()); g.edge_Z.copy_(torch.from_numpy(eZ).cuda())
            g.state[0] = E
            gt = torch.from_numpy(gt_np).cuda()
            nd = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")
            for B in (1, 16):
                est_np = np.stack([np.vstack([pg.noisy(gt_np[:n], 7 + b, rot=0.01, trans=0.05), gt_np[n:]]) for b in range(B)])
                est = torch.from_numpy(est_np).cuda()
                for bench, kw, log in (("full", dict(deltas=(1, 10), lengths=lengths, step=1, edge_capacity=EC), g), ("ate", dict(deltas=(), lengths=()), None)):
                    te = api.TrajectoryEval(ctx, NC, B=B, align="sim3", gt_kind="w2c", **kw)
                    out = {nm: torch.zeros(s, dtype=torch.int32 if dt == np.int32 else torch.float64, device="cuda")
                           for nm, (s, dt) in te.shapes(log is not None).items() if nm in ("ate", "rpe", "seg", "clo", "edge_err")}
                    fn = lambda: te.run_torch(est, nd, gt, log=log, out=out, optional=())
                    fn()
                    st.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=st):
                        fn()
                    ulps = None
                    if log is not None:
                        want = tn.evaluate(est_np[:1], n, gt_np, align="sim3", gt_kind="w2c", log=(eij, eZ, [E]), edge_capacity=EC)["edge_err"][:E, 0]
                        got = out["edge_err"].cpu().numpy()[:E, 0]
                        ulps = float(np.max(np.abs(got - want) / np.spacing(np.maximum(want, 1e-300))))
                    for form, f in (("eager", fn), ("graph", graph.replay)):
                        t = timed(f)
                        ate = out["ate"].cpu().numpy()
                        lines.append(dict(bench=bench, form=form, nodes=n, node_capacity=NC, B=B, edges=E if log is not None else 0,
                                          scratch_bytes=te.scratch_bytes(), ate_rmse=float(ate[0, 2]), s=float(ate[0, 6]), theta_ulps=ulps,
                                          iters=a.iters, **t, **box))
                        print(json.dumps(lines[-1]), flush=True)
                    del graph
                    te.close()
            g.close()
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
