#!/usr/bin/env python3
"""Drive sessions (pr_session).  Method as tools/bench_gate.py: wall time from the call to the end of a stream
synchronisation, median (min .. max) over --iters after --warmup warm-ups, eager and as a graph replay.  Recorded, not gated.
  align          align_torch over a noisy two-lap circle of 4096 rows cut into two sessions, the second in a frame of its own, with
                 E = 64, 1024 and 16384 closures between them (all candidates; one in twenty measured from a row 5 places off);
                 status / a* / support / |I| go into the record
  relax          the relaxation at the drive of 4.17's timing case (3475 nodes, one closure per 20 nodes) with ONE session, in a fresh
                 process a run and --repeats runs a variant: `parent` = pr_posegraph_relax_dev of the tree given by --parent-tree (a
                 built checkout of the parent commit, package and library; without it the variant is left out), `plain` = pr_posegraph_relax_dev of this tree,
                 `session` = pr_session_relax_dev of this tree.  The record holds every run's median, the spread of the parent's runs
                 (largest - smallest median) and whether `plain` and `session` lie within that spread of the parent's middle run.

    python tools/bench_session.py [--iters 10] [--warmup 2] [--repeats 5] [--outer 5] [--inner 64] [--parent-tree PATH]
                                  [--out profiles/session/bench.jsonl]"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 4096


def timed(st, fn, warmup, iters):
    ts = []
    for i in range(warmup + iters):
        st.synchronize()
        t0 = time.perf_counter()
        fn()
        st.synchronize()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return dict(ms_median=float(np.median(ts)) * 1e3, ms_min=float(min(ts)) * 1e3, ms_max=float(max(ts)) * 1e3)


def both_forms(torch, st, fn, a):
    fn()
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        fn()
    out = {form: timed(st, f, a.warmup, a.iters) for form, f in (("eager", fn), ("graph", graph.replay))}
    del graph
    return out


def drive(torch, pg, n):
    gt = pg.circle_truth(n, 2, radius=10.0 + n / 8.0)
    sc = min(1.0, 12.0 / n) ** 0.5
    poses = torch.zeros((NC, 12), dtype=torch.float64, device="cuda")
    poses[:n] = torch.from_numpy(pg.noisy(gt, 7, rot=0.01 * sc, trans=0.05 * sc)).cuda()
    return gt, poses, torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")


def worker(a):
    """one variant of the relax comparison in this process -> one JSON line {eager, graph}"""
    import torch
    import posegraph_np as pg
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import _stream_context
    n = 3475
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        gt, poses, nd = drive(torch, pg, n)
        half = n // 2
        i = np.linspace(0, half - 1, max(n // 20, 1)).astype(np.int64)
        j = i + half
        P = pg.as34(gt)
        Z = pg.mul(P[i], pg.inv(P[j])).reshape(-1, 12)
        E, EC = len(i), NC // 20 + 8
        g = api.PoseGraph(ctx, NC, EC, max_outer=a.outer, max_inner=a.inner)
        g.edge_ij[:E] = torch.from_numpy(np.stack([i, j], axis=1).astype(np.int32)).cuda(); g.edge_Z[:E] = torch.from_numpy(Z).cuda()
        g.edge_w[:E] = torch.tensor([100.0, 10.0], dtype=torch.float64, device="cuda")
        g.state[0] = E
        out = torch.zeros((NC, 12), dtype=torch.float64, device="cuda")
        rep = torch.zeros(a.outer + 2, dtype=torch.float64, device="cuda")
        prm = dict(outer=a.outer, inner=a.inner, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0)
        if a.worker == "session":
            from so_dso_place_recognition_amd import graph
            table = graph.SessionTable(ctx, NC, EC, 4)
            fn = lambda: table.relax_torch(g, poses, nd, out=out, report=rep, **prm)
        else:
            fn = lambda: g.relax_torch(poses, nd, out=out, report=rep, **prm)
        res = both_forms(torch, st, fn, a)
        res.update(nodes=n, edges=E, cost=rep.cpu().numpy().tolist())
        print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--outer", type=int, default=5)
    ap.add_argument("--inner", type=int, default=64)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--tree", default="")
    ap.add_argument("--worker", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree) if a.tree else ROOT             # (a worker's package and library: every project import is below this line)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    if a.worker:
        return worker(a)
    import torch
    import posegraph_np as pg
    import session_np as sn
    from so_dso_place_recognition_amd import api, graph
    from so_dso_place_recognition_amd.matcher import _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    lines = []
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        n, half = NC, NC // 2
        gt = pg.circle_truth(n, 2, radius=10.0 + n / 8.0)
        own = sn.drives(gt, [0, half], n, 7, dict(rot=1e-5, trans=1e-4))
        poses = torch.from_numpy(own).cuda()
        nd = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")
        P = pg.as34(gt)
        for E in (64, 1024, 16384):
            rng = np.random.default_rng(E)
            i = rng.integers(0, half, E)
            j = np.clip(i + half + rng.integers(-3, 4, E), half, n - 1)
            src = np.where(rng.integers(0, 20, E) == 0, np.minimum(i + 5, half - 1), i)
            Z = pg.mul(P[src], pg.inv(P[j])).reshape(-1, 12)
            log = api.PoseGraph(ctx, NC, E)
            log.edge_ij[:] = torch.from_numpy(np.stack([i, j], axis=1).astype(np.int32)).cuda(); log.edge_Z[:] = torch.from_numpy(Z).cuda()
            log.edge_w[:] = torch.tensor([100.0, 10.0], dtype=torch.float64, device="cuda")
            log.state[0] = E
            table = graph.SessionTable(ctx, NC, E, 4)
            table.begin(torch.tensor([half], dtype=torch.int32, device="cuda"))
            keep = table.align_torch(log, poses, nd)
            fn = lambda: table.align_torch(log, poses, nd, out=keep.poses, G=keep.G, hyp=keep.hyp, support=keep.support, inlier=keep.inlier, info=keep.info)
            for form, t in both_forms(torch, st, fn, a).items():
                info = keep.info.cpu().numpy()
                lines.append(dict(bench="align", form=form, nodes=n, edges=E, node_capacity=NC, edge_capacity=E, status=int(info[0]), a_star=int(info[1]),
                                  support=int(info[2]), candidates=int(info[3]), inliers=int(info[4]), scratch_bytes=table.scratch_bytes(),
                                  iters=a.iters, **t, **box))
                print(json.dumps(lines[-1]), flush=True)
            table.close(); log.close()
        ctx.close()
    # the relax comparison: a fresh process a run, so that the package and library of the parent commit can be loaded
    runs = {}
    for variant in (["parent"] if a.parent_tree else []) + ["plain", "session"]:
        env = dict(os.environ)
        env.pop("PR_AMD_LIB", None)
        tree = os.path.abspath(a.parent_tree) if variant == "parent" else ROOT
        runs[variant] = []
        for _ in range(a.repeats):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "session" if variant == "session" else "plain", "--iters", str(a.iters),
                   "--warmup", str(a.warmup), "--outer", str(a.outer), "--inner", str(a.inner), "--tree", tree]
            r = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"bench_session: the {variant} worker failed:\n{r.stdout}\n{r.stderr}")
            runs[variant].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    for form in ("eager", "graph"):
        med = {v: sorted(x[form]["ms_median"] for x in rs) for v, rs in runs.items()}
        rec = dict(bench="relax", form=form, nodes=runs["plain"][0]["nodes"], edges=runs["plain"][0]["edges"], node_capacity=NC, sessions=1,
                   outer=a.outer, inner=a.inner, iters=a.iters, repeats=a.repeats, ms_medians=med,
                   same_cost=all(x["cost"] == runs["plain"][0]["cost"] for rs in runs.values() for x in rs), **box)
        if "parent" in med:
            mid, spread = med["parent"][len(med["parent"]) // 2], med["parent"][-1] - med["parent"][0]
            rec.update(parent_ms=mid, parent_spread_ms=spread,
                       **{v + "_within_spread": abs(med[v][len(med[v]) // 2] - mid) <= spread for v in ("plain", "session")})
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
