#!/usr/bin/env python3
"""The registration information (pr_reginfo) beside the refine call it follows, c = 5 slots of about 60 and about 2000
source points.  The method of DESIGN.md 4.15: wall time from the call to the end of a stream synchronise, median (min .. max) of
--iters after --warmup warm-ups, eager and as a graph replay.
  reginfo_point  RegistrationInfo.point_torch behind a finished pr_icp_nn_radius_dev pass (info: two launches), the pass and the
                 information together (pairs_torch), and icp_refine_torch of the same pairs with --icp-iters forced iterations
  reginfo_plane  RegistrationInfo.plane_torch behind a finished pr_maploc_nn_dev pass, the pass and the information together
                 (maploc_torch), and PlaneLocalizer.refine_torch of the same pairs: 3 (max_iter + 1) launches against the information's two
The world of the plane form is a floor and two walls of 12 m fused at cell 0.5.  The comparison that matters is the ratio information /
refine of the same shape; no threshold is attached.

    python tools/bench_reginfo.py [--iters 10] [--warmup 2] [--icp-iters 10] [--out profiles/reginfo/bench.jsonl]"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, SIZES, CELL, MAX_CORR = 5, (60, 2000), 0.5, 0.499
PRM = dict(min_ratio=1e-4, sigma_min=0.01, w_max=1e6)


def planes(rng, n, extent):
    """n points on a floor and two walls (z, x, y = 0.05) of `extent` m"""
    pts = []
    for k, plane in enumerate((2, 0, 1)):
        m = n // 3 + (1 if k < n % 3 else 0)
        pts.append(np.insert(extent * rng.random((m, 2)), plane, 0.05, axis=1))
    return np.vstack(pts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--icp-iters", type=int, default=10)
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

    def ratios(ms):
        return {f"ratio_{k}_over_refine_{m}": ms[k][m]["median"] / ms["refine"][m]["median"] for k in ("info", "pass_and_info") for m in ("eager", "graph")}

    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    rng = np.random.default_rng(5)
    ang = np.deg2rad(1.0)
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    seed = np.hstack([Rz, [[0.05], [-0.04], [0.03]]])
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        # ---- the plane form's world: four keyframes with identity poses, each a cloud on the three planes
        K, M = 4, 30000
        km = api.KeyframeMap(ctx, K, K * M, M, max_append=K)
        eye = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12), (K, 1))
        st.synchronize()
        km.append_torch(dev(np.vstack([planes(rng, M, 12.0) for _ in range(K)]), np.float64), torch.zeros(K * M, dtype=torch.float32, device="cuda"),
                        torch.arange(K + 1, dtype=torch.int64, device="cuda") * M, torch.zeros((K, 16), dtype=torch.float64, device="cuda"),
                        poses=dev(eye, np.float64), ids=torch.arange(K, dtype=torch.int32, device="cuda"))
        probe = api.WorldMap(ctx, km, K * M)
        rows = int(probe.fuse_torch(cell=CELL, min_count=1, keep="first").cpu()[0])
        probe.close()
        wm = api.WorldMap(ctx, km, rows)
        wm.fuse_torch(cell=CELL, min_count=1, keep="first")
        for n in SIZES:
            # ---- the point form: c clouds and their targets (the cloud moved back by the seed, 5 mm of noise), pair p = (p, p)
            src = [planes(rng, n, 6.0) - (3.0, 3.0, 1.0) for _ in range(C)]
            dst = [(s - seed[:, 3]) @ seed[:, :3] + rng.normal(0.0, 0.005, s.shape) for s in src]          # so that seed^-1 registers src onto dst
            inv = np.hstack([seed[:, :3].T, (-seed[:, :3].T @ seed[:, 3])[:, None]])
            xq, xd = dev(np.vstack(src), np.float64), dev(np.vstack(dst), np.float64)
            oq = torch.arange(C + 1, dtype=torch.int64, device="cuda") * n
            ps = torch.arange(C, dtype=torch.int32, device="cuda")
            idx = ps.reshape(C, 1).contiguous()
            T0 = dev(np.tile(np.eye(3, 4), (C, 1, 1)), np.float64)
            T = dev(np.tile(inv, (C, 1, 1)), np.float64)
            acc = torch.ones((C, 1), dtype=torch.bool, device="cuda")
            kw = dict(max_iter=a.icp_iters, max_corr=MAX_CORR, tol_rmse=0.0, tol_fitness=0.0, min_inliers=3)
            ri = api.RegistrationInfo(ctx, C, n)
            ref = api.icp_refine_torch(xq, oq, xd, oq, ps, ps, T0, n, n, ctx=ctx, **kw)
            Tq = T.reshape(C, 1, 3, 4)
            # slot p of pairs_torch reads query cloud p: one query per slot
            res = ri.pairs_torch((xq, oq), (xd, oq), idx, Tq, acc, n, n, max_corr=MAX_CORR, min_inliers=10, **PRM)
            nn = ri._work[("pairs", C, 1)]["nn"]
            st.synchronize()
            stat = res.stat.cpu().numpy()
            ms = dict(info=both(lambda: ri.point_torch(xq, oq, ps, T, nn, None, MAX_CORR, 10, out=res, **PRM)),
                      pass_and_info=both(lambda: ri.pairs_torch((xq, oq), (xd, oq), idx, Tq, acc, n, n, max_corr=MAX_CORR, min_inliers=10, out=res, **PRM)),
                      refine=both(lambda: api.icp_refine_torch(xq, oq, xd, oq, ps, ps, T0, n, n, ctx=ctx, out=ref, **kw)))
            emit(dict(bench="reginfo_point", c=C, src_pts=n, icp_iters=a.icp_iters, max_corr=MAX_CORR, n_inl=stat[:, 0].tolist(), flags=stat[:, 3].tolist(),
                      w=res.w.cpu().numpy().tolist(), ms=ms, scratch_bytes=int(_lib.load().pr_reginfo_scratch_bytes(C, n)), **ratios(ms)))
            # ---- the plane form: c clouds on the world's planes in a sensor frame 1 degree and 8 cm off
            ml = api.MapLocalizer(ctx, wm, CELL, C, n)
            pl = api.PlaneLocalizer(ctx, ml)
            ml.index_torch()
            nout = pl.normals_torch(0.99 * CELL, min_nbrs=4, max_ratio=0.05)
            srcw = [planes(rng, n, 11.0) for _ in range(C)]
            xq = dev(np.vstack([(s - seed[:, 3]) @ seed[:, :3] for s in srcw]), np.float64)
            Ts = dev(np.tile(seed, (C, 1, 1)), np.float64)
            kwp = dict(max_iter=a.icp_iters, max_corr=MAX_CORR, tol_rmse=0.0, tol_fitness=0.0, min_inliers=6)
            refp = pl.refine_torch(xq, oq, ps, Ts, nout[0], nout[1], **kwp)
            resp = ri.maploc_torch(pl, xq, oq, ps, Ts, nout[0], nout[1], max_corr=MAX_CORR, min_inliers=10, **PRM)
            nnp = ri._work[("maploc", C)]
            st.synchronize()
            stat = resp.stat.cpu().numpy()
            ms = dict(info=both(lambda: ri.plane_torch(xq, oq, ps, Ts, nnp, wm.xyz, nout[0], nout[1], None, MAX_CORR, 10, out=resp, **PRM)),
                      pass_and_info=both(lambda: ri.maploc_torch(pl, xq, oq, ps, Ts, nout[0], nout[1], max_corr=MAX_CORR, min_inliers=10, out=resp, **PRM)),
                      refine=both(lambda: pl.refine_torch(xq, oq, ps, Ts, nout[0], nout[1], out=refp, **kwp)))
            emit(dict(bench="reginfo_plane", c=C, src_pts=n, icp_iters=a.icp_iters, refine_launches=3 * (a.icp_iters + 1), info_launches=2,
                      max_corr=MAX_CORR, world_rows=rows, n_inl=stat[:, 0].tolist(), n_plane=stat[:, 1].tolist(), flags=stat[:, 3].tolist(),
                      w=resp.w.cpu().numpy().tolist(), ms=ms, **ratios(ms)))
            pl.close(); ml.close(); ri.close()
        wm.close(); km.close(); ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
