#!/usr/bin/env python3
"""Rows that moments_select_kernel answered through a second sweep (pr_select_fallback_rows), after one step of bench.py's shape
(SC, --queries x --db, k = 1, no mask) and after the self-match of extra.kitti_shape's size (3475 generated SC signatures, mask 100; rows
of that length go through the one-wave selection, so its count says that the fused kernel did not run).  One JSON line each.

    python tools/select_fallback_rows.py [--db 100000] [--queries 4096] [--no-kitti-shape]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fallback_rows(ctx) -> int:
    v = C.c_int64(0)
    ctx.check(ctx.lib.pr_select_fallback_rows(ctx.h, C.byref(v)))
    return int(v.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--no-kitti-shape", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from so_dso_place_recognition_amd import api, synth
    from so_dso_place_recognition_amd.api import Context
    from so_dso_place_recognition_amd.matcher import Matcher
    dev = torch.device("cuda", 0)
    cur = int(torch.cuda.current_stream(dev).cuda_stream)
    n, m = args.db, args.queries
    db = synth.sc_database_torch(45, n, first=0, device=dev)
    q_host, planted = synth.sc_queries(46, np.empty((0, 2400)), m, db_first=0, n_global=n, db_seed=45)
    q = torch.from_numpy(q_host).to(dev)
    mt = Matcher("sc", m, n, ctx=Context(0, stream=cur))
    mt.pack_database(db)
    fallback_rows(mt.ctx)
    idx, _ = mt.match(q, 0, 2.0, 1)
    fell = fallback_rows(mt.ctx)
    print(json.dumps({"shape": "bench", "queries": m, "db": n, "k": 1, "mask": 0, "second_sweep_rows": fell, "fraction": fell / m,
                      "top1_planted": float((idx.cpu().numpy()[:, 0] == planted).mean())}), flush=True)
    mt.close()
    del mt, db, q
    if args.no_kitti_shape:
        return
    N = 3475
    xyz, it, offs, lap = synth.drive_clouds_torch(N, 6000, 5, stops=((400, 60), (1500, 40), (2600, 80)), device=dev)
    ctx = Context(0, stream=cur)
    sig = torch.from_numpy(api.sc_generate(xyz, it, offs, ctx=ctx)).to(dev)
    mt = Matcher("sc", N, N, ctx=ctx)
    mt.pack_database(sig)
    fallback_rows(ctx)
    mt.match(sig, 100, 2.0, 1)
    fell = fallback_rows(ctx)
    print(json.dumps({"shape": "kitti_shape", "queries": N, "db": N, "k": 1, "mask": 100, "second_sweep_rows": fell, "fraction": fell / N}), flush=True)
    mt.close()


if __name__ == "__main__":
    main()
