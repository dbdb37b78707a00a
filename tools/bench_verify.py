#!/usr/bin/env python3
"""The verify stage of an SC matcher at m = 64 queries, k = 1, 4096-point clouds and 30 forced ICP iterations (tol_* = 0): the
host-seeded Matcher.verify (variants read back, pr_sc_relative_pose on the host, seeds uploaded) against the stream-ordered
Matcher.verify_dev (pr_verify_pairs_dev) with one and with two hypotheses.  A box scene seen twice, the second view turned by 137 degrees
and moved by 0.3 m with 2 cm jitter; the candidates are the true entries.  Both forms are timed the same way - wall clock from the call
to the end of a device synchronisation, since verify() itself waits for the device in the middle - after --warmup calls; one JSON line
per form with the median (min .. max) of --iters calls, the device's name and the box (host, compute units, the device's maximum
engine clock as the runtime reports it - the clocks are not pinned -, HBM size, torch / HIP versions).

    python tools/bench_verify.py [--iters 20] [--warmup 3] [--out profiles/verify/bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from so_dso_place_recognition_amd import api, synth
    from so_dso_place_recognition_amd.matcher import Matcher
    m, P = a.queries, a.points
    xyz, it, offs = synth.scene_clouds(7, m, P)
    rng = np.random.default_rng(8)
    th = np.radians(137.0)
    R = np.array([[np.cos(th), 0, -np.sin(th)], [0, 1, 0], [np.sin(th), 0, np.cos(th)]])
    xq = xyz + rng.normal(0, 0.02, xyz.shape)
    xd = xyz @ R.T + np.array([0.3, 0.02, -0.2]) + rng.normal(0, 0.02, xyz.shape)
    sig_q, sig_d = api.sc_generate(xq, it, offs), api.sc_generate(xd, it, offs)
    fq, fd = api.cloud_frames(xq, it, offs), api.cloud_frames(xd, it, offs)
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    mt = Matcher("sc", m, m)
    mt.pack_database(dev(sig_d, np.float64))
    mt.match(dev(sig_q, np.float64), 0, 2.0, 1)
    idx = torch.arange(m, dtype=torch.int32, device="cuda").reshape(m, 1).contiguous()
    cq, cd = (dev(xq, np.float64), dev(offs, np.int64)), (dev(xd, np.float64), dev(offs, np.int64))
    dfq, dfd = dev(fq, np.float64), dev(fd, np.float64)
    kw = dict(max_iter=a.max_iter, tol_rmse=0.0, tol_fitness=0.0)
    forms = {
        "verify (host seed)": lambda: mt.verify(idx, cq, cd, fq, fd, P, P, **kw),
        "verify_dev hypotheses=1": lambda: mt.verify_dev(idx, cq, cd, dfq, dfd, P, P, hypotheses=1, **kw),
        "verify_dev hypotheses=2": lambda: mt.verify_dev(idx, cq, cd, dfq, dfd, P, P, hypotheses=2, **kw),
    }
    import platform
    pr = torch.cuda.get_device_properties(0)
    box = dict(host=platform.node(), compute_units=pr.multi_processor_count, max_engine_clock_mhz=getattr(pr, "clock_rate", 0) // 1000,
               hbm_gib=round(pr.total_memory / 2 ** 30, 1), torch=torch.__version__, hip=torch.version.hip,
               note="clocks are the device's defaults (not pinned); the box is shared")
    lines = []
    for name, fn in forms.items():
        ts = []
        for i in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        st = np.frombuffer(res[1].cpu().numpy().tobytes(), api.ICP_STATS)
        line = dict(bench="verify", form=name, queries=m, k=1, points=P, max_iter=a.max_iter, iters=a.iters, warmup=a.warmup,
                    ms=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), accepted=int(res[2].sum()),
                    iters_done=sorted(set(st["iters"].tolist())), hyp1=int(res[3].sum()) if len(res) > 3 else None,
                    device=torch.cuda.get_device_name(0), box=box)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    mt.close()


if __name__ == "__main__":
    main()
