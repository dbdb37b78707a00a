#!/usr/bin/env python3
"""One push of the resident point window (pr_window_push_dev) per keyframe, on two drives: the 140-pose KITTI seq07
drive of the tests (60 points per pose) and a heavier one (2000 points per pose).  Per drive and per form - eager push_torch, and the
same push captured once in a graph and replayed - the wall time of every EMITTING push from the call to the end of a stream
synchronisation; the drive is replayed --iters times after --warmup warm-ups, per push the median over the replays is taken, and the line
records the median and the max of those over the emitting pushes.  Beside them: the alive count, K = n_out, and which order path ran (LDS
or global scratch) at the last push, and - the comparison figure - pr_clouds_avg_ms of pr_pts_preprocess_gpu on the same files in the same
run: the batch form's amortised time per pose.  A push is expected to cost more per pose than that; the line puts the ratio on record.

    python tools/bench_window.py [--iters 20] [--warmup 3] [--out profiles/window/bench.jsonl]"""
import argparse
import json
import os
import socket
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import helpers
    from so_dso_place_recognition_amd import _lib, api
    from so_dso_place_recognition_amd.matcher import _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    poses = os.path.join(ROOT, "tests", "golden", "kitti_seq07", "poses_history_file.txt")
    tmp = tempfile.mkdtemp()
    lines = []
    for name, per_pose in (("seq07_60", 60), ("seq07_2000", 2000)):
        pts = os.path.join(tmp, name + ".txt")
        helpers.write_synthetic_points(poses, pts, per_pose=per_pose, max_poses=140)
        short = os.path.join(tmp, name + "_poses.txt")
        open(short, "w").write("\n".join([l for l in open(poses).read().split("\n") if l.strip()][:140]) + "\n")
        pid, w, qid, xyz, it = api.read_poses_points(short, pts)
        cuts = api.split_points_by_pose(pid, qid)
        api.pts_preprocess(short, pts, None, 45.0, False, gpu=True)               # warm-up of the batch form
        api.pts_preprocess(short, pts, None, 45.0, False, gpu=True)
        batch_ms = api.pts_preprocess.last_avg_ms
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            ctx = _stream_context(0)
            cap, mx = int(cuts[-1]), int(np.diff(cuts).max())
            pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((mx, 3), dtype=torch.float64, device="cuda")
            ii = torch.zeros(mx, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
            dw = torch.from_numpy(w).cuda(); dx = torch.from_numpy(xyz).cuda(); di = torch.from_numpy(it).cuda()
            dn = torch.from_numpy(np.diff(cuts).astype(np.int32)).cuda()

            def load(p):
                k = int(cuts[p + 1] - cuts[p])
                pose.copy_(dw[p]); x[:k].copy_(dx[cuts[p]:cuts[p + 1]]); ii[:k].copy_(di[cuts[p]:cuts[p + 1]]); n.copy_(dn[p:p + 1])

            for form in ("eager", "graph"):
                win = api.CloudWindow(ctx, 45.0, False, cap, mx, cap)
                out = win.empty_out()
                load(0)
                win.push_torch(pose, x, ii, n, out=out)
                st.synchronize()
                g = None
                if form == "graph":
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=st):
                        win.push_torch(pose, x, ii, n, out=out)
                times = np.zeros((a.iters, len(pid)))
                for r in range(a.warmup + a.iters):
                    win.reset()
                    for p in range(len(pid)):
                        load(p)
                        st.synchronize()
                        t0 = time.perf_counter()
                        if g is None:
                            win.push_torch(pose, x, ii, n, out=out)
                        else:
                            g.replay()
                        st.synchronize()
                        if r >= a.warmup:
                            times[r - a.warmup, p] = (time.perf_counter() - t0) * 1e3
                info = out["info"].cpu().numpy()
                per_push = np.median(times, axis=0)[30:]                          # (no reset in this drive: pushes 31 .. 140 emit)
                lines.append(dict(bench="window_push", drive=name, poses=len(pid), per_pose=per_pose, form=form, iters=a.iters, warmup=a.warmup,
                                  push_ms_median=float(np.median(per_push)), push_ms_max=float(per_push.max()),
                                  last_push=dict(alive=int(info[2]), K=int(info[1]), n_out=int(info[1]),
                                                 order_path="global" if info[3] & _lib.WINDOW_ORDER_GLOBAL else "lds", overflow=bool(info[3] & 1)),
                                  batch_pr_clouds_avg_ms=float(batch_ms), ratio_push_over_batch=float(np.median(per_push) / batch_ms), **box))
                del g
                win.close()
            ctx.close()
    for l in lines:
        print(json.dumps(l))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
