#!/usr/bin/env python3
"""The resident keyframe map (pr_map) on the 140-pose KITTI seq07 drive of tools/bench_window.py (60 points per pose).
Per EMITTING keyframe, the wall time from the call to the end of a stream synchronisation, median over --iters replays of the drive after
--warmup warm-ups, then the median and the max over the keyframes:
  push               the window push alone (the common part; about a millisecond: its one-lane order kernel)
  push_cat           how a caller manages without a map (the comparison, not the code under test): push, read n_out back, torch.cat onto
                     the CSR tensors xyz / inten / offs / frames
  push_append        push -> append_push, eager; push_append_graph: the pair captured once in a graph and replayed
  append_alone       the push is enqueued and synchronised first, then append_push alone is timed (eager, and captured: _graph)
  cat_alone          the same for the read-back + torch.cat
The *_alone forms are there because the push dominates the pair: the append's launches are enqueued while the push still runs, so the
pair's time barely moves with what follows the push.
Then one verify_dev from the map at m = 1, k = 2: the last keyframe's SC row matched against the rows of the drive (the 5 neighbouring
keyframes masked), align + seed + ICP + choice, median over --iters calls.  The expectation on record: an append is three small launches,
launch-bound - a few launch times, whatever the cloud's size here.

    python tools/bench_map.py [--iters 10] [--warmup 2] [--out profiles/map/bench.jsonl]"""
import argparse
import ctypes as C
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import helpers
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import Matcher, _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    poses = os.path.join(ROOT, "tests", "golden", "kitti_seq07", "poses_history_file.txt")
    tmp = tempfile.mkdtemp()
    name, per_pose = "seq07_60", 60
    pts = os.path.join(tmp, name + ".txt")
    helpers.write_synthetic_points(poses, pts, per_pose=per_pose, max_poses=140)
    short = os.path.join(tmp, name + "_poses.txt")
    open(short, "w").write("\n".join([l for l in open(poses).read().split("\n") if l.strip()][:140]) + "\n")
    pid, w, qid, xyz, it = api.read_poses_points(short, pts)
    cuts = api.split_points_by_pose(pid, qid)
    P = len(pid)
    lines = []
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        cap, mx = int(cuts[-1]), int(np.diff(cuts).max())
        kcap, pcap = P, cap * (P - 30)
        pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((mx, 3), dtype=torch.float64, device="cuda")
        ii = torch.zeros(mx, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
        kid = torch.zeros(1, dtype=torch.int32, device="cuda"); info = torch.zeros(4, dtype=torch.int32, device="cuda")
        dw = torch.from_numpy(w).cuda(); dx = torch.from_numpy(xyz).cuda(); di = torch.from_numpy(it).cuda()
        dn = torch.from_numpy(np.diff(cuts).astype(np.int32)).cuda(); dpid = torch.from_numpy(pid.astype(np.int32)).cuda()

        def load(p):
            k = int(cuts[p + 1] - cuts[p])
            pose.copy_(dw[p]); x[:k].copy_(dx[cuts[p]:cuts[p + 1]]); ii[:k].copy_(di[cuts[p]:cuts[p + 1]]); n.copy_(dn[p:p + 1]); kid.copy_(dpid[p:p + 1])

        km = api.KeyframeMap(ctx, kcap, pcap, cap)
        for form in ("push", "push_cat", "cat_alone", "append_alone", "append_alone_graph", "push_append", "push_append_graph"):
            win = api.CloudWindow(ctx, 45.0, False, cap, mx, cap)
            out = win.empty_out()
            csr = {}

            def fresh():
                csr.update(xyz=torch.zeros((0, 3), dtype=torch.float64, device="cuda"), inten=torch.zeros(0, dtype=torch.float32, device="cuda"),
                           offs=torch.zeros(1, dtype=torch.int64, device="cuda"), frames=torch.zeros((0, 16), dtype=torch.float64, device="cuda"))

            def tail():
                if "append" in form:
                    km.append_push(out, pose=pose, id=kid, info=info)
                elif "cat" in form:
                    h = out["info"].cpu()                                           # the read-back a caller cannot avoid
                    if int(h[0]):
                        k = int(h[1])
                        csr["xyz"] = torch.cat([csr["xyz"], out["xyz"][:k]]); csr["inten"] = torch.cat([csr["inten"], out["inten"][:k]])
                        csr["offs"] = torch.cat([csr["offs"], csr["offs"][-1:] + k]); csr["frames"] = torch.cat([csr["frames"], out["frame"][None]])

            alone = "alone" in form

            def step():                                                             # what the clock sees
                if not alone:
                    win.push_torch(pose, x, ii, n, out=out)
                tail()

            load(0); fresh()
            win.push_torch(pose, x, ii, n, out=out)
            tail()
            st.synchronize()
            g = None
            if form.endswith("_graph"):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st):
                    step()
            times = np.zeros((a.iters, P))
            for r in range(a.warmup + a.iters):
                win.reset(); km.reset(); fresh()
                for p in range(P):
                    load(p)
                    if alone:
                        win.push_torch(pose, x, ii, n, out=out)
                    st.synchronize()
                    t0 = time.perf_counter()
                    if g is None:
                        step()
                    else:
                        g.replay()
                    st.synchronize()
                    if r >= a.warmup:
                        times[r - a.warmup, p] = (time.perf_counter() - t0) * 1e6
            per_kf = np.median(times, axis=0)[30:]                                  # (no reset in this drive: pushes 31 .. 140 emit)
            keyframes, points, flags = km.count()
            lines.append(dict(bench="map_append", drive=name, poses=P, per_pose=per_pose, form=form, iters=a.iters, warmup=a.warmup,
                              us_per_keyframe_median=float(np.median(per_kf)), us_per_keyframe_max=float(per_kf.max()),
                              map=dict(keyframes=keyframes, points=points, flags=flags) if "append" in form else None,
                              last_cloud_points=int(out["info"].cpu()[1]), **box))
            del g
            win.close()

        # one verify_dev from the map (left by the last replay of the graph form: the whole drive): m = 1, k = 2
        keyframes, points, flags = km.count()
        assert keyframes == P - 30 and flags == 0, (keyframes, flags)
        mt = Matcher("sc", 1, keyframes, ctx=ctx)
        sig = torch.empty((keyframes, 2400), dtype=torch.float64, device="cuda")
        p_ = lambda t: C.c_void_p(t.data_ptr())
        ctx.check(ctx.lib.pr_sc_generate_frames_dev(ctx.h, p_(km.xyz), p_(km.inten), p_(km.offs), keyframes, 45.0, p_(km.frames), 1, p_(sig)))
        mt.pack_database(sig)
        q = keyframes - 1
        o = km.offs[q:q + 2].cpu()
        cq = (km.xyz[int(o[0]):int(o[1])].clone(), torch.tensor([0, int(o[1] - o[0])], dtype=torch.int64, device="cuda"))
        fq = km.frames[q:q + 1].clone()
        idx, score = mt.match(sig[q:q + 1].clone(), 5, 2.0, 2, q_row0=q)
        res = km.verify_dev(mt, idx, cq, fq, cap, hypotheses=1)
        st.synchronize()
        t = []
        for r in range(a.warmup + a.iters):
            st.synchronize()
            t0 = time.perf_counter()
            km.verify_dev(mt, idx, cq, fq, cap, hypotheses=1, out=res)
            st.synchronize()
            if r >= a.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        stats = np.frombuffer(res[1].cpu().numpy().tobytes(), api.ICP_STATS)
        lines.append(dict(bench="map_verify_dev", drive=name, m=1, k=2, hypotheses=1, query_keyframe=q, query_points=int(o[1] - o[0]),
                          candidates=idx.cpu().numpy().reshape(-1).tolist(), max_src_pts=cap, max_dst_pts=cap, iters=a.iters, warmup=a.warmup,
                          verify_ms_median=float(np.median(t)), icp_iters=stats["iters"].tolist(), status=stats["status"].tolist(),
                          fitness=stats["fitness"].tolist(), accepted=res[2].cpu().numpy().reshape(-1).astype(int).tolist(), **box))
        mt.close(); km.close(); ctx.close()
    for l in lines:
        print(json.dumps(l))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
