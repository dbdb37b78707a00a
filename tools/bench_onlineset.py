#!/usr/bin/env python3
"""The online signature sets (pr_onlineset).  Method as tools/bench_online.py: wall time from the call to the end of a
stream synchronisation, medians over --iters after --warmup warm-ups.  Recorded, not gated.
  onlineset_step   the 140-pose KITTI seq07 drive of tools/bench_online.py (60 points per pose): the signatures of its 110 emitting
                   keyframes are generated once (CloudWindow + the generators); then, per keyframe, microseconds (median over the
                   replays of the drive, then median and max over the keyframes) of match + append in two forms:
                     eager_host   the host-counted loop: FusedMatcher.match (from 3 rows on, q_row0 = the count) plus the two
                                  append_database calls; DelightMatcher.match (from 1 row on) plus append_database
                     graph        ONE replay of the captured api.OnlineSet.step_torch (the count lives on the device)
  onlineset_match  match_torch alone (k = 1, mask 0) at --rows rows of synthetic signatures, milliseconds, per kind

    python tools/bench_onlineset.py [--iters 10] [--warmup 2] [--rows 3475] [--out profiles/onlineset/bench.jsonl]"""
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
    ap.add_argument("--rows", type=int, default=3475)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import helpers
    from so_dso_place_recognition_amd import api, synth
    from so_dso_place_recognition_amd.matcher import DelightMatcher, FusedMatcher, _stream_context
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
    MASK, K = 5, 1
    lines = []
    p_ = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        lib = ctx.lib
        cap, mx = int(cuts[-1]), int(np.diff(cuts).max())
        # ---- the drive's signatures, once
        win = api.CloudWindow(ctx, 45.0, False, cap, mx, cap)
        out = win.empty_out()
        x = torch.zeros((mx, 3), dtype=torch.float64, device="cuda"); ii = torch.zeros(mx, dtype=torch.float32, device="cuda")
        n = torch.zeros(1, dtype=torch.int32, device="cuda")
        sc, m2, de = [], [], []
        for p in range(P):
            k = int(cuts[p + 1] - cuts[p])
            x[:k].copy_(torch.from_numpy(xyz[cuts[p]:cuts[p + 1]])); ii[:k].copy_(torch.from_numpy(it[cuts[p]:cuts[p + 1]])); n.fill_(k)
            win.push_torch(torch.from_numpy(w[p].reshape(12).copy()).cuda(), x, ii, n, out=out)
            st.synchronize()
            if not int(out["info"].cpu()[0]):
                continue
            s0 = torch.zeros((1, 2400), dtype=torch.float64, device="cuda"); s1 = torch.zeros((4, 384), dtype=torch.float64, device="cuda")
            s2 = torch.zeros((16, 256), dtype=torch.float64, device="cuda")
            g_ = (p_(out["xyz"]), p_(out["inten"]), p_(out["offs"]))
            ctx.check(lib.pr_sc_generate_frames_dev(ctx.h, *g_, 1, 45.0, p_(out["frame"]), 1, p_(s0)))
            ctx.check(lib.pr_m2dp_generate_frames_dev(ctx.h, *g_, 1, 45.0, p_(out["frame"]), 1, p_(s1)))
            ctx.check(lib.pr_delight_generate_frames_dev(ctx.h, *g_, 1, p_(out["frame"]), p_(s2)))
            sc.append(s0); m2.append(s1); de.append(s2)
        win.close()
        KF = len(sc)
        for kind in ("fused", "delight"):
            sigs = list(zip(sc, m2)) if kind == "fused" else de
            static = tuple(torch.zeros_like(t) for t in (sigs[0] if kind == "fused" else (sigs[0],)))
            arg = static if kind == "fused" else static[0]
            for form in ("eager_host", "graph"):
                mt = oset = g = None

                def fresh():
                    if kind == "fused":
                        m = FusedMatcher(1, KF, ctx=ctx)
                        m.sc.reserve_database(); m.m2.reserve_database()
                        m.n = 0
                    else:
                        m = DelightMatcher(1, KF, ctx=ctx)
                        m.reserve_database()
                    return m

                def eager():
                    if kind == "fused":
                        if mt.n >= 3:
                            mt.match(static[0], static[1], MASK, 2.0, K, q_row0=mt.n)
                        mt.sc.append_database(static[0]); mt.m2.append_database(static[1])
                        mt.n = mt.sc.n
                    else:
                        if mt.n >= 1:
                            mt.match(static[0], MASK, K, q_row0=mt.n)
                        mt.append_database(static[0])

                if form == "graph":
                    oset = api.OnlineSet(ctx, kind, KF, max_k=K)
                    mout = (torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros((1, K), dtype=torch.float64, device="cuda"))
                    oinfo = torch.zeros(4, dtype=torch.int32, device="cuda")
                    oset.step_torch(arg, MASK, 2.0, K, out=mout, info=oinfo)
                    st.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=st):
                        oset.step_torch(arg, MASK, 2.0, K, out=mout, info=oinfo)
                times = np.zeros((a.iters, KF))
                for r in range(a.warmup + a.iters):
                    if oset is not None:
                        oset.reset()
                    else:                                                           # (a host-counted database only grows: a fresh matcher per drive)
                        if mt is not None:
                            mt.close()
                        mt = fresh()
                    for j in range(KF):
                        for t, s in zip(static, sigs[j] if kind == "fused" else (sigs[j],)):
                            t.copy_(s)
                        st.synchronize()
                        t0 = time.perf_counter()
                        if g is None:
                            eager()
                        else:
                            g.replay()
                        st.synchronize()
                        if r >= a.warmup:
                            times[r - a.warmup, j] = (time.perf_counter() - t0) * 1e6
                per_kf = np.median(times, axis=0)
                rows = oset.count()[0] if oset is not None else mt.n
                lines.append(dict(bench="onlineset_step", kind=kind, drive=name, poses=P, per_pose=per_pose, keyframes=KF, form=form, mask_width=MASK,
                                  k=K, iters=a.iters, warmup=a.warmup, us_per_keyframe_median=float(np.median(per_kf)),
                                  us_per_keyframe_max=float(per_kf.max()), us_last_keyframe=float(per_kf[-1]), rows=rows, **box))
                del g
                if oset is not None:
                    oset.close()
                if mt is not None:
                    mt.close()

        cnt = a.rows
        for kind in ("fused", "delight"):
            oset = api.OnlineSet(ctx, kind, cnt, max_k=1)
            if kind == "fused":                                                     # (caller-owned buffers: the rows and the count written directly)
                oset.sc.copy_(synth.sc_database_torch(77, cnt)); oset.m2dp.copy_(synth.m2dp_database_torch(79, cnt))
                q = (oset.sc[cnt // 3:cnt // 3 + 1].clone(), oset.m2dp[4 * (cnt // 3):4 * (cnt // 3) + 4].clone())
                q[0][0, :20] = 0.0                                                  # a near-copy of one row
            else:
                oset.delight.copy_(synth.delight_signatures_torch(81, cnt))
                q = oset.delight[16 * (cnt // 3):16 * (cnt // 3) + 16].clone()
                q[0, :20] = 0.0
            oset.state[0] = cnt
            mout = oset.match_torch(q, 0, 2.0, 1)
            st.synchronize()
            t = []
            for r in range(a.warmup + a.iters):
                st.synchronize()
                t0 = time.perf_counter()
                oset.match_torch(q, 0, 2.0, 1, out=mout)
                st.synchronize()
                if r >= a.warmup:
                    t.append((time.perf_counter() - t0) * 1e3)
            lines.append(dict(bench="onlineset_match", kind=kind, rows=cnt, m=1, k=1, iters=a.iters, warmup=a.warmup, match_ms_median=float(np.median(t)),
                              top1=int(mout[0][0, 0]), planted=cnt // 3, **box))
            oset.close()
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
