#!/usr/bin/env python3
"""The online signature database (pr_online).  Method as tools/bench_map.py: wall time from the call to the end of a
stream synchronisation, medians over --iters after --warmup warm-ups.  Recorded, not gated.
  online_step   the 140-pose KITTI seq07 drive of tools/bench_map.py (60 points per pose), microseconds per EMITTING keyframe (median
                over the replays of the drive, then median and max over the keyframes) for the whole step
                push -> generate -> match -> append -> map append -> align -> verify, in two forms:
                  eager_host   the loop of INTEGRATION.md 3 before pr_online: push + generate, the push's info read back, and on an emitted
                               keyframe Matcher.match (from 3 rows on) + append_database + map append + verify_dev, all eager
                  graph        ONE replay of the captured step over api.OnlineDatabase (no host decision)
  online_match  match_torch alone (k = 1, mask 0) at --counts rows beside Matcher.match with m = 1 on the same rows (SC, synthetic
                signatures), milliseconds, and the ratio - at 100 000 rows the number that decides about a spectra form of the rows kernel

    python tools/bench_online.py [--iters 10] [--warmup 2] [--counts 3475,100000] [--out profiles/online/bench.jsonl]"""
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
    ap.add_argument("--counts", default="3475,100000")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import helpers
    from so_dso_place_recognition_amd import api, synth
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
    MASK, K = 5, 1
    lines = []
    p_ = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        cap, mx = int(cuts[-1]), int(np.diff(cuts).max())
        kcap, pcap = P, cap * (P - 30)
        pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((mx, 3), dtype=torch.float64, device="cuda")
        ii = torch.zeros(mx, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
        kid = torch.zeros(1, dtype=torch.int32, device="cuda"); minfo = torch.zeros(4, dtype=torch.int32, device="cuda")
        oinfo = torch.zeros(4, dtype=torch.int32, device="cuda")
        sig = torch.zeros((1, 2400), dtype=torch.float64, device="cuda")
        dw = torch.from_numpy(w).cuda(); dx = torch.from_numpy(xyz).cuda(); di = torch.from_numpy(it).cuda()
        dn = torch.from_numpy(np.diff(cuts).astype(np.int32)).cuda(); dpid = torch.from_numpy(pid.astype(np.int32)).cuda()

        def load(p):
            k = int(cuts[p + 1] - cuts[p])
            pose.copy_(dw[p]); x[:k].copy_(dx[cuts[p]:cuts[p + 1]]); ii[:k].copy_(di[cuts[p]:cuts[p + 1]]); n.copy_(dn[p:p + 1]); kid.copy_(dpid[p:p + 1])

        for form in ("eager_host", "graph"):
            win = api.CloudWindow(ctx, 45.0, False, cap, mx, cap)
            km = api.KeyframeMap(ctx, kcap, pcap, cap)
            out = win.empty_out()
            keep = dict(al=None, v=None)
            mt = odb = None
            if form == "eager_host":
                mt = Matcher("sc", 1, kcap, ctx=ctx)
                mt.reserve_database()
            else:
                odb = api.OnlineDatabase(ctx, "sc", kcap, max_k=K)
                mout = (torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros((1, K), dtype=torch.float64, device="cuda"))

            def front():
                win.push_torch(pose, x, ii, n, out=out)
                ctx.check(ctx.lib.pr_sc_generate_frames_dev(ctx.h, p_(out["xyz"]), p_(out["inten"]), p_(out["offs"]), 1, 45.0, p_(out["frame"]), 1, p_(sig)))

            def step():
                front()
                if form == "eager_host":
                    if int(out["info"].cpu()[0]):                                   # the host decision
                        idx = None
                        if mt.n >= 3:
                            idx, _ = mt.match(sig, MASK, 2.0, K, q_row0=mt.n)
                        mt.append_database(sig)
                        km.append_push(out, pose=pose, id=kid, info=minfo)
                        if idx is not None:
                            keep["v"] = mt.verify_dev(idx, (out["xyz"], out["offs"]), km, out["frame"][None], None, cap, None, hypotheses=1, out=keep["v"])
                else:
                    odb.step_torch(sig, MASK, 2.0, K, emitted=out["info"], out=mout, info=oinfo)
                    km.append_push(out, pose=pose, id=kid, info=minfo)
                    keep["al"] = odb.align(mout[0], sig, out=keep["al"])
                    keep["v"] = km.verify_variants("sc", mout[0], keep["al"][0], (out["xyz"], out["offs"]), out["frame"][None], cap, hypotheses=1,
                                                   out=keep["v"])

            load(0)
            step()
            st.synchronize()
            g = None
            if form == "graph":
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st):
                    step()
            times = np.zeros((a.iters, P))
            for r in range(a.warmup + a.iters):
                win.reset(); km.reset()
                if odb is not None:
                    odb.reset()
                else:                                                               # (a sigset's row count only grows: a fresh matcher per drive)
                    mt.close()
                    mt = Matcher("sc", 1, kcap, ctx=ctx)
                    mt.reserve_database()
                for p in range(P):
                    load(p)
                    st.synchronize()
                    t0 = time.perf_counter()
                    if g is None:
                        step()
                    else:
                        g.replay()
                    st.synchronize()
                    if r >= a.warmup:
                        times[r - a.warmup, p] = (time.perf_counter() - t0) * 1e6
            per_kf = np.median(times, axis=0)[30:]
            rows = odb.count()[0] if odb is not None else mt.n
            lines.append(dict(bench="online_step", drive=name, poses=P, per_pose=per_pose, form=form, mask_width=MASK, k=K, iters=a.iters,
                              warmup=a.warmup, us_per_keyframe_median=float(np.median(per_kf)), us_per_keyframe_max=float(per_kf.max()),
                              us_last_keyframe=float(per_kf[-1]), database_rows=rows, map_keyframes=km.count()[0], **box))
            del g
            if odb is not None:
                odb.close()
            if mt is not None:
                mt.close()
            km.close(); win.close()

        for cnt in [int(c) for c in a.counts.split(",") if c]:
            db = synth.sc_database_torch(77, cnt)
            q = synth.sc_database_torch(78, 1)
            q[0] = db[cnt // 3]
            q[0, :20] = 0.0                                                          # a near-copy of one row
            odb = api.OnlineDatabase(ctx, "sc", cnt, max_k=1)
            odb.sig.copy_(db)                                                        # (caller-owned buffers: the rows and the count written directly)
            odb.state[0] = cnt
            mt = Matcher("sc", 1, cnt, ctx=ctx)
            mt.pack_database(db)
            mout = odb.match_torch(q, 0, 2.0, 1)
            mi, ms = mt.match(q, 0, 2.0, 1)
            st.synchronize()
            same = bool(mi[0, 0] == mout[0][0, 0])
            t = {"online": [], "matcher": []}
            for r in range(a.warmup + a.iters):
                for who in ("online", "matcher"):
                    st.synchronize()
                    t0 = time.perf_counter()
                    if who == "online":
                        odb.match_torch(q, 0, 2.0, 1, out=mout)
                    else:
                        mt.match(q, 0, 2.0, 1)
                    st.synchronize()
                    if r >= a.warmup:
                        t[who].append((time.perf_counter() - t0) * 1e3)
            on, fast = float(np.median(t["online"])), float(np.median(t["matcher"]))
            lines.append(dict(bench="online_match", type="sc", rows=cnt, m=1, k=1, iters=a.iters, warmup=a.warmup, online_match_ms_median=on,
                              matcher_match_ms_median=fast, ratio_online_to_matcher=on / fast, same_top1=same,
                              score_difference=float((mout[1][0, 0] - ms[0, 0]).abs()), **box))
            odb.close(); mt.close()
            del db
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
