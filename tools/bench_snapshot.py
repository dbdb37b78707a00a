#!/usr/bin/env python3
"""Snapshots (pr_snapshot).  Method as tools/bench_session.py and 4.15: wall time from the call to the end of a stream
synchronisation, median (min .. max) over --iters after --warmup warm-ups.  Recorded, not gated.  Two states:
  seq07   the 110 keyframes of the committed seq07 drive: the batch pre-stage's clouds, their SC signatures as the online database, a log
          of 100 edges
  seq00   a synthetic state of seq00's size: 3475 keyframes x 400 points, both online databases (SC and M2DP), 173 edges
and per state: pack_torch and unpack_torch (device forms, eager), save and load (host forms, a file in --dir), and in the SAME run a plain
device-to-device copy of the same number of bytes (torch's copy_ of a uint8 tensor on the same stream: one hipMemcpyAsync) - what the
kernels are held to: they read the data once (pack) or twice (unpack), so about 2 - 3 x the copy is what a memory-bound form gives.

    python tools/bench_snapshot.py [--iters 10] [--warmup 2] [--dir DIR] [--out profiles/snapshot/bench.jsonl]"""
import argparse
import json
import os
import socket
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import snapshot_rig
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import _stream_context
    from so_dso_place_recognition_amd.snapshot import Snapshot
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    work = a.dir or tempfile.mkdtemp(prefix="bench_snapshot_")
    os.makedirs(work, exist_ok=True)
    lines = []
    rng = np.random.default_rng(7)
    cuda = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()

    def edges(g, E, n):
        g.edge_ij[:E] = cuda(np.stack([rng.integers(0, n // 2, E), rng.integers(n // 2, n, E)], 1), np.int32)
        g.edge_Z[:E] = cuda(rng.standard_normal((E, 12)), np.float64)
        g.edge_w[:E] = torch.tensor([100.0, 10.0], dtype=torch.float64, device="cuda")
        g.state[0] = E

    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        for name in ("seq07", "seq00"):
            if name == "seq07":
                cl = snapshot_rig.seq07_batch_clouds(os.path.join(ROOT, "tests", "golden"), work)
                n, pts = len(cl["ids"]), int(cl["offs"][-1])
                km = api.KeyframeMap(ctx, 112, 1 << 18, 9000)
                km.xyz[:pts] = cuda(cl["xyz"], np.float64); km.inten[:pts] = cuda(cl["inten"], np.float32)
                km.offs[:n + 1] = cuda(cl["offs"], np.int64); km.frames[:n] = cuda(cl["frames"], np.float64)
                km.poses[:n] = cuda(cl["poses"], np.float64); km.ids[:n] = cuda(cl["ids"], np.int32)
                dbs = [api.OnlineDatabase(ctx, "sc", 112)]
                dbs[0].sig[:n] = cuda(api.sc_generate(cl["xyz"], cl["inten"], cl["offs"]), np.float64)
                E, EC = 100, 300
            else:
                n, per = 3475, 400
                pts = n * per
                km = api.KeyframeMap(ctx, 3500, pts + 4096, 9000)
                km.xyz[:pts] = torch.randn((pts, 3), dtype=torch.float64, device="cuda") * 30.0
                km.inten[:pts] = torch.rand(pts, dtype=torch.float32, device="cuda")
                km.offs[:n + 1] = torch.arange(n + 1, dtype=torch.int64, device="cuda") * per
                km.frames[:n] = torch.randn((n, 16), dtype=torch.float64, device="cuda"); km.poses[:n] = torch.randn((n, 12), dtype=torch.float64, device="cuda")
                km.ids[:n] = torch.arange(n, dtype=torch.int32, device="cuda")
                dbs = [api.OnlineDatabase(ctx, "sc", 3500), api.OnlineDatabase(ctx, "m2dp", 3500)]
                dbs[0].sig[:n] = torch.rand((n, 2400), dtype=torch.float64, device="cuda")
                dbs[1].sig[:4 * n] = torch.randn((4 * n, 384), dtype=torch.float64, device="cuda")
                E, EC = 173, 256
            km.state[0] = n
            for d in dbs:
                d.state[0] = n
            g = api.PoseGraph(ctx, km.keyframe_capacity, EC)
            edges(g, E, n)
            snap = Snapshot(ctx, map=km, online=dbs, graphs=(g,))
            bound = snap.bound()
            blob = torch.zeros(bound, dtype=torch.uint8, device="cuda")
            info = torch.zeros(4, dtype=torch.int64, device="cuda")
            snap.pack_torch(blob, info=info)
            st.synchronize()
            nbytes, flags = int(info[0]), int(info[2])
            assert flags == 0 and nbytes <= bound
            path = os.path.join(work, name + ".snap")
            other = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            runs = {"pack": lambda: snap.pack_torch(blob, info=info), "unpack": lambda: snap.unpack_torch(blob, nbytes, info=info),
                    "save": lambda: snap.save(path), "load": lambda: snap.load(path), "copy_d2d": lambda: other.copy_(blob[:nbytes])}
            res = {k: timed(st, f, a.warmup, a.iters) for k, f in runs.items()}
            st.synchronize()
            assert info.cpu().tolist() == [len(dbs) + 9, -1, 0, 0]                  # the last device call was an unpack that passed
            copy = res["copy_d2d"]["ms_median"]
            for k, t in res.items():
                lines.append(dict(bench=k, state=name, keyframes=n, points=pts, edges=E, databases=len(dbs), bytes=nbytes, bound=bound,
                                  gb_per_s=nbytes / (t["ms_median"] * 1e-3) / 1e9, x_copy=t["ms_median"] / copy, iters=a.iters, **t, **box))
                print(json.dumps(lines[-1]), flush=True)
            snap.close(); g.close()
            for d in dbs:
                d.close()
            km.close()
            del blob, other
            torch.cuda.empty_cache()
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
