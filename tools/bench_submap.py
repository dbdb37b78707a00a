#!/usr/bin/env python3
"""The local submaps (pr_submap).  Method as tools/bench_graph.py (4.15): wall time from the call to the end of a stream
synchronisation, median (min .. max) over --iters after --warmup warm-ups, eager and as a graph replay.  Recorded, not gated.
  build_dev   c = 32 and 1024 slots with w = 2 and 5 on a map of 4096 keyframes of 400 points each (slot_capacity = c, w_max = w,
              centres spread over the map, no avoid list); points and bytes = what the gather reads plus writes (24 B in and 24 B out a point)
  d2d_copy    in the same run, a device-to-device copy of points x 24 B: it reads and writes the bytes the gather reads and writes

    python tools/bench_submap.py [--iters 10] [--warmup 2] [--out profiles/submap/bench.jsonl]"""
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
    import submap_cases as cases
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    lines = []
    st = torch.cuda.Stream()
    KF, PER = 4096, 400

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

    def record(**line):
        lines.append(dict(iters=a.iters, **line, **box))
        print(json.dumps(lines[-1]), flush=True)

    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        km = api.KeyframeMap(ctx, KF, KF * PER, PER)
        rng = np.random.default_rng(1)
        _, _, poses = cases.random_map([0] * KF, seed=1)
        km.xyz.copy_(torch.from_numpy(rng.normal(size=(KF * PER, 3)) * 10.0))
        km.offs.copy_(torch.arange(KF + 1, dtype=torch.int64) * PER)
        km.poses.copy_(torch.from_numpy(poses))
        km.state.copy_(torch.tensor([KF, 0, 0, 0], dtype=torch.int32))
        for c in (32, 1024):
            for w in (2, 5):
                L = 2 * w + 1
                sb = api.SubmapBuilder(ctx, c, w, c * L * PER, PER, KF)
                cen = torch.from_numpy(rng.integers(w, KF - w, c).astype(np.int32)).cuda()
                fn = lambda: sb.build_torch(km, cen, w=w, max_pts=L * PER)
                out = fn()
                st.synchronize()
                info = out.info.cpu().numpy()
                points = int(info[1]) + (int(info[2]) << 32)
                assert points == c * L * PER and int(info[0]) == c and int(info[3]) == 0
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st):
                    fn()
                res = {}
                for form, f in (("eager", fn), ("graph", graph.replay)):
                    res[form] = timed(f)
                    record(bench="build_dev", form=form, c=c, w=w, keyframes=KF, cloud_points=PER, points=points, bytes_read_plus_written=48 * points,
                           gbps=48 * points / res[form]["ms_median"] / 1e6, scratch_bytes=sb.scratch_bytes(), **res[form])
                del graph
                src = torch.empty(points * 3, dtype=torch.float64, device="cuda").normal_()
                dst = torch.empty_like(src)
                t = timed(lambda: dst.copy_(src))
                record(bench="d2d_copy", form="eager", c=c, w=w, points=points, bytes_read_plus_written=48 * points, gbps=48 * points / t["ms_median"] / 1e6,
                       build_graph_over_copy=res["graph"]["ms_median"] / t["ms_median"], **t)
                del src, dst
                sb.close()
        km.close()
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
