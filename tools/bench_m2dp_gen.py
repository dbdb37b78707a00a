#!/usr/bin/env python3
"""M2DP generation timing: the figures of bench.py's config 2 (pr_m2dp_generate_dev on synthetic 50 000-point clouds, 128 and 1024 clouds; one
warm-up call, then the mean of 2 timed calls, as bench.py's timed(reps=2)), SAMPLES such figures per process, one JSON line.
    python tools/bench_m2dp_gen.py [SAMPLES]
PR_AMD_LIB selects the library, so two builds can be measured alternately, a fresh process each (profiles/m2dp_svd_ties/bench.jsonl)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from so_dso_place_recognition_amd import synth
from so_dso_place_recognition_amd.api import Context

samples = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda", 0)
N, PTS = 1024, 50_000
xyz, it, offs = synth.scene_clouds_torch(42, N, PTS, device=dev)
ctx = Context(0)
P = lambda t: t.data_ptr()
out = {"bench": "m2dp_generate_dev", "points_per_cloud": PTS}
for n in (128, 1024):
    sig = torch.empty((4 * n, 384), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    res = []
    for _ in range(samples):
        ts = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(); ctx.check(ctx.lib.pr_m2dp_generate_dev(ctx.h, P(xyz), P(it), P(offs), n, 45.0, P(sig))); b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        res.append(float(np.mean(ts[1:])))
    out[f"ms_{n}_clouds"] = res
pr = torch.cuda.get_device_properties(0)
out.update(device=pr.name, compute_units=pr.multi_processor_count, torch=torch.__version__, hip=torch.version.hip)
print(json.dumps(out), flush=True)
