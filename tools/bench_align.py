#!/usr/bin/env python3
"""Cost of the alignment of matched pairs (align.hip, pr_align_pairs_dev): m = 4096 queries x k in {1, 5} pairs against a resident
n-entry DB, for SC (both channels), M2DP (both channels) and the fused form (all four), with the pairs spread over the whole DB
(random rows: the DB entries come from HBM, not from cache).  One JSON line per (form, k): ms per call (HIP events around `reps`
back-to-back calls on one stream, after a warm-up).  usage: python tools/bench_align.py [n] [m] [reps]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from so_dso_place_recognition_amd import _lib, api, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
m = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
dev = torch.device("cuda", 0)
ctx = api.Context(0, stream=int(torch.cuda.current_stream(dev).cuda_stream))
sc_db = synth.sc_database_torch(45, n, device=dev)
m2_db = synth.m2dp_database_torch(43, n, device=dev)
sc_q = synth.sc_database_torch(46, m, device=dev)
m2_q = synth.m2dp_database_torch(44, m, device=dev)
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
g = torch.Generator(device=dev)
g.manual_seed(7)
for k in (1, 5):
    idx = torch.randint(0, n, (m, k), generator=g, device=dev, dtype=torch.int32)
    var = torch.empty((m, k, 4), dtype=torch.int32, device=dev)
    dist = torch.empty((m, k, 4), dtype=torch.float64, device=dev)
    for form, (qs, ds, qm, dm) in (("sc", (sc_q, sc_db, None, None)), ("m2dp", (None, None, m2_q, m2_db)), ("fused", (sc_q, sc_db, m2_q, m2_db))):
        def call():
            ctx.check(ctx.lib.pr_align_pairs_dev(ctx.h, p(qs), p(ds), _lib.F64, p(qm), p(dm), _lib.F64, m, n, 0, k, p(idx), p(var), p(dist)))
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        found = int((var[..., :2] >= 0).sum().item()) if qs is not None else int((var[..., 2:] >= 0).sum().item())
        print(json.dumps({"form": form, "n": n, "m": m, "k": k, "pairs": m * k, "ms": round(ms, 4), "us_per_pair": round(1e3 * ms / (m * k), 4),
                          "variants_found": found}), flush=True)
ctx.close()
