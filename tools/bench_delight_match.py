"""The device-resident DELIGHT matcher (matcher.DelightMatcher / pr_delight_*) on one MI355X: DB build, match time at m = 4096 / 64 / 1
(k = 1, 5), the online step (match one cloud + append it), the flagged count, the all-exact mode, and the parent path for the same job
(Matcher('delight'): the m x n fp32 matrix and an fp32 selection).  The DB is drawn on the GPU (synth.delight_signatures_torch).
Prints one JSON line per measurement (median and min .. max over the repetitions).
  python tools/bench_delight_match.py [--n 100000] [--M 4096] [--reps 7] [--m M] [--k K] [--no-parent | --parent-only] [--quick]
--quick: only the k = 1 match at m = M and the parent path (the comparison of DESIGN.md 4.9).
The kernel split comes from runs of their own, one query count and k each so that a kernel's calls are alike:
  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_delight_match.py --reps 3 --m 1024 --k 1 --n 20000 --no-parent"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so_dso_place_recognition_amd import synth  # noqa: E402
from so_dso_place_recognition_amd.matcher import DelightMatcher, Matcher  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    """ms of reps calls (events on the current stream, synchronised): median, min, max"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(ms=float(np.median(out)), ms_min=float(min(out)), ms_max=float(max(out)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--M", type=int, default=4096, help="the largest query count")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--m", type=int, default=0, help="only this query count")
    ap.add_argument("--k", type=int, default=0, help="only this k")
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--parent-only", action="store_true")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    n, M, steps = a.n, a.M, 32
    db = synth.delight_signatures_torch(21, n + steps)
    q = synth.delight_signatures_torch(22, M)
    base = db[:16 * n]
    torch.cuda.synchronize()
    if not a.parent_only:
        mt = DelightMatcher(M, n + steps)
        mt.pack_database(base)
        emit(what="build", n=n, device_bytes=mt.device_bytes, bytes_per_signature=49668, **timed(lambda: mt.pack_database(base), a.reps))
        only = a.m or a.k or a.quick
        for m in ((a.m,) if a.m else (M,) if a.quick else (M, 64, 1)):
            qm = q[:16 * m].contiguous()
            for k in ((a.k,) if a.k else (1,) if a.quick else (1, 5)):
                mt.match(qm, k=k)
                t = timed(lambda: mt.match(qm, k=k), a.reps)
                emit(what="match", n=n, m=m, k=k, flagged=mt.flagged_count(), queries_per_s=m / t["ms"] * 1e3, **t)
        if not only:
            mt.set_exact(True)
            for mx in (1, 64):
                qm = q[:16 * mx].contiguous()
                mt.match(qm, k=1)
                emit(what="match, every query from its exact row", n=n, m=mx, k=1, **timed(lambda: mt.match(qm, k=1), max(2, a.reps // 2)))
            mt.set_exact(False)
            at = [n]

            def online():
                r = db[16 * at[0]:16 * (at[0] + 1)]
                mt.match(r, k=1, mask_width=50, q_row0=at[0])
                mt.append_database(r)
                at[0] += 1
            online()
            emit(what="online step (match 1 + append 1)", n=n, **timed(online, min(steps - 1, 3 * a.reps)))
        mt.close()
    if not a.no_parent and not a.m and not a.k:
        pm = Matcher("delight", M, n)
        pm.pack_database(base)
        pm.match(q, 0, 2.0, 1)
        emit(what="parent path: Matcher('delight'), m x n fp32 matrix, fp32 selection", n=n, m=M, k=1,
             **timed(lambda: pm.match(q, 0, 2.0, 1), a.reps))
        pm.close()


if __name__ == "__main__":
    main()
