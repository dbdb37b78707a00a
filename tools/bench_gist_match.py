"""The device-resident GIST matcher (matcher.GistMatcher / pr_gist_*) on one MI355X: DB build, match time at m = 4096 / 64 / 1 (k = 1, 5),
the online step (match one image + append it), the flagged count, the all-exact mode, and the parent path for the same job
(pr_match_topk_cols('gist') with host buffers, which materialises the m x n fp32 matrix).  The DB is drawn on the GPU
(synth.gist_signatures_torch).  Prints one JSON line per measurement (median and min .. max over the repetitions).
  python tools/bench_gist_match.py [--n 100000] [--cols 512] [--reps 7] [--m M] [--k K] [--no-parent | --parent-only]
PR_GIST_CENTRE=0 in the environment packs the rows uncentred (recorded in every line as "centre").
The kernel split comes from runs of their own, one query count and k each so that a kernel's calls are alike:
  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_gist_match.py --reps 3 --m 4096 --k 1 --no-parent
  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_gist_match.py --reps 3 --parent-only"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so_dso_place_recognition_amd import api, synth  # noqa: E402
from so_dso_place_recognition_amd.matcher import GistMatcher  # noqa: E402


def emit(**kw):
    kw.update(centre=os.environ.get("PR_GIST_CENTRE", "1"))
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
    ap.add_argument("--cols", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--m", type=int, default=0, help="only this query count")
    ap.add_argument("--k", type=int, default=0, help="only this k")
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--parent-only", action="store_true")
    a = ap.parse_args()
    n, cols, M, steps = a.n, a.cols, 4096, 64
    db = synth.gist_signatures_torch(21, n + steps, cols)
    q = synth.gist_signatures_torch(22, M, cols)
    torch.cuda.synchronize()
    if a.parent_only:
        parent(a, q, db[:n], n, cols, M)
        return
    mt = GistMatcher(M, n + steps, cols)
    base = db[:n]
    mt.pack_database(base)
    emit(what="build", n=n, cols=cols, device_bytes=mt.device_bytes, **timed(lambda: mt.pack_database(base), a.reps))
    for m in ((a.m,) if a.m else (M, 64, 1)):
        qm = q[:m].contiguous()
        for k in ((a.k,) if a.k else (1, 5)):
            mt.match(qm, k=k)
            t = timed(lambda: mt.match(qm, k=k), a.reps)
            emit(what="match", n=n, cols=cols, m=m, k=k, flagged=mt.flagged_count(), queries_per_s=m / t["ms"] * 1e3, **t)
    if a.m or a.k:
        mt.close()
        return
    mt.set_exact(True)
    qm = q[:256].contiguous()
    mt.match(qm, k=1)
    emit(what="match, every query from its exact row", n=n, cols=cols, m=256, k=1, **timed(lambda: mt.match(qm, k=1), max(2, a.reps // 2)))
    mt.set_exact(False)
    at = [n]

    def online():
        r = db[at[0]:at[0] + 1]
        mt.match(r, k=1, mask_width=50, q_row0=at[0])
        mt.append_database(r)
        at[0] += 1
    online()
    emit(what="online step (match 1 + append 1)", n=n, cols=cols, **timed(online, min(steps - 1, 3 * a.reps)))
    mt.close()
    if not a.no_parent:
        parent(a, q, base, n, cols, M)


def parent(a, q, base, n, cols, M):
    h1, h2 = q.cpu().numpy(), base.cpu().numpy()
    api.match_topk("gist", h1[:64], h2[:1000], 0, 2.0, 1)
    emit(what="parent path: pr_match_topk_cols('gist'), host buffers, m x n fp32 matrix", n=n, cols=cols, m=M, k=1,
         **timed(lambda: api.match_topk("gist", h1, h2, 0, 2.0, 1), max(2, a.reps // 2)))


if __name__ == "__main__":
    main()
