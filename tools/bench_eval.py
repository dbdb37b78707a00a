#!/usr/bin/env python3
"""The device evaluation (csrc/eval.hip) against the host pr_precision_recall on the same inputs, cols = 3:
self-evaluation at n = 3 475 (the reference's shape, mask 100) and n = 100 000, and m = 1 / m = 64 against n = 100 000 (online use).
Per shape one JSON line: the ground-truth launch (pr_ground_truth_pairs_dev), the whole evaluation (pr_precision_recall_dev), the sweep
(their difference), the ordered trapz chain on its own (pr_trapz_dev) - HIP-event times on the context's stream, median of --iters - and the
host function's wall time (one thread, as it is) where --host-max-pairs allows it.

    python tools/bench_eval.py [--iters 5] [--only 3475] [--host-max-pairs 1e10] [--out profiles/eval/bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((3475, 3475, 100), (100000, 100000, 100), (1, 100000, 0), (64, 100000, 0))


def drive(seed, m, n):
    """A drive that passes every place twice and per-query matches that find most of the loops."""
    rng = np.random.default_rng(seed)
    base = np.cumsum(rng.normal(0, 1.5, ((n + 1) // 2, 3)), 0)
    gt2 = np.concatenate([base, base[: n - len(base)] + rng.normal(0, 0.5, (n - len(base), 3))])
    gt1 = gt2[:m] + 0.0 if m == n else gt2[rng.integers(n // 2, n, m)] + rng.normal(0, 0.5, (m, 3))
    idx = rng.integers(0, n, m).astype(np.int32)
    v = rng.random(m)
    return gt1, gt2, v, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", type=int, default=0, help="only the shapes whose m is this")
    ap.add_argument("--host-max-pairs", type=float, default=1e10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from so_dso_place_recognition_amd import _lib
    from so_dso_place_recognition_amd.matcher import _stream_context
    ctx = _stream_context(0)
    lib = ctx.lib
    p = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda x: x.ctypes.data_as(C.c_void_p)
    lines = []
    for m, n, mask in SHAPES:
        if a.only and m != a.only:
            continue
        loop_diff = 3.0
        gt1, gt2, v, idx = drive(m + n, m, n)
        t1, t2, tv, ti = (torch.from_numpy(x).cuda() for x in (gt1, gt2, v, idx))
        rec = torch.zeros(3, dtype=torch.float64, device="cuda")
        lp = torch.empty((m, 2), dtype=torch.int32, device="cuda"); ld = torch.empty((m, 2), dtype=torch.int32, device="cuda")
        pr = torch.empty(m, dtype=torch.float64, device="cuda"); rc = torch.empty(m, dtype=torch.float64, device="cuda")
        mj = torch.empty(m, dtype=torch.int32, device="cuda"); md = torch.empty(m, dtype=torch.float64, device="cuda")
        ng = torch.empty(1, dtype=torch.int32, device="cuda"); auc = torch.empty(1, dtype=torch.float64, device="cuda")
        calls = {
            "gt": lambda: lib.pr_ground_truth_pairs_dev(ctx.h, p(t1), m, p(t2), n, 3, loop_diff, mask, p(mj), p(md), p(lp), p(ng)),
            "eval": lambda: lib.pr_precision_recall_dev(ctx.h, p(tv), p(ti), 1, m, p(t1), p(t2), n, 3, loop_diff, mask, p(rec), p(lp), p(ld), p(pr), p(rc)),
            "auc_chain": lambda: lib.pr_trapz_dev(ctx.h, p(rc), p(pr), m, p(auc)),
        }
        ms = {}
        for name, fn in calls.items():
            ts = []
            for it in range(a.iters + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.check(fn())
                e1.record()
                e1.synchronize()
                if it >= 2:
                    ts.append(e0.elapsed_time(e1))
            ms[name] = float(np.median(ts))
        cnt = rec[2:].view(torch.int32).cpu().numpy()
        line = dict(bench="eval", m=m, n=n, cols=3, mask_width=mask, loop_diff=loop_diff, iters=a.iters, gt_ms=round(ms["gt"], 4),
                    eval_ms=round(ms["eval"], 4), sweep_ms=round(ms["eval"] - ms["gt"], 4), auc_chain_ms=round(ms["auc_chain"], 4),
                    pairs_per_s=round(m * n / (ms["gt"] * 1e-3), 1), n_gt=int(cnt[0]), n_detected=int(cnt[1]), auc=float(rec[0].item()))
        if float(m) * n <= a.host_max_pairs:
            ha, ht, hn = C.c_double(), C.c_double(), C.c_int32()
            t0 = time.perf_counter()
            r = lib.pr_precision_recall(hp(v), hp(idx), m, hp(gt1), hp(gt2), n, 3, loop_diff, mask, C.byref(ha), C.byref(ht), None, C.byref(hn))
            line["host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            assert r == _lib.PR_OK
            same = (ha.value == line["auc"] or (np.isnan(ha.value) and np.isnan(line["auc"]))) and hn.value == line["n_detected"]
            line["host_equal"] = bool(same)
            line["speedup"] = round(line["host_ms"] / ms["eval"], 1)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
