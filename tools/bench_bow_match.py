"""The inverted-file BoW matcher (matcher.BowMatcher / pr_bow_*) on one MI355X: index build, queries/s at m = 4096 (k = 1, 5), m = 1 latency,
the online step (match one keyframe + append it at n = 100k, the BoW counterpart of bench.py's extra.sc_online_loop), per word distribution
(uniform, Zipf); then pr_match_topk_cols (the fp32 all-pairs path) next to the new path on tools/bench_plain.py's BoW case.
The DB is drawn on the GPU (synth.bow_signatures_torch).  Prints one JSON line per measurement.
  python tools/bench_bow_match.py [--n 100000] [--words 1000] [--vocab 1000000] [--quick]
Environment knobs read at matcher creation (recorded in the output): PR_BOW_THREADS (64 | 256), PR_BOW_CHUNK, PR_BOW_TAIL_ROWS."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so_dso_place_recognition_amd import api, synth  # noqa: E402
from so_dso_place_recognition_amd.matcher import BowMatcher  # noqa: E402


def emit(**kw):
    kw.update(threads=os.environ.get("PR_BOW_THREADS", "256"), chunk=os.environ.get("PR_BOW_CHUNK", "default"))
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    """median ms of reps calls (events on the current stream, synchronised)"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def run_dist(name, zipf, n, words, vocab, m, reps, online_steps):
    cols = words + 1
    t0 = time.perf_counter()
    # queries from the same draw (one rank -> id permutation: a Zipf query shares the DB's near-stop words)
    db = synth.bow_signatures_torch(21, n + online_steps + m, cols=cols, vocab=vocab, fill=(words, words), zipf=zipf)
    q = db[2 * (n + online_steps):].contiguous()
    db = db[:2 * (n + online_steps)]
    torch.cuda.synchronize()
    draw_s = time.perf_counter() - t0
    posts = int((db[0::2, :cols - 1] > -1).sum().item())
    mt = BowMatcher(m, n + online_steps, cols, vocab, max_postings=posts)
    base = db[:2 * n]
    mt.pack_database(base)                                   # warm-up
    build_ms = timed(lambda: mt.pack_database(base), reps)
    emit(case=name, what="build", n=n, words_per_image=words, vocab=vocab, postings=posts, ms=build_ms, draw_s=round(draw_s, 2))
    for k in (1, 5):
        mt.match(q, k=k)
        ms = timed(lambda: mt.match(q, k=k), reps)
        emit(case=name, what="match", n=n, m=m, k=k, ms=ms, queries_per_s=m / ms * 1e3)
    q1 = q[:2].contiguous()
    mt.match(q1, k=5)
    emit(case=name, what="latency m=1", n=n, k=5, ms=timed(lambda: mt.match(q1, k=5), max(reps, 20)))
    # online: match keyframe t against rows [0, t) with a mask, then append it (the tail; one fold every PR_BOW_TAIL_ROWS steps)
    steps = []
    for t in range(n, n + online_steps):
        row = db[2 * t:2 * t + 2]
        torch.cuda.synchronize()
        s = time.perf_counter()
        idx, sc = mt.match(row, mask_width=50, k=1, q_row0=t)
        mt.append_database(row)
        torch.cuda.synchronize()
        steps.append((time.perf_counter() - s) * 1e3)
    emit(case=name, what="online step (match 1 + append 1)", n=n, steps=online_steps, ms_median=float(np.median(steps)),
         ms_max=float(np.max(steps)), tail_rows=os.environ.get("PR_BOW_TAIL_ROWS", "1024"))
    mt.close()


def run_plain(reps):
    """tools/bench_plain.py's BoW case: 256 x 5000 images, 4000 columns, 150-400 words, vocabulary 20 000 (host rows, host results)."""
    h1 = synth.bow_signatures(3, 256, 4000, 20000, (150, 400))
    h2 = synth.bow_signatures(4, 5000, 4000, 20000, (150, 400))
    ctx = api.Context(0)
    for label, fn in (("pr_match_topk_cols (fp32 all-pairs, host)", lambda: api.match_topk("bow", h1, h2, 0, k=1, ctx=ctx)),
                      ("pr_bow_match_topk_f64 (inverted file, host)", lambda: api.bow_match_topk(h1, h2, 0, 1, ctx=ctx))):
        fn()
        ts = []
        for _ in range(reps):
            s = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - s) * 1e3)
        emit(case="bench_plain bow 256 x 5000 x 4000", what=label, wall_ms=float(np.median(ts)))
    i0, _ = api.match_topk("bow", h1, h2, 0, k=1, ctx=ctx)
    i1, _ = api.bow_match_topk(h1, h2, 0, 1, ctx=ctx)
    emit(case="bench_plain bow 256 x 5000 x 4000", what="top-1 agreement fp32 vs fp64", agree=float((i0 == i1).mean()))
    mt = BowMatcher(256, 5000, 4000, 20000, ctx=None)
    d2, d1 = torch.from_numpy(h2).cuda(), torch.from_numpy(h1).cuda()
    mt.pack_database(d2)
    mt.match(d1, k=1)
    emit(case="bench_plain bow 256 x 5000 x 4000", what="BowMatcher.match (device rows, resident index)", ms=timed(lambda: mt.match(d1, k=1), reps))
    mt.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--online", type=int, default=64)
    ap.add_argument("--zipf", type=float, default=0.9)
    ap.add_argument("--cases", default="uniform,zipf,plain")
    a = ap.parse_args()
    cases = a.cases.split(",")
    if "uniform" in cases:
        run_dist("uniform", None, a.n, a.words, a.vocab, a.m, a.reps, a.online)
    if "zipf" in cases:
        run_dist(f"zipf s={a.zipf}", a.zipf, a.n, a.words, a.vocab, a.m, a.reps, a.online)
    if "plain" in cases:
        run_plain(a.reps)


if __name__ == "__main__":
    main()
