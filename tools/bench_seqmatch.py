#!/usr/bin/env python3
"""The sequence matcher (pr_seq_select_dev, pr_seqmatch).  Method of DESIGN.md 4.15 / tools/bench_graph.py: wall time from
the call to the end of a stream synchronisation, median (min .. max) over --iters after --warmup warm-ups.  Recorded, not gated.
  batch    pr_seq_select_dev at 4096 x 100 000 and 3475 x 3475 over uniform random fp32 matrices (the selection's cost does not depend on
           the values), L = 8 with six velocities and L = 1 with one, ALTERNATED in the same run with pr_moments_select_f64_dev on the
           same matrices - the single-frame selection it stands beside.  Every record carries the ratio and the byte model:
             hbm_bytes = 2 matrices x 4 B x m n x (R + L - 1) / R x (W + 2 reach) / W   (every slab is formed once per row tile, with its
                         lag rows and its halo) + the outputs
             lds_bytes = 8 B x m n x (sum over v, l of one fp64 read)  with the mean lag count of the first L rows left at L
           against the 6.29 TB/s measured copy rate of HBM and 256 B/clk/CU x 256 CUs x 2.4 GHz = 157 TB/s of ds_read_b64, and names
           the larger share as the bound.
  online   one pr_seqmatch push at capacity 4096 (two channels, L = 8, six velocities, k = 8), eager and as a graph replay
  drive    a generated drive with stops (synth.drive_clouds_torch): AUC / top_recall of the single-frame selection against the sequence
           selection through Matcher.evaluate; recorded, not asserted

    python tools/bench_seqmatch.py [--iters 10] [--warmup 2] [--frames 600] [--skip-large] [--out profiles/seqmatch/bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY = 6.29e12
LDS_PEAK = 256 * 256 * 2.4e9
REACH = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from so_dso_place_recognition_amd import api, synth
    from so_dso_place_recognition_amd.matcher import Matcher, _stream_context
    props = torch.cuda.get_device_properties(0)
    box = dict(host=socket.gethostname(), device=props.name, compute_units=props.multi_processor_count, hbm_gib=round(props.total_memory / 2**30),
               torch=torch.__version__, hip=torch.version.hip)
    lines = []
    st = torch.cuda.Stream()
    R, W = api.seq_tile()

    def emit(**kw):
        lines.append(dict(**kw, iters=a.iters, **box))
        print(json.dumps(lines[-1]), flush=True)

    def once(fn):
        st.synchronize()
        t0 = time.perf_counter()
        fn()
        st.synchronize()
        return time.perf_counter() - t0

    def stats(ts):
        return dict(ms_median=float(np.median(ts)) * 1e3, ms_min=float(min(ts)) * 1e3, ms_max=float(max(ts)) * 1e3)

    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        lib, p = ctx.lib, (lambda t: C.c_void_p(t.data_ptr()))
        # ---- batch
        for m, n in ((3475, 3475),) + (() if a.skip_large else ((4096, 100000),)):
            g = torch.Generator(device="cuda"); g.manual_seed(m + n)
            d_p = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32)
            d_i = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32)
            mom = torch.zeros((m, 2, 3), dtype=torch.float64, device="cuda")
            mom2 = torch.zeros((m, 2, 3), dtype=torch.float64, device="cuda")
            ctx.check(lib.pr_row_moments_dev(ctx.h, p(d_p), p(d_i), m, n, p(mom)))
            for L, vel, k in ((8, [1, -1, 0.75, -0.75, 1.25, -1.25], 1), (8, [1, -1, 0.75, -0.75, 1.25, -1.25], 9), (1, [0], 1), (1, [0], 9)):
                steps = torch.from_numpy(api.seq_steps(L, vel)).cuda()
                V = steps.shape[0]
                out = api.seq_select_torch(d_p, d_i, mom, steps, 0, 0, 100, 2.0, k, ctx=ctx)
                sidx = torch.zeros((m, k), dtype=torch.int32, device="cuda"); ssc = torch.zeros((m, k), dtype=torch.float32, device="cuda")
                ssc64 = torch.zeros((m, k), dtype=torch.float64, device="cuda")
                seq = lambda: api.seq_select_torch(d_p, d_i, mom, steps, 0, 0, 100, 2.0, k, ctx=ctx, out=out)
                single = lambda: ctx.check(lib.pr_moments_select_f64_dev(ctx.h, p(d_p), p(d_i), m, n, p(mom2), 0, 0, 100, 2.0, k, p(sidx), p(ssc), p(ssc64)))
                ts, tm = [], []
                for i in range(a.warmup + a.iters):          # alternated: one of each per round
                    t1, t2 = once(seq), once(single)
                    if i >= a.warmup:
                        ts.append(t1); tm.append(t2)
                hbm = 2 * 4 * m * n * (R + L - 1) / R * (W + 2 * REACH) / W + m * k * 16
                lds = 8.0 * m * n * V * L
                sec = float(np.median(ts))
                emit(bench="seq_select", m=m, n=n, L=L, V=V, k=k, mask_width=100, **stats(ts),
                     single_frame={"call": "pr_moments_select_f64_dev", **stats(tm)}, ratio_to_single_frame=sec / float(np.median(tm)),
                     hbm_bytes=hbm, lds_bytes=lds, hbm_tb_s=hbm / sec / 1e12, hbm_share_of_copy_rate=hbm / sec / HBM_COPY,
                     lds_tb_s=lds / sec / 1e12, lds_share_of_peak=lds / sec / LDS_PEAK,
                     bound="LDS" if lds / LDS_PEAK > hbm / HBM_COPY else "HBM")
            del d_p, d_i, mom, mom2
        # ---- online
        cap, ch, L, k = 4096, 2, 8, 8
        f = api.SequenceFilter(ctx, cap, ch, api.seq_steps(L, [1, -1, 0.75, -0.75, 1.25, -1.25]), k)
        rows = torch.rand((ch, cap), device="cuda", dtype=torch.float64)
        state = torch.tensor([cap, 0, 0, 0], dtype=torch.int32, device="cuda")
        out = f.push_torch(rows, state, (2.0, 1.0), True, 100, k)
        push = lambda: f.push_torch(rows, state, (2.0, 1.0), True, 100, k, out=out)
        for _ in range(L):
            push()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            push()
        for form, fn in (("eager", push), ("graph", graph.replay)):
            ts = [once(fn) for _ in range(a.warmup + a.iters)][a.warmup:]
            emit(bench="seq_push", form=form, capacity=cap, channels=ch, L=L, V=6, k=k, mask_width=100, **stats(ts))
        del graph
        f.close()
        # ---- a drive with stops: single-frame against sequence selection
        N = a.frames
        stops = ((N // 8, 12), (N // 2 + N // 6, 20))
        xyz, it, offs, lap, pos = synth.drive_clouds_torch(N, 3000, 5, stops=stops, positions=True)
        sig = torch.from_numpy(api.sc_generate(xyz, it, offs, ctx=ctx)).cuda()
        gt = torch.from_numpy(np.ascontiguousarray(pos)).cuda()
        mt = Matcher("sc", N, N, ctx=ctx)
        mt.pack_database(sig)
        mask, loop_diff = 50, 3.0
        i0, s0 = mt.match(sig, mask, 2.0, 1)
        e0 = {kk: float(v.cpu().numpy().reshape(-1)[0]) for kk, v in mt.evaluate(i0, s0, gt, gt, loop_diff, mask).items() if kk in ("auc", "top_recall")}
        emit(bench="drive_eval", selection="single_frame", frames=N, lap=int(lap), stops=list(stops), mask_width=mask, loop_diff=loop_diff, **e0)
        for L, vel in ((4, [1, 0.5, 0, 1.5]), (8, [1, 0.75, 0.5, 0, 1.25, 1.5])):
            i1, s1, v1 = mt.match_sequence(sig, api.seq_steps(L, vel), mask, 2.0, 1)
            e1 = {kk: float(v.cpu().numpy().reshape(-1)[0]) for kk, v in mt.evaluate(i1, s1, gt, gt, loop_diff, mask).items() if kk in ("auc", "top_recall")}
            emit(bench="drive_eval", selection="sequence", L=L, velocities=vel, frames=N, lap=int(lap), stops=list(stops), mask_width=mask,
                 loop_diff=loop_diff, **e1)
        mt.close()
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            for l in lines:
                fo.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
