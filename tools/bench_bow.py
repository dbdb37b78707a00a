"""BoW generation throughput (pr_bow_generate_dev through api.bow_generate_torch) against a synthetic k = 10, L = 6 vocabulary (1 111 111
nodes, 10^6 words, built from arrays by synth.bow_vocabulary).  One JSON line per (lanes, N): images of `--feats` uniformly random ORB
descriptors already on the GPU, cols = 4000, images/s from HIP events around `--reps` calls after `--warmup` calls.  --lanes lists the
lanes per descriptor of the descent (PR_BOW_LANES; the library's default is 4).  `tb_per_s` counts the 320 B of sibling descriptors
every level of every descent reads (6 levels)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4096")
    ap.add_argument("--feats", type=int, default=4000)
    ap.add_argument("--lanes", default="4")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from so_dso_place_recognition_amd import api, synth
    voc = api.ORBVocabulary.from_arrays(10, 6, 0, 0, *synth.bow_vocabulary(0, k=10, L=6))
    g = torch.Generator(device="cuda").manual_seed(0)
    sizes = [int(s) for s in a.sizes.split(",")]
    desc = torch.randint(0, 256, (max(sizes) * a.feats, 32), dtype=torch.uint8, device="cuda", generator=g)
    for lanes in (int(x) for x in a.lanes.split(",")):
        os.environ["PR_BOW_LANES"] = str(lanes)
        ctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)    # reads PR_BOW_LANES at its first BoW call
        for n in sizes:
            d = desc[:n * a.feats]
            offs = torch.arange(0, n + 1, device="cuda", dtype=torch.int64) * a.feats
            out = torch.empty((2 * n, 4000), dtype=torch.float64, device="cuda")
            nw = torch.empty(n, dtype=torch.int32, device="cuda")
            for _ in range(a.warmup):
                api.bow_generate_torch(d, offs, voc, cols=4000, ctx=ctx, out=out, n_words=nw)
            torch.cuda.synchronize()
            reps = a.reps if n > 64 else 20 * a.reps
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                api.bow_generate_torch(d, offs, voc, cols=4000, ctx=ctx, out=out, n_words=nw)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / reps
            print(json.dumps({"bench": "bow_generate", "lanes": lanes, "N": n, "feats": a.feats, "ms_per_call": round(ms, 4),
                              "images_per_s": round(n / (ms * 1e-3), 1), "tb_per_s": round(n * a.feats * 6 * 320 / (ms * 1e-3) / 1e12, 3),
                              "max_words": int(nw.max().item()), "truncated": bool(ctx.take_warnings() & 32)}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
