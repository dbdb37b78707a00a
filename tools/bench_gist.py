"""GIST generation throughput (pr_gist_generate_dev through api.gist_generate_torch): one JSON line per batch size N in {1, 64, 4096}
of 256 x 256 u8 images already on the GPU.  images/s from HIP events around `--reps` calls after `--warmup` calls; `frac_157tf` is
the rate of the nominal 5 n log2 n flop count of the 33 256 x 256 complex transforms per image (one forward, 32 inverse) against
the 157 TF fp32 vector figure (the prefilter's GEMMs are not counted)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOP_PER_IMAGE = 33 * 5 * 65536 * math.log2(65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,4096")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    from so_dso_place_recognition_amd import api
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (int(s) for s in a.sizes.split(",")):
        img = torch.randint(0, 256, (n, 256, 256), dtype=torch.uint8, device="cuda", generator=g)
        out = torch.empty((n, 512), dtype=torch.float32, device="cuda")
        for _ in range(a.warmup):
            api.gist_generate_torch(img, out=out)
        torch.cuda.synchronize()
        reps = a.reps if n > 64 else 10 * a.reps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            api.gist_generate_torch(img, out=out)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        rate = n / (ms * 1e-3)
        print(json.dumps({"bench": "gist_generate", "N": n, "ms_per_call": round(ms, 4), "images_per_s": round(rate, 1),
                          "frac_157tf": round(rate * FLOP_PER_IMAGE / 157e12, 4), "finite": bool(torch.isfinite(out).all().item())}),
              flush=True)


if __name__ == "__main__":
    main()
