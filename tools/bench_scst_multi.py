"""Cost of a self-critical step (`TrainStep.scst_step`) with S sampled captions per image, at BASELINE configs[1] (batch 64 of
224 x 224 images through the bf16 ResNet-152 stack, E 256, H 512, V 10 000, one LSTM layer, 20 steps, no encoder look-ahead): HIP-
event medians of REGIONS regions of STEPS steps, each case after its own warm-up, the cases interleaved region by region so that
clock drift hits all alike.  A case is S:baseline ("1:greedy", "5:greedy", "5:sample_mean"); "1:greedy" makes the call without the
keywords, so `--root DIR` can time another checkout of the package (one that does not know them) with the same script.  One JSON
object on stdout; `--out FILE` also writes it there (profiles/scst_multi_bench.txt collects the runs)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

B, E, H, V, T, IMAGE = 64, 256, 512, 10000, 20, 224
END = 2


def region_ms(fn, steps):
    """one region: `steps` calls between two HIP events on the current stream, per-call milliseconds"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--cases", default="1:greedy,5:greedy,5:sample_mean")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cached", action="store_true", help="precomputed [B, E] features instead of images: the decoder's share")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    sat = importlib.import_module("show-and-tell_amd")
    torch.manual_seed(123)
    arch = dict(arch=dict(layers=(1, 1, 1, 1), width=8)) if args.cached else {}
    model = sat.ShowAndTell(E, H, V, 1, compute_dtype="bf16", **arch).cuda().train()
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    g = torch.Generator().manual_seed(7)
    inputs = (torch.randn(B, E, generator=g) if args.cached else torch.randn(B, 3, IMAGE, IMAGE, generator=g)).cuda()
    rng = np.random.Generator(np.random.PCG64(5))
    # 1 000 images x 5 references, Zipf-like ids over the vocabulary, 8-16 tokens (tools/bench_scst.py's corpus)
    refs = [[[int(t) for t in np.minimum(rng.zipf(1.3, rng.integers(8, 17)) + 3, V - 1)] for _ in range(5)] for _ in range(1000)]
    scorer = sat.CiderScorer(refs)
    index = torch.arange(B, dtype=torch.int32).cuda()

    def case(spec):
        S, baseline = spec.split(":")
        kw = {} if (int(S), baseline) == (1, "greedy") else dict(num_samples=int(S), baseline=baseline)
        return lambda: ts.scst_step(inputs, index, scorer, **kw)

    cases = {spec: case(spec) for spec in args.cases.split(",")}
    res = {"root": os.path.abspath(args.root), "inputs": "cached features" if args.cached else "images",
           "shape": dict(B=B, E=E, H=H, V=V, steps=T, image=IMAGE), "region_steps": args.steps, "regions": args.regions,
           "warmup": args.warmup, "timer": "HIP events"}
    samples = {k: [] for k in cases}
    for _ in range(args.regions):                  # interleaved: every case once per round (its buffers re-warmed: one set is kept)
        for k, fn in cases.items():
            for _ in range(args.warmup):
                fn()
            samples[k].append(region_ms(fn, args.steps))
    ts.check_ids()
    for k, v in samples.items():
        res[k + "_ms"] = sorted(v)[len(v) // 2]
        res[k + "_ms_all"] = [round(x, 4) for x in v]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
