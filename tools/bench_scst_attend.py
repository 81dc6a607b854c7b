#!/usr/bin/env python3
"""Cost of one self-critical step of the Show-Attend-Tell model (`scst_forward` + `backward`) next to one teacher-forced step
(`forward` + cross entropy + `backward`) of the same model, at the config defaults: batch 64, 224 x 224 images through the frozen bf16
VGG16 stack (P 196, C 512), E 512, H 1024, V 10 000, 20 steps.  HIP-event medians of REGIONS regions of STEPS steps after a warm-up,
the kinds of step interleaved region by region so that clock drift hits all alike.  Also the pieces on cached features: the conv
stack, the sampled rollout, the arg-max rollout, and the teacher-forced decoder forward.  No optimizer step in any of them.
    python tools/bench_scst_attend.py [--steps 10] [--regions 7] [--warmup 5] [--out profiles/scst_attend_bench.txt]"""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sat = importlib.import_module("show-and-tell_amd")
B, T, V, END = 64, 20, 10000, 2


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(123)
    model = sat.ShowAttendTellModel(1024, 512, V, 512, None, compute_dtype="bf16").cuda().train()
    images = torch.randn(B, 3, 224, 224, device="cuda")
    caps = torch.randint(4, V, (B, T + 1), device="cuda")
    caps[:, 0], caps[:, -1] = 1, END
    targets, l1 = sat.pack_targets(caps, [T + 1] * B)          # 20 decoder steps, as the rollout's
    rng = np.random.Generator(np.random.PCG64(5))
    # 1 000 images x 5 references, Zipf-like ids over the vocabulary, 8-16 tokens
    refs = [[[int(t) for t in np.minimum(rng.zipf(1.3, rng.integers(8, 17)) + 3, V - 1)] for _ in range(5)] for _ in range(1000)]
    scorer = sat.CiderScorer(refs)
    index = torch.arange(B, dtype=torch.int32).cuda()
    crit = torch.nn.CrossEntropyLoss()
    with torch.no_grad():
        feats, fmean = model._encode(images)

    def scst_step():
        model.zero_grad()
        model.scst_forward(images, index, scorer, end_id=END, steps=T).backward()

    def teacher_forced_step():
        model.zero_grad()
        crit(model(images, caps[:, :-1], l1), targets).backward()

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    cases = {
        "scst_forward + backward": scst_step,
        "teacher-forced forward + CE + backward": teacher_forced_step,
        "conv stack (frozen, bf16)": no_grad(lambda: model._encode(images)),
        "sampled rollout, forward only": no_grad(lambda: model.rollout(feats, fmean, T)),
        "arg-max rollout": lambda: model.rollout(feats, fmean, T, greedy=True),
        "teacher-forced decoder forward": no_grad(lambda: model.decode(feats, fmean, caps[:, :-1], l1)),
    }
    samples = {k: [] for k in cases}
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    for _ in range(args.regions):                  # interleaved: every case once per round
        for k, fn in cases.items():
            samples[k].append(region_ms(fn, args.steps))
    med = {k: statistics.median(v) for k, v in samples.items()}
    lines = ["Show-Attend-Tell, batch %d, 224 x 224 (P 196, C 512), E 512, H 1024, V %d, %d steps, bf16 conv stack frozen, f32 decoder"
             % (B, V, T),
             "HIP events, %d warm-up calls, medians of %d interleaved regions of %d calls each; ms per call (min .. max of the regions)"
             % (args.warmup, args.regions, args.steps)]
    for k, v in samples.items():
        lines.append("  %-40s %8.3f  (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
    a, b = med["scst_forward + backward"], med["teacher-forced forward + CE + backward"]
    lines.append("ratio self-critical / teacher-forced: %.2f (+%.3f ms)" % (a / b, a - b))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
