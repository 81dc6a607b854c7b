"""Cost of a self-critical step (`TrainStep.scst_step`) next to the teacher-forced `TrainStep.step`, at BASELINE configs[1]'s decoder
shapes (batch 64, E 256, H 512, V 10 000, 20 steps) with cached [B, E] features: HIP-event medians of REGIONS regions of STEPS steps,
each after a warm-up, the two kinds of step interleaved region by region so that clock drift hits both alike.  Also the pieces of
the self-critical step alone (rollout forward, greedy decode, the two CIDEr calls, weights + weighted CE).  One JSON object on
stdout; `--out FILE` also writes it there (profiles/scst_bench.json)."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
D = importlib.import_module("show-and-tell_amd.decoder")
B, E, H, V, T = 64, 256, 512, 10000, 20
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(123)
    model = sat.ShowAndTell(E, H, V, 1, arch=dict(layers=(1, 1, 1, 1), width=8), compute_dtype="bf16").cuda().train()
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    dec = model.decoder
    g = torch.Generator().manual_seed(7)
    feats = torch.randn(B, E, generator=g).cuda()
    caps = torch.randint(4, V, (B, T), generator=g)
    caps[:, 0], caps[:, T - 1] = 1, END
    caps = caps.cuda()
    lengths = [T] * B
    rng = np.random.Generator(np.random.PCG64(5))
    # 1 000 images x 5 references, Zipf-like ids over the vocabulary, 8-16 tokens
    refs = [[[int(t) for t in np.minimum(rng.zipf(1.3, rng.integers(8, 17)) + 3, V - 1)] for _ in range(5)] for _ in range(1000)]
    scorer = sat.CiderScorer(refs)
    index = torch.arange(B, dtype=torch.int32).cuda()
    params = dict(dec.named_parameters())
    sc = sat.SelfCritical(scorer, END)

    def rollout():
        return D.rollout_forward(ts.lib, feats, params, T, 12345, 0)

    ids, logits, _, _ = rollout()
    reward = torch.rand(B, dtype=torch.float64).cuda()

    def weighted_ce():
        w, _, _ = sat.scst_weights(ids, reward, None, END)
        sat.ce_rows_weighted(logits[:, :V], ids, w, write_grad=False)

    cases = {
        "scst_step_ms": lambda: ts.scst_step(feats, index, scorer),
        "teacher_forced_step_ms": lambda: ts.step(feats, caps, lengths),
        "rollout_forward_ms": rollout,
        "greedy_decode_ms": lambda: dec.sample(feats),
        "rewards_ms": lambda: sc.rewards(dec, feats, ids, index),
        "weights_and_weighted_ce_ms": weighted_ce,
    }
    res = {"shape": dict(B=B, E=E, H=H, V=V, steps=T), "decoder_gemm_dtype_of_step": ts.decoder_gemm_dtype,
           "region_steps": args.steps, "regions": args.regions, "warmup": args.warmup, "timer": "HIP events"}
    samples = {k: [] for k in cases}
    for k, fn in cases.items():
        for _ in range(args.warmup):
            fn()
    for _ in range(args.regions):                  # interleaved: every case once per round
        for k, fn in cases.items():
            samples[k].append(region_ms(fn, args.steps))
    ts.check_ids()
    for k, v in samples.items():
        res[k] = sorted(v)[len(v) // 2]
        res[k + "_all"] = v
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
