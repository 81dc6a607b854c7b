"""Cost of scheduled sampling at BASELINE configs[1] (batch 64, 224x224 images, length-20 captions, ResNet-152, E 256, H 512,
V 10 000, bf16 throughput mode): TrainStep with ss_prob 0 and 0.25, timed as bench.py times the headline (median of REGIONS regions
of STEPS steps, device-synchronised on both sides, encoder look-ahead on), the same with cached features (decoder-only steps), and
the decoder forward alone (teacher-forced vs the 19-step sampling loop).  One JSON object on stdout.
`--forward-only N`: just N sampling forwards (for `rocprofv3 --kernel-trace --stats`)."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
D = importlib.import_module("show-and-tell_amd.decoder")
B, E, H, V, T, S = 64, 256, 512, 10000, 20, 224


def synth(seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, S, S, generator=g)
    caps = torch.randint(4, V, (B, T), generator=g)
    caps[:, 0], caps[:, T - 1] = 1, 2
    return images.cuda(), caps.cuda()


def regions(fn, n_regions, steps):
    out = []
    for _ in range(n_regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return sorted(out)[len(out) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ss-prob", type=float, default=0.25)
    ap.add_argument("--forward-only", type=int, default=0)
    args = ap.parse_args()
    torch.manual_seed(123)
    model = sat.ShowAndTell(E, H, V, 1, compute_dtype="bf16").cuda().train()
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    dec, lib = model.decoder, ts.lib
    images, caps = synth(123)
    lengths = [T] * B
    feats = torch.randn(B, E, device="cuda")
    params = dict(dec.named_parameters())
    pi = sat.PackInfo.get([T - 1] * B, "cuda")

    def ss_forward(n):
        for _ in range(n):
            D.decoder_forward(lib, feats, params, caps[:, :-1], pi, ss=(args.ss_prob, 12345, 0), store_logits=False)

    if args.forward_only:
        ss_forward(args.forward_only)
        torch.cuda.synchronize()
        print(json.dumps({"forward_only": args.forward_only}))
        return

    def tf_forward(n):
        for _ in range(n):
            D.decoder_forward(lib, feats, params, caps[:, :-1], pi)

    res = {"shape": dict(B=B, E=E, H=H, V=V, cap_len=T, image=S), "ss_prob": args.ss_prob, "steps": args.steps,
           "regions": args.regions}
    for name, fn in (("forward_teacher_forced_f32_ms", tf_forward), ("forward_ss_loop_ms", ss_forward)):
        fn(args.warmup)
        res[name], res[name + "_all"] = regions(fn, args.regions, args.steps)

    batches = [images] + [synth(977 * (k + 1))[0] for k in range(model.encoder.lookahead_depth)]
    nb = len(batches)
    depth = model.encoder.lookahead_depth
    model.encoder.build_lookahead(images)
    for p in (0.0, args.ss_prob):
        dec.ss_prob = p

        def full(n):
            for i in range(n):
                nxt = [batches[j % nb] for j in range(i + 1, i + 1 + depth) if j < n]
                ts.step(batches[i % nb], caps, lengths, next_images=nxt or None)

        def cached(n):
            for _ in range(n):
                ts.step(feats, caps, lengths)

        for name, fn in (("train_step_ms", full), ("decoder_only_step_ms", cached)):
            fn(args.warmup)
            key = "%s_ss%g" % (name, p)
            res[key], res[key + "_all"] = regions(fn, args.regions, args.steps)
    ts.check_ids()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
