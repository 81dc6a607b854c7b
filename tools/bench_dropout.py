"""Cost of dropout on the cross-entropy step at BASELINE config 2 (batch 64, 224x224 images, E 256, H 512, V 10 000, length-20
captions, bf16 throughput mode), one process: `TrainStep.step` with `decoder.dropout_p` = 0 and = P, strictly sequential steps
(no encoder look-ahead), the two settings ALTERNATING region by region so that both see the same box and clock; then
`sat_dropout_f32` alone, in place on the step's top tape shape [1216, 512].  Median of REGIONS regions of STEPS steps,
device-synchronised on both sides.  One JSON object on stdout (`DESIGN.md` section 3.3g)."""
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
L = sat._lib
B, E, H, V, T = 64, 256, 512, 10000, 20


def region(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--features", action="store_true", help="cached [B, E] features: the decoder-only step")
    args = ap.parse_args()
    torch.manual_seed(123)
    model = sat.ShowAndTell(E, H, V, 1, compute_dtype="bf16").cuda().train()
    ts = sat.TrainStep(model)
    images = torch.randn(B, E, device="cuda") if args.features else torch.randn(B, 3, 224, 224, device="cuda")
    caps = torch.randint(4, V, (B, T), device="cuda")
    caps[:, 0], caps[:, -1] = 1, 2
    lengths = [T] * B
    dec = model.decoder

    def step(p):
        dec.dropout_p = p
        return lambda: ts.step(images, caps, lengths)

    res = {"shape": dict(B=B, E=E, H=H, V=V, T=T, images="features" if args.features else "224x224"),
           "decoder_gemm_dtype": ts.decoder_gemm_dtype, "p": args.p, "steps": args.steps, "regions": args.regions}
    for p in (0.0, args.p):
        for _ in range(args.warmup):
            step(p)()
    t0, t1 = [], []
    for _ in range(args.regions):
        t0.append(region(step(0.0), args.steps))
        t1.append(region(step(args.p), args.steps))
    ts.check_ids()
    res["step_ms_p0"], res["step_ms_p"] = round(median(t0), 4), round(median(t1), 4)
    res["step_ms_p0_all"], res["step_ms_p_all"] = [round(x, 4) for x in t0], [round(x, 4) for x in t1]
    res["delta_us"] = round((median(t1) - median(t0)) * 1e3, 2)

    lib, st = L.load(), L.stream()
    N = B * (T - 1)
    x = torch.randn(N, H, device="cuda")

    def kernel():
        L.check(lib.sat_dropout_f32(x.data_ptr(), H, x.data_ptr(), H, N, H, args.p, 7, 0, 1, st), "sat_dropout_f32")
    for _ in range(args.warmup):
        kernel()
    res["kernel_%dx%d_in_place_us" % (N, H)] = round(median([region(kernel, 200) for _ in range(args.regions)]) * 1e3, 2)
    res["kernel_bytes"] = 2 * N * H * 4
    print(json.dumps(res))


if __name__ == "__main__":
    main()
