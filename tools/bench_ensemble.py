"""Cost of the ensemble decode next to the single-model beam decode, one process, batch 64, beam 5, E 256, H 512, V 10 000, 20 steps,
end_id 2, on cached features: `DecoderRNN.sample_beam` (sat_beam_decode) of one model, then the ensemble loop
(sat_beam_decode_ensemble) for M = 1, 2, 4 members of that shape in both modes, then the single model again.  Then the combine
kernel alone (sat_ensemble_logprobs) on R = 320 rows: microseconds per call and achieved bytes per second, counting every input
matrix read once and the output written once ((M + 1) * R * V * 4 bytes).
Median of REGIONS regions of STEPS calls, device-synchronised on both sides.  One JSON object on stdout.
With SAT_LIB naming a build without the ensemble entry points (the parent commit's library) only the single-model figure is
measured: that times M is the yardstick of the loop."""
import argparse
import ctypes as C
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
B, K, E, H, V, T, END = 64, 5, 256, 512, 10000, 20, 2
MS = (1, 2, 4)


def regions(fn, n_regions, steps):
    out = []
    for _ in range(n_regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(123)
    decs = []
    for _ in range(max(MS)):
        dec = sat.DecoderRNN(E, H, V, 1).cuda().eval()
        with torch.no_grad():                 # a sharper output layer and an <end> that occurs
            dec.linear.weight.mul_(8.0)
            dec.linear.bias[END] += 1.0
        decs.append(dec)
    feats = [torch.randn(B, E, device="cuda") for _ in decs]
    lib, st = L.load(), L.stream()
    have = hasattr(lib, "sat_beam_decode_ensemble")
    res = {"shape": dict(B=B, K=K, E=E, H=H, V=V, decode_steps=T), "steps": args.steps, "regions": args.regions,
           "library": os.path.basename(L.LIB_PATH), "ensemble_entry_points": have}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return round(regions(fn, args.regions, args.steps), 4)

    res["single_beam_decode_ms"] = timed(lambda: decs[0].sample_beam(feats[0], K, END))
    if have:
        from importlib import import_module
        cons = import_module("show-and-tell_amd.models").check_beam_constraints()
        for mode in ("prob", "logprob"):
            for M in MS:
                ens = sat.Ensemble(decs[:M], None, mode)
                res["ensemble_M%d_%s_ms" % (M, mode)] = timed(lambda: ens._decoder_beam(feats[:M], K, END, T, cons, 1, 0.0))
        res["single_beam_decode_again_ms"] = timed(lambda: decs[0].sample_beam(feats[0], K, END))
        # the combine alone, on logits of a trained model's spread (N(0, 2.5^2))
        R = B * K
        logits = [(torch.randn(R, V, device="cuda") * 2.5).contiguous() for _ in range(max(MS))]
        out = torch.empty(R, V, device="cuda")
        for mode in (0, 1):
            for M in MS:
                ptrs = (C.c_void_p * M)(*[t.data_ptr() for t in logits[:M]])

                def combine():
                    L.check(lib.sat_ensemble_logprobs(ptrs, M, V, None, mode, R, V, out.data_ptr(), V, st), "sat_ensemble_logprobs")
                us = timed(combine) * 1e3
                res["kernel_combine_M%d_mode%d_us" % (M, mode)] = round(us, 2)
                res["kernel_combine_M%d_mode%d_GBps" % (M, mode)] = round((M + 1) * R * V * 4 / (us * 1e-6) / 1e9, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
