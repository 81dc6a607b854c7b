"""Cost of the stochastic decode next to the two deterministic ones, one process, batch 64, E 256, H 512, V 10 000, 20 steps
(`DecoderRNN` on cached features): `sample`, `sample_stochastic` at (temperature, top_k, top_p) = (1, 0, 1), (0.7, 0, 1), (1, 50, 1)
and (1, 0, 0.9), `sample_beam(5)`; then the selection kernels alone on the same logits: `sat_sample_filtered` over 64 rows at those
settings against `sat_beam_step` over the 320 rows of a beam-5 step (beam_row_kernel + the merge).  Median of REGIONS regions of
STEPS calls, device-synchronised on both sides.  One JSON object on stdout."""
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
B, E, H, V, K = 64, 256, 512, 10000, 5
SETTINGS = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 50, 1.0), (1.0, 0, 0.9), (0.7, 50, 0.9)]


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
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(123)
    dec = sat.DecoderRNN(E, H, V, 1).cuda().eval()
    feats = torch.randn(B, E, device="cuda")
    lib, st = L.load(), L.stream()
    res = {"shape": dict(B=B, E=E, H=H, V=V, decode_steps=20, beam=K), "steps": args.steps, "regions": args.regions}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return round(regions(fn, args.regions, args.steps), 4)

    res["sample_ms"] = timed(lambda: dec.sample(feats))
    for tau, k, p in SETTINGS[:4]:
        res["sample_stochastic_t%g_k%d_p%g_ms" % (tau, k, p)] = timed(
            lambda: dec.sample_stochastic(feats, temperature=tau, top_k=k, top_p=p, seed=7))
    res["sample_stochastic_t1_k0_p0.9_logprobs_ms"] = timed(
        lambda: dec.sample_stochastic(feats, top_p=0.9, seed=7, return_logprobs=True))
    res["sample_beam5_ms"] = timed(lambda: dec.sample_beam(feats, K))

    # the selection kernels alone, on logits of a trained model's spread (N(0, 2.5^2))
    logits = (torch.randn(B * K, V, device="cuda") * 2.5).contiguous()
    ids = torch.empty(B * K, dtype=torch.int64, device="cuda")
    logp = torch.empty(B, device="cuda")
    kept = torch.empty(B, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(lib.sat_sample_filtered_ws_bytes(B, V), 1), dtype=torch.uint8, device="cuda")
    for tau, k, p in SETTINGS:
        for name, lp, kp in (("", None, None), ("_logprobs", logp.data_ptr(), kept.data_ptr())):
            def one():
                L.check(lib.sat_sample_filtered(logits.data_ptr(), V, B, V, tau, k, p, 7, 3, 0, ids.data_ptr(), 1, lp, kp, ws.data_ptr(),
                                                ws.numel(), st), "sat_sample_filtered")
            res["kernel_filtered_64rows_t%g_k%d_p%g%s_us" % (tau, k, p, name)] = round(timed(one) * 1e3, 2)
    scores = torch.zeros(B, K, device="cuda")
    scores2 = torch.empty(B, K, device="cuda")
    parent = torch.empty(B * K, dtype=torch.int32, device="cuda")
    bws = torch.empty(lib.sat_beam_step_ws_bytes(B, K), dtype=torch.uint8, device="cuda")

    def beam():
        L.check(lib.sat_beam_step(logits.data_ptr(), V, scores.data_ptr(), None, -1, B, K, V, parent.data_ptr(), ids.data_ptr(),
                                  scores2.data_ptr(), bws.data_ptr(), bws.numel(), st), "sat_beam_step")
    res["kernel_beam_step_320rows_us"] = round(timed(beam) * 1e3, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
