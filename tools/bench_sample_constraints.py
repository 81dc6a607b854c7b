"""Cost of constrained sampling at the decode benchmark's size (batch 64, E 256, H 512, V 10 000, 20 steps, top_p 0.9), one process:
`DecoderRNN.sample_stochastic` with the defaults (one `sat_sample_decode`) and with suppress_ids=[0, 1, 3], min_length=5,
no_repeat_ngram_size=3, repetition_penalty=1.2 (one `sat_sample_decode_ex`); then the single launch alone on 64 rows of N(0, 2.5^2)
logits: `sat_sample_filtered` against `sat_sample_filtered_ex` under the same rules at step 7, with and without logp / kept.
Median of REGIONS regions of STEPS calls, device-synchronised on both sides; the two variants of a pair alternate region by region.
--defaults-only times the default path alone: with SAT_LIB=<a build of the parent commit> that is the A/B of the unchanged path
(such a build lacks the new symbols).  One JSON object on stdout."""
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
B, E, H, V = 64, 256, 512, 10000
RULES = dict(suppress_ids=[0, 1, 3], min_length=5, end_id=2, no_repeat_ngram_size=3, repetition_penalty=1.2)


def region(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def alternate(fns, warmup, regions, steps):
    """median ms per call of every fn; region i of one fn is followed by region i of the next"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    times = [[] for _ in fns]
    for _ in range(regions):
        for i, fn in enumerate(fns):
            times[i].append(region(fn, steps))
    return [dict(median_ms=round(sorted(t)[len(t) // 2], 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--defaults-only", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(123)
    dec = sat.DecoderRNN(E, H, V, 1).cuda().eval()
    feats = torch.randn(B, E, device="cuda")
    lib, st = L.load(), L.stream()
    res = {"shape": dict(B=B, E=E, H=H, V=V, decode_steps=20, top_p=0.9), "steps": args.steps, "regions": args.regions,
           "device": torch.cuda.get_device_name(0), "library": L.LIB_PATH}

    def plain_decode():
        dec.sample_stochastic(feats, top_p=0.9, seed=7)

    def ruled_decode():
        dec.sample_stochastic(feats, top_p=0.9, seed=7, **RULES)

    if args.defaults_only:
        res["sample_stochastic_defaults"] = alternate([plain_decode], args.warmup, args.regions, args.steps)[0]
        print(json.dumps(res))
        return
    res["sample_stochastic_defaults"], res["sample_stochastic_constrained"] = alternate([plain_decode, ruled_decode], args.warmup,
                                                                                       args.regions, args.steps)
    # the single launch, on logits of a trained model's spread; the prefix holds seven tokens of a small alphabet per row
    logits = (torch.randn(B, V, device="cuda") * 2.5).contiguous()
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    logp = torch.empty(B, device="cuda")
    kept = torch.empty(B, dtype=torch.int32, device="cuda")
    prefix = torch.randint(4, 10, (B, 64), device="cuda")
    cons = sat.models.check_sample_constraints(vocab_size=V, steps=20, **RULES)
    cs = cons.struct("cuda")
    ws = torch.empty(max(lib.sat_sample_filtered_ws_bytes(B, V), 1), dtype=torch.uint8, device="cuda")
    for name, lp, kp in (("", None, None), ("_logprobs", logp.data_ptr(), kept.data_ptr())):
        def one():
            L.check(lib.sat_sample_filtered(logits.data_ptr(), V, B, V, 1.0, 0, 0.9, 7, 7, 0, ids.data_ptr(), 1, lp, kp, ws.data_ptr(),
                                            ws.numel(), st), "sat_sample_filtered")

        def one_ex():
            L.check(lib.sat_sample_filtered_ex(logits.data_ptr(), V, B, V, 1.0, 0, 0.9, 7, 7, 0, ids.data_ptr(), 1, lp, kp, C.byref(cs),
                                               prefix.data_ptr(), 64, ws.data_ptr(), ws.numel(), st), "sat_sample_filtered_ex")
        a, b = alternate([one, one_ex], args.warmup, args.regions, args.steps * 10)
        res["kernel_filtered_64rows_p0.9%s" % name], res["kernel_filtered_ex_64rows_p0.9%s" % name] = a, b
    print(json.dumps(res))


if __name__ == "__main__":
    main()
