"""Cost of gradient accumulation, one process.

A. The launch alone, at the flat size of BASELINE configs[1] (Show-and-Tell: embed 256, hidden 512, vocab 10000):
  accumulate        sat_grad_accumulate, a later fold: read acc and g, write acc (12 B / parameter)
  accumulate_first  the first fold: read g, write acc (8 B / parameter)
  ema               sat_ema_update over the same n: the same 12 B / parameter, the streaming rate to compare with
B. The step, decoder-only (cached [B, 256] features, so that no BatchNorm lies in the path and the three sides train on the same
   64 captions per update or pair of updates), bf16 decoder mode:
  accumulated_2x32  `TrainStep.step_accumulated` over two micro-batches of 32: two backwards, two folds, one update
  two_steps_32      two plain `step`s of 32: two backwards, two updates
  one_step_64       one plain `step` of 64: one backward, one update (`step` is the parent commit's code)

The sides ALTERNATE region by region (a region of A holds 16 x --steps launches, one of B --steps calls); a region is timed with
HIP events around its launches, the median region and the lowest and highest are reported per side in microseconds per call.  The
launches of A run on the same 117 MB again and again: less than the chip's last-level cache, so their rate is that of a buffer
the step in front has just touched, not of cold HBM.  One JSON object on stdout."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
E, H, V, T = 256, 512, 10000, 20


def alternate(fns, n_regions, steps, warmup):
    """{name: us per call: median, lowest, highest region}: the sides take turns, one event-timed region each"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(n_regions):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            t1.synchronize()
            out[k].append(t0.elapsed_time(t1) * 1e3 / steps)
    return {k: dict(median_us=round(sorted(v)[len(v) // 2], 2), lowest_us=round(min(v), 2), highest_us=round(max(v), 2))
            for k, v in out.items()}


def engine():
    torch.manual_seed(3)
    return sat.TrainStep(sat.ShowAndTell(E, H, V, 1, compute_dtype="bf16").cuda().train())


def batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = sorted(torch.randint(8, T + 1, (B,), generator=g).tolist(), reverse=True)
    caps = torch.randint(4, V, (B, T), generator=g)
    caps[:, 0] = 1
    return torch.randn(B, E, generator=g).cuda(), caps.cuda(), lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is measured on a CPU"
    lib, st = L.load(), L.stream()
    res = {"steps": args.steps, "regions": args.regions}

    # ---- A. the launch alone ----
    probe = engine()
    n = probe.flat.n
    del probe
    g = torch.Generator().manual_seed(5)
    acc, grads, acc1, ema, params = [(torch.randn(n + 4, generator=g) * 0.01).cuda() for _ in range(5)]
    for t in (acc, grads, acc1):
        t[n + 1:] = 0.0
    fns = {"accumulate": lambda: L.check(lib.sat_grad_accumulate(acc.data_ptr(), grads.data_ptr(), n, 1.0, 0, st)),
           "accumulate_first": lambda: L.check(lib.sat_grad_accumulate(acc1.data_ptr(), grads.data_ptr(), n, 1.0, 1, st)),
           "ema": lambda: L.check(lib.sat_ema_update(ema.data_ptr(), params.data_ptr(), n, 0.999, None, None, st))}
    r = alternate(fns, args.regions, args.steps * 16, args.warmup)
    torch.cuda.synchronize()
    assert torch.isfinite(acc).all(), "a benchmark buffer went non-finite"
    for k, v in r.items():
        v["bytes_per_call"] = n * (8 if k == "accumulate_first" else 12)
        v["TB_per_s_at_median"] = round(v["bytes_per_call"] / (v["median_us"] * 1e-6) / 1e12, 3)
    res["launch"] = {"n": n, "sides": r}

    # ---- B. the step ----
    big = batch(64, 11)
    halves = [sat.dp_shard(*big, r_, 2)[:3] for r_ in range(2)]
    a, b, c = engine(), engine(), engine()

    def two_steps():
        b.step(*halves[0])
        b.step(*halves[1])
    fns = {"accumulated_2x32": lambda: a.step_accumulated(halves), "two_steps_32": two_steps, "one_step_64": lambda: c.step(*big)}
    r = alternate(fns, args.regions, args.steps, args.warmup)
    torch.cuda.synchronize()
    for ts in (a, b, c):
        ts.check_ids()
        assert torch.isfinite(ts.flat.params).all()
    res["step"] = {"E": E, "H": H, "V": V, "tokens_per_update": sum(l - 1 for l in big[2]), "decoder_gemm_dtype": a.decoder_gemm_dtype,
                   "sides": r}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
