"""Cost of global-norm clipping and AdamW weight decay in the optimizer step, alone, at the flat sizes of BASELINE configs[1]
(Show-and-Tell: embed 256, hidden 512, vocab 10000) and of the Show-Attend-Tell drop-in model (1024, 512, 10000, 512), one process:

  off          sat_clamp_adam_step_guarded -- the call `TrainStep.optimizer_step` makes with max_grad_norm and weight_decay off
  norm         sat_grad_sumsq + sat_adamw_step with max_norm = +inf: the norm is measured, the coefficient is 1
  norm_scales  the same with a max_norm below the norm: every gradient is multiplied by the coefficient
  norm_decay   norm_scales + weight_decay 0.01 with six exempt ranges (the 1-D parameters)
  decay        sat_adamw_step alone, weight_decay 0.01, no norm pass
  ema          `off` + sat_ema_update behind it (decay 0.999, the same fault word): what `optimizer_step` launches with ema_decay set
  parent_off   (--parent-lib) sat_clamp_adam_step_guarded of ANOTHER build of the library, the parent commit's: `off` makes the
               same call into the same code, so the two must lie inside each other's spread

All with clip 0.1 and the fault word (zero) as in the trainer.  The sides ALTERNATE region by region (REGIONS regions of STEPS steps
each); a region is timed with HIP events around its launches, the median region and the lowest and highest are reported per side in
microseconds per step, with the bytes a step must move (28 B / parameter, + 4 B for the norm pass, + 12 B for the average) over
the median.  The kernels run
on their own output again and again: a fixed Adam step count, values stay finite, the work does not depend on them (in `norm_scales`
the written-back gradient settles at norm = max_norm, where the coefficient max_norm / (max_norm + 1e-6) still is not 1).
One JSON object on stdout."""
import argparse
import ctypes
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
HP = (1e-3, 0.9, 0.999, 1e-8, 0.1, 10)          # lr, beta1, beta2, eps, clip, step


def flat_sizes():
    """{name: (n, exempt ranges)} of the two models' flat buffers, from the modules built on the CPU (nothing is run)"""
    optim = importlib.import_module("show-and-tell_amd.optim")
    out = {}
    for name, model in (("show_and_tell_cfg1", sat.ShowAndTell(256, 512, 10000, 1, compute_dtype="bf16")),
                        ("show_attend_tell", sat.ShowAttendTellModel(1024, 512, 10000, 512, None, compute_dtype="bf16"))):
        off, ranges = 0, []
        for p in model.parameters():
            if p.requires_grad:
                if p.dim() <= 1:
                    ranges.append((off, off + p.numel()))
                off += L.pad4(p.numel())
        out[name] = (off, optim.merge_ranges(ranges))
    return out


def alternate(fns, n_regions, steps, warmup):
    """{name: us per step: median, lowest, highest region}: the sides take turns, one event-timed region each"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libsat_hip.so of the parent commit (same ABI version)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is measured on a CPU"
    lib, st = L.load(), L.stream()
    parent = L.open_library(args.parent_lib) if args.parent_lib else None
    res = {"steps": args.steps, "regions": args.regions, "clip": HP[4], "sizes": {}}
    for name, (n, ranges) in flat_sizes().items():
        g = torch.Generator().manual_seed(5)

        def state():
            return [t.cuda() for t in (torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.01,
                                       torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4)]

        skip = torch.zeros(1, device="cuda")
        P = lib.sat_grad_sumsq_partials(n)
        partials = torch.empty(2 * P, dtype=torch.float64, device="cuda")
        norm_out = torch.zeros(2, dtype=torch.float64, device="cuda")
        ex = (ctypes.c_int64 * (2 * len(ranges)))(*[x for r in ranges for x in r])

        def guarded(which, bufs):
            ptrs = [t.data_ptr() for t in bufs]
            return lambda: L.check(which.sat_clamp_adam_step_guarded(*ptrs, n, *HP, skip.data_ptr(), st))

        def adamw(bufs, max_norm, wd):
            ptrs = [t.data_ptr() for t in bufs]
            norm = max_norm is not None

            def fn():
                if norm:
                    L.check(lib.sat_grad_sumsq(ptrs[1], n, HP[4], partials.data_ptr(), 0, P, st))
                L.check(lib.sat_adamw_step(*ptrs, n, *HP, wd, ex if wd > 0 else None, len(ranges) if wd > 0 else 0,
                                           max_norm if norm else 0.0, partials.data_ptr() if norm else None, P if norm else 0,
                                           norm_out.data_ptr() if norm else None, skip.data_ptr(), st))
            return fn

        def with_ema(bufs):
            update, avg = guarded(lib, bufs), bufs[0].clone()
            ptrs = (avg.data_ptr(), bufs[0].data_ptr())

            def fn():
                update()
                L.check(lib.sat_ema_update(*ptrs, n, 0.999, skip.data_ptr(), None, st))
            return fn

        fns = {"off": guarded(lib, state()), "ema": with_ema(state()), "norm": adamw(state(), float("inf"), 0.0), "norm_scales": adamw(state(), 1.0, 0.0),
               "norm_decay": adamw(state(), 1.0, 0.01), "decay": adamw(state(), None, 0.01)}
        if parent is not None:
            fns["parent_off"] = guarded(parent, state())
        r = alternate(fns, args.regions, args.steps, args.warmup)
        torch.cuda.synchronize()
        assert norm_out[1].item() == 0.0, "a benchmark buffer went non-finite"
        for k, v in r.items():
            nbytes = n * (28 + (4 if k.startswith("norm") else 0) + (12 if k == "ema" else 0))
            v["bytes_per_step"] = nbytes
            v["TB_per_s_at_median"] = round(nbytes / (v["median_us"] * 1e-6) / 1e12, 3)
        res["sizes"][name] = {"n": n, "exempt_ranges": len(ranges), "partial_pairs": P, "settings": r}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
