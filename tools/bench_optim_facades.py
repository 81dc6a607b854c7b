"""Host cost of the two optimizer facades: the wall time `TrainStep.optimizer_step()` and `FusedClampAdam.step()` take to ISSUE their
launches (tools/bench_optim.py times the kernels through the C ABI and never enters the classes).  Small buffers on purpose -- a
tiny ShowAndTell (about 20 000 parameters) and twelve small tensors -- so that the kernels are short and the Python in front of
them is what is measured.  Per class two settings: `plain` (the one clamp + Adam launch) and `full` (global norm + weight decay with
the 1-D parameters exempt + averaged weights: sum of squares, AdamW, EMA).

Only public names are used, so the file runs unchanged against another checkout: --root DIR imports the package from there.
REGIONS regions of STEPS calls per setting, the settings taking turns; a region is timed with time.perf_counter around its calls
(the device is synchronized before and after, outside the clock for the host figure, inside for the other).  Reported per setting,
in microseconds per call: median, lowest and highest region of the host time, and the median with the device drained.
One JSON object on stdout."""
import argparse
import importlib
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--regions", type=int, default=9)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    sat = importlib.import_module("show-and-tell_amd")
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is measured on a CPU"

    def train_step(full):
        torch.manual_seed(1)
        model = sat.ShowAndTell(32, 32, 53, 1, arch=dict(layers=(1, 1, 1, 1), width=8), compute_dtype="f32").cuda().train()
        ts = sat.TrainStep(model)
        if full:
            ts.max_grad_norm, ts.weight_decay, ts.no_decay, ts.ema_decay = 1.0, 0.01, sat.no_decay_names(model), 0.999
        return ts.optimizer_step, ts.check_ids

    def fused(full):
        g = torch.Generator().manual_seed(2)
        params = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in [(64, 33), (33,)] * 6]
        kw = dict(max_norm=1.0, weight_decay=0.01, no_decay=[p for p in params if p.dim() == 1]) if full else {}
        opt = sat.FusedClampAdam(params, lr=1e-3, clip=0.1, **kw)
        if full:
            opt.ema_decay = 0.999
        for p in params:
            p.grad.normal_()
        return opt.step, lambda: None

    sides = {"train_step_plain": train_step(False), "train_step_full": train_step(True),
             "fused_clamp_adam_plain": fused(False), "fused_clamp_adam_full": fused(True)}
    host, drained = {k: [] for k in sides}, {k: [] for k in sides}
    for k, (fn, settle) in sides.items():
        for _ in range(50):
            fn()
        settle()
    for _ in range(args.regions):
        for k, (fn, settle) in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            settle()
            host[k].append((t1 - t0) * 1e6 / args.steps)
            drained[k].append((t2 - t0) * 1e6 / args.steps)
    med = lambda v: round(sorted(v)[len(v) // 2], 2)
    print(json.dumps({"root": os.path.abspath(args.root), "steps": args.steps, "regions": args.regions,
                      "us_per_call": {k: dict(host_median=med(host[k]), host_lowest=round(min(host[k]), 2),
                                              host_highest=round(max(host[k]), 2), drained_median=med(drained[k])) for k in sides}}))


if __name__ == "__main__":
    main()
