"""Cost of the unlikelihood term in the cross entropy at BASELINE configs[1]'s CE shape ([1216, 10000] logits = 64 captions of 19
target steps, H 512), one process, timed with device events:

  kernel     sat_ce_rows_ls (the parent commit's kernel) against sat_ce_rows_ul with alpha 0 and alpha 1 on the same buffers: eps 0.1,
             gradient in place, every output written; and (`*_no_sum`) with the scalar outputs NULL: the row kernels alone
  bf16 pair  sat_vocab_ce_fwd_bf16_ls against sat_vocab_ce_fwd_bf16_ul with alpha 0 and alpha 1: casts, transposes, projection, CE
  step       TrainStep.forward_backward on the decoder of that shape (bf16 mode, features in) with unlikelihood 0 and 1

Targets come from 40 ids, so that captions repeat themselves: a row of step t has up to min(t, 39) candidates.  The sides of a group
ALTERNATE region by region (REGIONS regions of STEPS calls each between two events); the median region and the lowest and highest
are reported per side, in microseconds per call: the spread between regions is the noise a difference has to exceed.  The in-place
kernels run on their own output again and again: the values stay finite and the work does not depend on them.  One JSON object."""
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
B, T, H, V, EPS = 64, 19, 512, 10000, 0.1
N = B * T


def alternate(fns, n_regions, steps, warmup):
    """{name: (median, lowest, highest) us per call}: the sides take turns, one region each, device events around a region"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(n_regions):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / steps * 1e3)
    return {k: dict(median_us=round(sorted(v)[len(v) // 2], 2), lowest_us=round(min(v), 2), highest_us=round(max(v), 2))
            for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is measured on a CPU"
    lib, st = L.load(), L.stream()
    g = torch.Generator().manual_seed(3)
    inv = 1.0 / N
    pi = sat.PackInfo.get([T] * B, torch.device("cuda", 0))
    pre = L.ptr(pi.prefix_dev)
    tg = torch.randint(0, 40, (N,), generator=g).cuda()
    x0 = (torch.randn(N, V, generator=g) * 3).cuda()
    rl, rn, ru, lo, nl, ul = (torch.empty(n, device="cuda") for n in (N, N, N, 1, 1, 1))
    res = {"shape": dict(N=N, T=T, H=H, V=V, eps=EPS, target_ids=40), "steps": args.steps, "regions": args.regions,
           "logits_MB": round(N * V * 4 / 1e6, 1)}

    def ls(x, sums=True):
        return lambda: L.check(lib.sat_ce_rows_ls(L.ptr(x), V, L.ptr(tg), N, V, inv, EPS, L.ptr(x), V, L.ptr(rl), L.ptr(rn),
                                                  L.ptr(lo) if sums else None, L.ptr(nl) if sums else None, st))

    def ulk(x, alpha, sums=True):
        return lambda: L.check(lib.sat_ce_rows_ul(L.ptr(x), V, L.ptr(tg), pre, T, N, V, inv, EPS, alpha, L.ptr(x), V, L.ptr(rl), L.ptr(rn),
                                                  L.ptr(ru), L.ptr(lo) if sums else None, L.ptr(nl) if sums else None,
                                                  L.ptr(ul) if sums else None, st))
    bufs = [x0.clone() for _ in range(6)]
    res["kernel"] = alternate({
        "sat_ce_rows_ls": ls(bufs[0]), "sat_ce_rows_ul_alpha0": ulk(bufs[1], 0.0), "sat_ce_rows_ul_alpha1": ulk(bufs[2], 1.0),
        "sat_ce_rows_ls_no_sum": ls(bufs[3], False), "sat_ce_rows_ul_alpha0_no_sum": ulk(bufs[4], 0.0, False),
        "sat_ce_rows_ul_alpha1_no_sum": ulk(bufs[5], 1.0, False)}, args.regions, args.steps, args.warmup)
    del bufs

    Hs = torch.tanh(torch.randn(N, H, generator=g)).cuda()
    W = torch.empty(V, H).uniform_(-0.1, 0.1, generator=g).cuda()
    bias = (torch.randn(V, generator=g) * 0.01).cuda()
    wb = lib.sat_vocab_bf16_ws_bytes(N, H, V)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    lg = torch.empty(N, V, device="cuda")

    def bf_ul(alpha):
        return lambda: L.check(lib.sat_vocab_ce_fwd_bf16_ul(L.ptr(Hs), L.ptr(W), L.ptr(bias), L.ptr(tg), pre, T, N, H, V, inv, EPS, alpha,
                                                            L.ptr(lg), V, L.ptr(rl), L.ptr(rn), L.ptr(ru), L.ptr(lo), L.ptr(nl), L.ptr(ul),
                                                            L.ptr(ws), wb, st))
    res["bf16_pair"] = alternate({
        "sat_vocab_ce_fwd_bf16_ls": lambda: L.check(lib.sat_vocab_ce_fwd_bf16_ls(L.ptr(Hs), L.ptr(W), L.ptr(bias), L.ptr(tg), N, H, V, inv, EPS,
                                                                                 L.ptr(lg), V, L.ptr(rl), L.ptr(rn), L.ptr(lo), L.ptr(nl),
                                                                                 L.ptr(ws), wb, st)),
        "sat_vocab_ce_fwd_bf16_ul_alpha0": bf_ul(0.0), "sat_vocab_ce_fwd_bf16_ul_alpha1": bf_ul(1.0)},
        args.regions, max(args.steps // 3, 1), args.warmup)

    # one teacher-forced step (forward + backward, no optimizer) of the decoder of this shape in the bf16 mode, features in
    E = 256
    feats = torch.randn(B, E, generator=g).cuda()
    caps = torch.randint(4, 40, (B, T + 1), generator=g)
    caps[:, 0] = 1
    batch = (feats, caps.cuda(), [T + 1] * B)
    steps = {}
    for name, alpha in (("step_unlikelihood_0", 0.0), ("step_unlikelihood_1", 1.0)):
        model = sat.ShowAndTell(E, H, V, 1, arch=dict(layers=(1, 1, 1, 1), width=8), compute_dtype="bf16").cuda().train()
        ts = sat.TrainStep(model)
        ts.unlikelihood = alpha
        assert ts.decoder_gemm_dtype == "bf16"
        steps[name] = (lambda ts=ts: ts.forward_backward(batch, inv))
    res["step_fwd_bwd"] = alternate(steps, args.regions, max(args.steps // 10, 1), 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
