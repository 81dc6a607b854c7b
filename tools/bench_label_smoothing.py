"""Cost of label smoothing in the cross entropy at BASELINE configs[1]'s CE shape ([1216, 10000] logits, H 512), one process:

  kernel     sat_ce_rows (gradient in place) against sat_ce_rows_ls (eps 0.1, gradient in place, row_nll and nll_out written), each with
             its sum launch and (`*_no_sum`) with loss_out / nll_out NULL: the row kernels alone
  bf16 pair  sat_vocab_ce_fwd_bf16 against sat_vocab_ce_fwd_bf16_ls (eps 0.1): casts, transposes, projection GEMM, CE
  criterion  sat.CrossEntropy(0.1) forward + backward against torch.nn.CrossEntropyLoss(label_smoothing=0.1) forward + backward on
             the same [1216, 10000] leaf tensor

The two sides of a pair ALTERNATE region by region (REGIONS regions of STEPS calls each, device-synchronised on both sides); the
median region and the lowest and highest are reported per side, in microseconds per call.  The in-place kernels run on their own
output again and again: the values stay finite and the work does not depend on them.  One JSON object on stdout."""
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
N, H, V, EPS = 1216, 512, 10000, 0.1


def alternate(fns, n_regions, steps, warmup):
    """{name: (median, lowest, highest) us per call}: the sides take turns, one region each"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(n_regions):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / steps * 1e6)
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
    tg = torch.randint(0, V, (N,), generator=g).cuda()
    x0 = (torch.randn(N, V, generator=g) * 3).cuda()
    rl, rn, lo, nl = (torch.empty(n, device="cuda") for n in (N, N, 1, 1))
    res = {"shape": dict(N=N, H=H, V=V, eps=EPS), "steps": args.steps, "regions": args.regions, "logits_MB": round(N * V * 4 / 1e6, 1)}

    a, b, c = x0.clone(), x0.clone(), x0.clone()
    res["kernel"] = alternate({
        "sat_ce_rows": lambda: L.check(lib.sat_ce_rows(L.ptr(a), V, L.ptr(tg), N, V, inv, 1, L.ptr(rl), L.ptr(lo), st)),
        "sat_ce_rows_ls": lambda: L.check(lib.sat_ce_rows_ls(L.ptr(b), V, L.ptr(tg), N, V, inv, EPS, L.ptr(b), V, L.ptr(rl), L.ptr(rn),
                                                             L.ptr(lo), L.ptr(nl), st)),
        # the rows alone, without the launch that sums them: what the row kernels themselves cost
        "sat_ce_rows_no_sum": lambda: L.check(lib.sat_ce_rows(L.ptr(a), V, L.ptr(tg), N, V, inv, 1, L.ptr(rl), None, st)),
        "sat_ce_rows_ls_no_sum": lambda: L.check(lib.sat_ce_rows_ls(L.ptr(c), V, L.ptr(tg), N, V, inv, EPS, L.ptr(c), V, L.ptr(rl), L.ptr(rn),
                                                                    None, None, st)),
    }, args.regions, args.steps, args.warmup)

    Hs = torch.tanh(torch.randn(N, H, generator=g)).cuda()
    W = torch.empty(V, H).uniform_(-0.1, 0.1, generator=g).cuda()
    bias = (torch.randn(V, generator=g) * 0.01).cuda()
    wb = lib.sat_vocab_bf16_ws_bytes(N, H, V)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    lg = torch.empty(N, V, device="cuda")
    res["bf16_pair"] = alternate({
        "sat_vocab_ce_fwd_bf16": lambda: L.check(lib.sat_vocab_ce_fwd_bf16(L.ptr(Hs), L.ptr(W), L.ptr(bias), L.ptr(tg), N, H, V, inv, L.ptr(lg),
                                                                           V, L.ptr(rl), L.ptr(lo), L.ptr(ws), wb, st)),
        "sat_vocab_ce_fwd_bf16_ls": lambda: L.check(lib.sat_vocab_ce_fwd_bf16_ls(L.ptr(Hs), L.ptr(W), L.ptr(bias), L.ptr(tg), N, H, V, inv, EPS,
                                                                                 L.ptr(lg), V, L.ptr(rl), L.ptr(rn), L.ptr(lo), L.ptr(nl),
                                                                                 L.ptr(ws), wb, st)),
    }, args.regions, max(args.steps // 3, 1), args.warmup)

    x = x0.clone().requires_grad_(True)
    ours, torchs = sat.CrossEntropy(EPS), torch.nn.CrossEntropyLoss(label_smoothing=EPS)

    def fwd_bwd(crit):
        x.grad = None
        crit(x, tg).backward()
    res["criterion_fwd_bwd"] = alternate({"sat.CrossEntropy": lambda: fwd_bwd(ours), "torch.nn.CrossEntropyLoss": lambda: fwd_bwd(torchs)},
                                         args.regions, max(args.steps // 6, 1), args.warmup)
    ours.check_ids()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
