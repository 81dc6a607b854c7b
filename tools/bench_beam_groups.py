"""Cost of the diverse beam search next to the plain one, one process, batch 64, E 256, H 512, V 10 000, 20 steps
(`DecoderRNN.sample_beam` on cached features, end_id 2): the plain loops at beam 6 and beam 8 (sat_beam_decode), then the grouped
loops at (beam, groups) = (6, 3), (8, 4), (8, 8) with diversity_penalty 0.5 (sat_beam_decode_groups), then the plain loops again.
Then the selection alone on the same logits: `sat_beam_step` against `sat_beam_step_groups` at the same widths.  Last, the mean
number of distinct captions per image among the K results (each cut behind its first end_id) at penalty 0 and 0.5.
Median of REGIONS regions of STEPS calls, device-synchronised on both sides.  One JSON object on stdout.
With SAT_LIB naming a build without the grouped entry points only the plain figures are measured."""
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
B, E, H, V, T, END = 64, 256, 512, 10000, 20, 2
WIDTHS = (6, 8)
GROUPED = ((6, 3), (8, 4), (8, 8))
LAM = 0.5


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


def distinct(ids, scores):
    """mean number of distinct captions per image among the live results, each cut behind its first end_id"""
    ids, scores = ids.cpu().tolist(), scores.cpu().tolist()
    total = 0
    for rows, sc in zip(ids, scores):
        seen = set()
        for row, s in zip(rows, sc):
            if s != float("-inf"):
                seen.add(tuple(row[:row.index(END) + 1] if END in row else row))
        total += len(seen)
    return round(total / len(ids), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(123)
    dec = sat.DecoderRNN(E, H, V, 1).cuda().eval()
    with torch.no_grad():                     # a sharper output layer and an <end> that occurs: captions that can differ and finish
        dec.linear.weight.mul_(8.0)
        dec.linear.bias[END] += 1.0
    feats = torch.randn(B, E, device="cuda")
    lib, st = L.load(), L.stream()
    have = hasattr(lib, "sat_beam_decode_groups")
    res = {"shape": dict(B=B, E=E, H=H, V=V, decode_steps=T), "steps": args.steps, "regions": args.regions,
           "library": os.path.basename(L.LIB_PATH), "grouped_entry_points": have}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return round(regions(fn, args.regions, args.steps), 4)

    for K in WIDTHS:
        res["beam%d_plain_ms" % K] = timed(lambda: dec.sample_beam(feats, K, END))
    if have:
        for K, G in GROUPED:
            res["beam%d_groups%d_ms" % (K, G)] = timed(lambda: dec.sample_beam(feats, K, END, num_beam_groups=G, diversity_penalty=LAM))
        for K in WIDTHS:
            res["beam%d_plain_again_ms" % K] = timed(lambda: dec.sample_beam(feats, K, END))

    # the selection alone, on logits of a trained model's spread (N(0, 2.5^2))
    for K in WIDTHS:
        logits = (torch.randn(B * K, V, device="cuda") * 2.5).contiguous()
        scores, scores2 = torch.zeros(B, K, device="cuda"), torch.empty(B, K, device="cuda")
        parent = torch.empty(B * K, dtype=torch.int32, device="cuda")
        token = torch.empty(B * K, dtype=torch.int64, device="cuda")
        bws = torch.empty(lib.sat_beam_step_ws_bytes(B, K), dtype=torch.uint8, device="cuda")

        def plain():
            L.check(lib.sat_beam_step(logits.data_ptr(), V, scores.data_ptr(), None, -1, B, K, V, parent.data_ptr(), token.data_ptr(),
                                      scores2.data_ptr(), bws.data_ptr(), bws.numel(), st), "sat_beam_step")
        res["kernel_beam_step_K%d_us" % K] = round(timed(plain) * 1e3, 2)
        if have:
            for G in [g for k, g in GROUPED if k == K]:
                def grouped():
                    L.check(lib.sat_beam_step_groups(logits.data_ptr(), V, scores.data_ptr(), None, -1, B, K, V, None, None, None, 0, T, G,
                                                     LAM, parent.data_ptr(), token.data_ptr(), scores2.data_ptr(), bws.data_ptr(),
                                                     bws.numel(), st), "sat_beam_step_groups")
                res["kernel_beam_step_groups_K%d_G%d_us" % (K, G)] = round(timed(grouped) * 1e3, 2)
            res["kernel_beam_step_K%d_again_us" % K] = round(timed(plain) * 1e3, 2)

    if have:
        for K, G in GROUPED:
            for lam in (0.0, LAM):
                ids, sc = dec.sample_beam(feats, K, END, return_all=True, num_beam_groups=G, diversity_penalty=lam)
                res["distinct_captions_K%d_G%d_lambda%s" % (K, G, lam)] = distinct(ids, sc)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
