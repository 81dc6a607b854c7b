"""Cost of the constrained beam search next to the plain one, one process, batch 64, E 256, H 512, V 10 000, 20 steps, beam 5
(`DecoderRNN.sample_beam` on cached features, end_id 2): the plain loop (sat_beam_decode), then the loop under suppress_ids
[3, 0, 1] + min_length 6 with, in turn, no n-gram rule, no_repeat_ngram_size 1 / 2 / 3, block_repeat, bigrams + block_repeat, and
that with length_penalty 0.7 (sat_beam_decode_ex).  Then the selection alone on the same logits over 320 rows: `sat_beam_step`
against `sat_beam_step_ex` at steps 0, 1, 10 and 19 of a 20-step record (the depth of the prefix walk), trigram blocking on.
Median of REGIONS regions of STEPS calls, device-synchronised on both sides.  One JSON object on stdout.
With SAT_LIB naming a build without the constrained entry points only the plain figures are measured; SAT_BEAM_HISTORY=0 makes
the n-gram loops walk the records instead of keeping a per-slot history (DESIGN.md 3.3h compares the two)."""
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
B, E, H, V, K, T, END = 64, 256, 512, 10000, 5, 20, 2
BASE = dict(suppress_ids=[3, 0, 1], min_length=6)
LOOPS = [("suppress_minlen", {}), ("ngram1", dict(no_repeat_ngram_size=1)), ("ngram2", dict(no_repeat_ngram_size=2)),
         ("ngram3", dict(no_repeat_ngram_size=3)), ("block_repeat", dict(block_repeat=True)),
         ("ngram2_block", dict(no_repeat_ngram_size=2, block_repeat=True)),
         ("ngram2_block_penalty", dict(no_repeat_ngram_size=2, block_repeat=True, length_penalty=0.7))]


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
    dec = sat.DecoderRNN(E, H, V, 1).cuda().eval()
    feats = torch.randn(B, E, device="cuda")
    lib, st = L.load(), L.stream()
    have = hasattr(lib, "sat_beam_decode_ex")
    res = {"shape": dict(B=B, E=E, H=H, V=V, decode_steps=T, beam=K), "steps": args.steps, "regions": args.regions,
           "library": os.path.basename(L.LIB_PATH), "constrained_entry_points": have}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return round(regions(fn, args.regions, args.steps), 4)

    res["beam5_plain_ms"] = timed(lambda: dec.sample_beam(feats, K, END))
    if have:
        for name, kw in LOOPS:
            res["beam5_%s_ms" % name] = timed(lambda: dec.sample_beam(feats, K, END, **BASE, **kw))
        res["beam5_plain_again_ms"] = timed(lambda: dec.sample_beam(feats, K, END))

    # the selection alone, on logits of a trained model's spread (N(0, 2.5^2))
    logits = (torch.randn(B * K, V, device="cuda") * 2.5).contiguous()
    scores, scores2 = torch.zeros(B, K, device="cuda"), torch.empty(B, K, device="cuda")
    parent = torch.empty(B * K, dtype=torch.int32, device="cuda")
    token = torch.empty(B * K, dtype=torch.int64, device="cuda")
    bws = torch.empty(lib.sat_beam_step_ws_bytes(B, K), dtype=torch.uint8, device="cuda")

    def plain():
        L.check(lib.sat_beam_step(logits.data_ptr(), V, scores.data_ptr(), None, -1, B, K, V, parent.data_ptr(), token.data_ptr(),
                                  scores2.data_ptr(), bws.data_ptr(), bws.numel(), st), "sat_beam_step")
    res["kernel_beam_step_320rows_us"] = round(timed(plain) * 1e3, 2)
    if have:
        gen = torch.Generator().manual_seed(5)
        parents = torch.stack([torch.stack([torch.randperm(K, generator=gen) for _ in range(B)]) for _ in range(T)])
        parents = parents.to(torch.int32).view(T, B * K).cuda()
        tokens = torch.randint(4, 40, (T, B * K), generator=gen).cuda()
        sup = torch.tensor(BASE["suppress_ids"], dtype=torch.int64, device="cuda")
        for name, n_sup, ngram in (("suppress_only", 3, 0), ("trigram", 3, 3)):
            c = L.SatBeamConstraints(sup.data_ptr(), n_sup, 0, ngram, 0, 0.0)
            for i in (0, 1, 10, 19):
                def one():
                    L.check(lib.sat_beam_step_ex(logits.data_ptr(), V, scores.data_ptr(), None, -1, B, K, V, c, parents.data_ptr(),
                                                 tokens.data_ptr(), i, T, parent.data_ptr(), token.data_ptr(), scores2.data_ptr(),
                                                 bws.data_ptr(), bws.numel(), st), "sat_beam_step_ex")
                res["kernel_beam_step_ex_%s_i%d_us" % (name, i)] = round(timed(one) * 1e3, 2)
        res["kernel_beam_step_320rows_again_us"] = round(timed(plain) * 1e3, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
