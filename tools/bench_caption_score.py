"""Cost of scoring given captions (`DecoderRNN.score_captions`, sat_score_captions) on cached features, one process:

  cross_big      cross=True at B_img 64 x C 320 captions of mean length 12, E 256, H 512, V 10 000 -- the image-sentence ranking
                 matrix; its logits would be N * V * 4 bytes and are never stored
  projection     sat_vocab_logp alone on that call's N rows: time, and the achieved fraction of the bf16 MFMA peak counting the six
                 bf16 products per f32 multiply-add (2 * 6 * N * V * H flop)
  cross_small    the same at B_img 16 x C 80, the largest size at which the alternative's logits fit comfortably
  forward_small  the only route without score_captions: `forward` on hand-repeated inputs (its [N, V] logits stored), then torch
                 log_softmax + gather, at B_img 16 x C 80

HIP events around REGIONS regions of STEPS calls after WARMUP calls; the median region is reported.  One JSON object on stdout."""
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
PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA peak of the MI355X (bench.py's figure)


def regions(fn, n_regions, steps):
    out = []
    for _ in range(n_regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return sorted(out)[len(out) // 2]


def captions(Cn, gen):
    lengths = torch.randint(4, 21, (Cn,), generator=gen).tolist()              # mean 12
    caps = torch.randint(3, V, (Cn, T), generator=gen)
    caps[:, 0] = 1
    return caps.cuda(), lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.manual_seed(123)
    gen = torch.Generator().manual_seed(5)
    dec = sat.DecoderRNN(E, H, V, 1).cuda().eval()
    with torch.no_grad():
        dec.linear.weight.mul_(8.0)                                            # a sharper output layer than the initial one
    lib, st = L.load(), L.stream()
    res = {"shape": dict(E=E, H=H, V=V, T=T), "steps": args.steps, "regions": args.regions, "warmup": args.warmup,
           "workspace_budget": sat.score.WORKSPACE_BUDGET}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return round(regions(fn, args.regions, args.steps), 4)

    for name, B_img, Cn in (("cross_big", 64, 320), ("cross_small", 16, 80)):
        caps, lengths = captions(Cn, gen)
        feats = torch.randn(B_img, E, generator=gen).cuda()
        N = B_img * sum(lengths)
        res[name] = dict(B_img=B_img, C=Cn, N=N, mean_length=round(sum(lengths) / Cn, 2), logits_bytes_never_stored=N * V * 4,
                         workspace_bytes=lib.sat_score_captions_ws_bytes(B_img, B_img * Cn, N, E, H, V, 1),
                         ms=timed(lambda: dec.score_captions(feats, caps, lengths, cross=True)))
        if name == "cross_big":
            hs = torch.randn(N, H, device="cuda")
            tgt = torch.randint(0, V, (N,), device="cuda")
            tok = torch.empty(N, device="cuda")
            need = lib.sat_vocab_logp_ws_bytes(N, H, V)
            ws, ws_ptr = L.workspace256(need, "cuda")
            packed = torch.empty(lib.sat_gemm_f32x3_packed_bytes(V, H), dtype=torch.uint8, device="cuda")
            L.check(lib.sat_gemm_f32x3_pack(dec.linear.weight.data_ptr(), V, H, packed.data_ptr(), st), "pack")

            def project():
                L.check(lib.sat_vocab_logp(hs.data_ptr(), H, dec.linear.weight.data_ptr(), packed.data_ptr(), dec.linear.bias.data_ptr(),
                                           tgt.data_ptr(), N, H, V, tok.data_ptr(), None, ws_ptr, need, st), "sat_vocab_logp")
            ms = timed(project)
            tf = 12.0 * N * V * H / (ms * 1e-3) / 1e12
            res["projection"] = dict(N=N, ms=ms, workspace_bytes=need, bf16_tflops=round(tf, 1), peak_bf16_tflops=PEAK_BF16_TFLOPS,
                                     frac_of_bf16_mfma_peak=round(tf / PEAK_BF16_TFLOPS, 4))
            del hs, tgt, tok, ws, packed
        if name == "cross_small":
            # forward on hand-repeated inputs: rows caption-major, longest caption first (forward wants sorted lengths)
            order = sorted(range(Cn), key=lambda i: -lengths[i])
            caps_r = caps[order].repeat_interleave(B_img, 0).contiguous()
            feats_r = feats.repeat(Cn, 1).contiguous()
            lengths_r = [lengths[i] for i in order for _ in range(B_img)]
            targets, _ = sat.pack_validation_targets(caps_r, lengths_r)

            def forward_route():
                with torch.no_grad():
                    logits = dec(feats_r, caps_r, lengths_r)
                    return torch.log_softmax(logits, 1).gather(1, targets.view(-1, 1))
            res["forward_small"] = dict(B_img=B_img, C=Cn, N=N, logits_bytes=N * V * 4, ms=timed(forward_route))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
