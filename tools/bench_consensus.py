"""Cost of consensus reranking on the device (consensus.py, csrc/sat_cider.hip) at validation size, with tools/bench_cider.py's
corpus: 5 000 images x 5 references (Zipf-distributed ids over 10 000, 8-16 tokens) give the document frequencies.  B = 64 images,
T = 20, K in {5, 8, 32} candidates per image: variations of one caption per image (a shared stretch, then Zipf ids), 6..19 tokens.
Reports the HIP-event time of one `ConsensusReranker.rerank` call (its three launches) as the median of --regions regions of
--calls calls after a warm-up, and beside it, for scale, the same figure of `DecoderRNN.sample_beam(return_all=True)` at the same
B and K (E 256, H 512, V 10 000, one layer, 20 steps; the beam search takes K <= 8).  Text on stdout."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_cider import IMAGES, REFS, V, zipf_ids  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
B, T, END, E, H = 64, 20, 2, 256, 512
KS = (5, 8, 32)


def candidates(rng, K):
    ids = torch.full((B, K, T), END, dtype=torch.int64)
    for b in range(B):
        base = zipf_ids(rng, T)
        for i in range(K):
            n = int(rng.integers(6, T))
            keep = int(rng.integers(n // 2, n + 1))
            ids[b, i, :n] = torch.tensor((base[:keep] + zipf_ids(rng, n))[:n])
    return ids.cuda()


def median_us(fn, calls, regions, warmup):
    """median over `regions` of (HIP-event time of `calls` back-to-back calls) / calls, in microseconds; (median, min, max)"""
    for _ in range(warmup):
        fn()
    per = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / calls)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(1))
    refs = [[zipf_ids(rng, int(rng.integers(8, 17))) for _ in range(REFS)] for _ in range(IMAGES)]
    rr = sat.ConsensusReranker(sat.CiderScorer(refs), end_id=END)
    torch.manual_seed(1)
    decoder = sat.DecoderRNN(E, H, V, 1).cuda().eval()
    feats = torch.randn(B, E, device="cuda")
    print("tools/bench_consensus.py: corpus %d images x %d references, %d trie nodes; B %d, T %d; median (min-max) of %d regions of "
          "%d calls after %d warm-up calls, HIP events, us per call" % (IMAGES, REFS, rr.scorer.n_nodes, B, T, args.regions,
                                                                        args.calls, args.warmup))
    print("%-4s %-34s %-34s %-34s" % ("K", "rerank", "rerank, weights + pairwise", "sample_beam(return_all) E256 H512 V10000"))
    for K in KS:
        ids = candidates(rng, K)
        kept = sat.kept_tokens(ids.view(B * K, T), END).view(B, K)
        w = torch.rand(B, K, dtype=torch.float64, device="cuda")
        plain = median_us(lambda: rr.rerank(ids, kept=kept), args.calls, args.regions, args.warmup)
        full = median_us(lambda: rr.rerank(ids, kept=kept, weights=w, return_pairwise=True), args.calls, args.regions, args.warmup)
        beam = None
        if K <= 8:
            beam = median_us(lambda: decoder.sample_beam(feats, K, END, return_all=True), max(args.calls // 5, 1), args.regions, 3)
        fmt = lambda r: "%.1f (%.1f-%.1f)" % r if r else "- (beam_size <= 8)"         # noqa: E731
        print("%-4d %-34s %-34s %-34s" % (K, fmt(plain), fmt(full), fmt(beam)))
        best, utility = rr.rerank(ids, kept=kept)
        print("     mean utility of the pick %.4f, of slot 0 %.4f; picks that are not slot 0: %d of %d"
              % (utility.gather(1, best.view(-1, 1)).mean().item(), utility[:, 0].mean().item(), int((best != 0).sum().item()), B))


if __name__ == "__main__":
    main()
