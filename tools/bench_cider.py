"""Cost of CIDEr on the device (cider.py, csrc/sat_cider.hip) at validation size: a synthetic corpus of 5 000 images x 5 references
(Zipf-distributed ids over 10 000, 8-16 tokens), a batch of 64 rows of 20 tokens.  Reports the HIP-event time of
`CiderScorer.score` (both launches) over --calls calls after a warm-up, the construction time (numpy trie, upload, table insert,
reference norms, the one status read) and the time of the pure-Python f64 restatement (tests/cider_reference.py) for the same
batch with its corpus already cooked.  One JSON object on stdout."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cider_reference as R  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
IMAGES, REFS, V, B, T, END = 5000, 5, 10000, 64, 20, 2


def zipf_ids(rng, n):
    """ids 3 .. V-1 with probability ~ 1 / rank"""
    p = 1.0 / np.arange(1, V - 2)
    return (3 + rng.choice(V - 3, size=n, p=p / p.sum())).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(1))
    refs = [[zipf_ids(rng, int(rng.integers(8, 17))) for _ in range(REFS)] for _ in range(IMAGES)]
    idx = [int(i) for i in rng.integers(0, IMAGES, B)]
    hyps = []
    for b, i in enumerate(idx):                       # half the rows share a stretch with a reference, as decoded captions do
        n = int(rng.integers(6, T))
        hyps.append((refs[i][b % REFS][:n // 2] + zipf_ids(rng, n))[:n] if b % 2 else zipf_ids(rng, n))
    ids = torch.full((B, T), END, dtype=torch.int64)
    for b, h in enumerate(hyps):
        ids[b, :len(h)] = torch.tensor(h)
    ids = ids.cuda()
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    scorer = sat.CiderScorer(refs)
    torch.cuda.synchronize()
    construct_s = time.perf_counter() - t0
    index = torch.tensor(idx, dtype=torch.int32).cuda()

    for _ in range(args.warmup):
        mean, scores = scorer.score(ids, index, end_id=END)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.calls + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for c in range(args.calls):
        mean, scores = scorer.score(ids, index, end_id=END)
        ev[c + 1].record()
    torch.cuda.synchronize()
    per_call = sorted(ev[c].elapsed_time(ev[c + 1]) * 1e3 for c in range(args.calls))

    t0 = time.perf_counter()
    cpu = R.Corpus(refs)
    cook_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_mean, want = cpu.score(hyps, idx)
    cpu_s = time.perf_counter() - t0
    err = float(np.abs(scores.cpu().numpy() - np.asarray(want)).max())
    print(json.dumps({
        "images": IMAGES, "refs_per_image": REFS, "B": B, "T": T, "nodes": scorer.n_nodes, "capacity": scorer.capacity,
        "score_us_median": per_call[len(per_call) // 2], "score_us_min": per_call[0], "score_us_max": per_call[-1],
        "score_us_mean_of_calls": sum(per_call) / len(per_call), "calls": args.calls,
        "construct_s": construct_s, "cpu_restatement_batch_ms": cpu_s * 1e3, "cpu_restatement_cook_corpus_s": cook_s,
        "cider": float(mean.cpu()[0]), "max_abs_err_vs_restatement": err}))


if __name__ == "__main__":
    main()
