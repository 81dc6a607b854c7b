"""Cost of BLEU and ROUGE-L on the device (langstats.py, csrc/sat_langstats.hip) next to CIDEr (cider.py) at validation size: the
synthetic corpus of tools/bench_cider.py (5 000 images x 5 references, Zipf-distributed ids over 10 000, 8-16 tokens), a batch of
64 rows of 20 tokens.  Two figures per metric, both HIP-event times of regions of --calls calls, median over --regions regions
after a warm-up, the three metrics taking turns region by region:

    *_method_us   the Python method (`CiderScorer.score`, `BleuScorer.update`, `RougeLScorer.score`): output allocation, the image
                  index upload check and both launches -- what a validation loop pays per batch
    *_entry_us    the C entry point alone on preallocated outputs (sat_cider_score, sat_bleu_comps with totals and mean,
                  sat_rouge_l_score): the launches, as close to the kernels as events around a call get

One JSON object on stdout.  It needs the MI355X and fails without it."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bleu_rouge_reference as R  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
IMAGES, REFS, V, B, T, END = 5000, 5, 10000, 64, 20, 2


def zipf_ids(rng, n):
    """ids 3 .. V-1 with probability ~ 1 / rank"""
    p = 1.0 / np.arange(1, V - 2)
    return (3 + rng.choice(V - 3, size=n, p=p / p.sum())).tolist()


def regions(fns, calls, n_regions, warmup):
    """median over regions of (event time of `calls` calls) / calls, in microseconds, per function; the functions take turns"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(n_regions):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / calls)
    return {name: {"median": float(np.median(t)), "min": min(t), "max": max(t)} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_langstats needs the MI355X")
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
    index = torch.tensor(idx, dtype=torch.int32).cuda()
    cider = sat.CiderScorer(refs)
    bleu, rouge = sat.BleuScorer.from_scorer(cider), sat.RougeLScorer.from_scorer(cider)

    method = regions({"cider": lambda: cider.score(ids, index, end_id=END), "bleu": lambda: bleu.update(ids, index, end_id=END),
                      "rouge": lambda: rouge.score(ids, index, end_id=END)}, args.calls, args.regions, args.warmup)

    f64 = dict(dtype=torch.float64, device=ids.device)
    scores, mean, sentence, mean4 = torch.empty(B, **f64), torch.empty(1, **f64), torch.empty(B, 4, **f64), torch.empty(4, **f64)
    comps = torch.empty(B, 10, dtype=torch.int64, device=ids.device)
    totals = torch.zeros(10, dtype=torch.int64, device=ids.device)
    lib, s = L.load(), L.stream()
    p = {k: v.data_ptr() for k, v in dict(ids=ids, index=index, scores=scores, mean=mean, sentence=sentence, mean4=mean4, comps=comps,
                                          totals=totals).items()}
    entry = regions({
        "cider": lambda: lib.sat_cider_score(C.byref(cider._corpus), p["ids"], T, B, T, None, END, p["index"], cider.sigma, p["scores"],
                                             p["mean"], s),
        "bleu": lambda: lib.sat_bleu_comps(C.byref(bleu._corpus), p["ids"], T, B, T, None, END, p["index"], p["comps"], p["sentence"],
                                           p["mean4"], p["totals"], s),
        "rouge": lambda: lib.sat_rouge_l_score(C.byref(rouge._corpus), p["ids"], T, B, T, None, END, p["index"], rouge.beta, p["scores"],
                                               p["mean"], s)}, args.calls, args.regions, args.warmup)

    bleu.reset()
    sent = bleu.update(ids, index, end_id=END)
    r_mean, r_scores = rouge.score(ids, index, end_id=END)
    want = R.bleu(hyps, refs, idx)
    err_b = float(np.abs(sent.cpu().numpy() - np.asarray(want[1])).max())
    err_c = float(np.abs(bleu.compute().cpu().numpy() - np.asarray(want[3])).max())
    err_r = float(np.abs(r_scores.cpu().numpy() - np.asarray(R.rouge_l(hyps, refs, idx)[1])).max())
    out = {"images": IMAGES, "refs_per_image": REFS, "B": B, "T": T, "calls_per_region": args.calls, "regions": args.regions}
    for name in ("cider", "bleu", "rouge"):
        out[name + "_method_us"], out[name + "_entry_us"] = method[name]["median"], entry[name]["median"]
        out[name + "_method_us_min_max"] = [method[name]["min"], method[name]["max"]]
        out[name + "_entry_us_min_max"] = [entry[name]["min"], entry[name]["max"]]
    out.update({"bleu_4_corpus": float(bleu.compute().cpu()[3]), "rouge_l": float(r_mean.cpu()[0]),
                "max_abs_err_bleu_sentence": err_b, "max_abs_err_bleu_corpus": err_c, "max_abs_err_rouge": err_r})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
