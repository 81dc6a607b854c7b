#!/usr/bin/env python3
"""Generate tests/golden/cider/G11_cider.npz: the scores of the REFERENCE's own `CiderScorer.compute_score()`
(pycocoevalcap/cider/cider_scorer.py) on three corpora of token ids drawn from fixed seeds.

    python tests/golden/make_goldens_cider.py [out_dir]

The reference's file is Python 2 (`xrange`, `dict.iteritems`).  It is loaded from the reference checkout (oracle/build_ref.py
names it) at generation time, unmodified, into a module whose globals already hold `xrange = range` and a `defaultdict` subclass
with `iteritems`; the class then runs as written.  Ids go in as decimal strings joined by blanks, which is what its `precook`
splits.  Only inputs and recorded results are written:

    <c>_tokens i64, <c>_ref_offsets i32, <c>_image_offsets i32      the corpus, flat (caption r = tokens[ref_offsets[r]:ref_offsets[r+1]],
                                                                    image i owns captions image_offsets[i]:image_offsets[i+1])
    <c>_hyp_tokens i64, <c>_hyp_offsets i32                         one hypothesis per image
    <c>_scores f64, <c>_mean f64                                    compute_score()
    <c>_df_ngrams i64 [G,4] (-1 padded), <c>_df_counts i64 [G]      the reference's document_frequency, sorted

for c in  small  (40 images, 8 ids: n-grams repeat, clipping bites, some hypotheses equal a reference; an empty, a one-token and
an all-absent hypothesis),  wide  (10 images, ids up to 2**31 - 1, pairs that differ only above bit 16)  and  one  (a single
image: ref_len = log 1 = 0 and every score is 0)."""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
NAME = "G11_cider.npz"


def load_reference_scorer():
    from oracle.build_ref import reference_checkout
    path = os.path.join(reference_checkout() or "", "pycocoevalcap", "cider", "cider_scorer.py")

    class defaultdict(collections.defaultdict):
        def iteritems(self):
            return self.items()
    glob = {"__name__": "cider_scorer", "xrange": range}
    with open(path) as f:
        code = compile(f.read(), path, "exec")
    exec(code, glob)
    glob["defaultdict"] = defaultdict            # after the module's own `from collections import defaultdict`
    return glob["CiderScorer"]


def reference_scores(CiderScorer, refs, hyps):
    scorer = CiderScorer(n=4, sigma=6.0)
    for hyp, image in zip(hyps, refs):
        scorer += (" ".join(str(t) for t in hyp), [" ".join(str(t) for t in r) for r in image])
    mean, scores = scorer.compute_score()
    # document_frequency is a defaultdict: compute_cider's look-ups of hypothesis n-grams leave zero entries behind, which are not counts
    df = sorted((tuple(int(w) for w in g), int(c)) for g, c in scorer.document_frequency.items() if c > 0)
    return float(mean), np.asarray(scores, dtype=np.float64), df


def small_corpus(rng):
    refs = [[[int(t) for t in rng.integers(0, 8, rng.integers(1, 13))] for _ in range(rng.integers(1, 7))] for _ in range(40)]
    hyps = [[int(t) for t in rng.integers(0, 8, rng.integers(0, 21))] for _ in range(40)]
    hyps[0] = []
    hyps[1] = [refs[1][0][0]]
    hyps[2] = [100, 101, 102, 103, 104, 100, 101]            # no n-gram of it is in the corpus
    for i in (3, 4, 5, 6):
        hyps[i] = list(refs[i][i % len(refs[i])])            # equal to one of the image's references
    hyps[7] = [3, 3, 3, 3, 3, 3, 3, 3]                         # one n-gram many times: clipping
    return refs, hyps


def wide_corpus(rng):
    base = [5, 70000, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30, 12345]
    ids = base + [b + (1 << 16) for b in base[:2]] + [5 + (1 << 24), 5 + (1 << 30), 12345 + (1 << 17)]   # equal low 16 bits
    ids += [int(t) for t in rng.integers(0, 2 ** 31, 6)]
    pick = lambda n: [ids[j] for j in rng.integers(0, len(ids), n)]           # noqa: E731
    refs = [[pick(rng.integers(2, 11)) for _ in range(rng.integers(1, 5))] for _ in range(10)]
    hyps = [pick(rng.integers(1, 15)) for _ in range(10)]
    hyps[0] = list(refs[0][0])
    hyps[1] = [t ^ (1 << 16) for t in refs[1][0]]             # a reference with bit 16 of every id flipped
    return refs, hyps


def one_corpus(rng):
    refs = [[[1, 2, 3, 4, 5], [1, 2, 6]]]
    return refs, [[1, 2, 3, 9]]


def flat(rows):
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    return np.asarray([t for r in rows for t in r], dtype=np.int64), off


def main(out_dir=os.path.join(HERE, "cider")):
    os.makedirs(out_dir, exist_ok=True)
    CiderScorer = load_reference_scorer()
    out = {}
    for name, make, seed in (("small", small_corpus, 1101), ("wide", wide_corpus, 1102), ("one", one_corpus, 1103)):
        refs, hyps = make(np.random.Generator(np.random.PCG64(seed)))
        mean, scores, df = reference_scores(CiderScorer, refs, hyps)
        out[name + "_tokens"], out[name + "_ref_offsets"] = flat([r for image in refs for r in image])
        out[name + "_image_offsets"] = np.cumsum([0] + [len(image) for image in refs]).astype(np.int32)
        out[name + "_hyp_tokens"], out[name + "_hyp_offsets"] = flat(hyps)
        out[name + "_scores"], out[name + "_mean"] = scores, np.float64(mean)
        out[name + "_df_ngrams"] = np.asarray([list(g) + [-1] * (4 - len(g)) for g, _ in df], dtype=np.int64)
        out[name + "_df_counts"] = np.asarray([c for _, c in df], dtype=np.int64)
    np.savez_compressed(os.path.join(out_dir, NAME), **out)
    print("wrote", os.path.join(out_dir, NAME))


if __name__ == "__main__":
    main(*sys.argv[1:2])
