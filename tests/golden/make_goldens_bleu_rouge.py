#!/usr/bin/env python3
"""Generate tests/golden/langstats/G12_bleu_rouge.npz: what the REFERENCE's own `BleuScorer.compute_score(option='closest')`
(pycocoevalcap/bleu/bleu_scorer.py; bleu.py:40 passes 'closest') and `Rouge` (pycocoevalcap/rouge/rouge.py) compute on four
corpora of token ids.

    python tests/golden/make_goldens_bleu_rouge.py [out_dir]

Both files are loaded from the reference checkout (oracle/build_ref.py names it) at generation time.  rouge.py compiles under
Python 3 as it is.  bleu_scorer.py is Python 2 (a tuple parameter, `xrange`, `iteritems`, `print` statements): it is converted IN
MEMORY with lib2to3 (fixers tuple_params, xrange, dict, print) and the result executed; nothing converted is written anywhere.
Ids go in as decimal strings joined by blanks.  Only inputs and recorded results are written:

    <c>_tokens i64, <c>_ref_offsets i32, <c>_image_offsets i32      the corpus, flat (as in G11_cider.npz)
    <c>_hyp_tokens i64, <c>_hyp_offsets i32                         one hypothesis per image
    <c>_comps i64 [I,10]                                            per image: testlen, closest reflen, guess[4], correct[4]
    <c>_bleu_list f64 [4,I], <c>_bleus f64 [4]                      compute_score's per-image list and corpus score
    <c>_lcs i64 [R]                                                 my_lcs of the image's hypothesis and each reference (split(" "))
    <c>_rouge_scores f64 [I], <c>_rouge_mean f64                    Rouge.compute_score

for c in  small, wide, one  (the corpora of make_goldens_cider.py, same seeds)  and  edges  (hand-made, below)."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_goldens_cider import flat, one_corpus, small_corpus, wide_corpus  # noqa: E402

NAME = "G12_bleu_rouge.npz"


def reference_file(*parts):
    from oracle.build_ref import reference_checkout
    return os.path.join(reference_checkout() or "", "pycocoevalcap", *parts)


def load_reference_bleu():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # lib2to3 is deprecated, and present
        from lib2to3 import refactor
    path = reference_file("bleu", "bleu_scorer.py")
    tool = refactor.RefactoringTool(["lib2to3.fixes.fix_" + f for f in ("tuple_params", "xrange", "dict", "print")])
    with open(path) as f:
        src = f.read()
    glob = {"__name__": "bleu_scorer"}
    exec(compile(str(tool.refactor_string(src if src.endswith("\n") else src + "\n", path)), path, "exec"), glob)
    return glob["BleuScorer"]


def load_reference_rouge():
    path = reference_file("rouge", "rouge.py")
    glob = {"__name__": "rouge"}
    with open(path) as f:
        exec(compile(f.read(), path, "exec"), glob)
    return glob["Rouge"], glob["my_lcs"]


def words(ids):
    return " ".join(str(t) for t in ids)


def reference_bleu(BleuScorer, refs, hyps):
    scorer = BleuScorer(n=4)
    for hyp, image in zip(hyps, refs):
        scorer += (words(hyp), [words(r) for r in image])
    with contextlib.redirect_stdout(io.StringIO()):
        bleus, bleu_list = scorer.compute_score(option="closest")
    comps = [[c["testlen"], scorer._single_reflen(c["reflen"], "closest", c["testlen"])] + list(c["guess"]) + list(c["correct"])
             for c in scorer.ctest]
    assert sum(c[0] for c in comps) == scorer._testlen and sum(c[1] for c in comps) == scorer._reflen
    return np.asarray(comps, dtype=np.int64), np.asarray(bleu_list, dtype=np.float64), np.asarray(bleus, dtype=np.float64)


def reference_rouge(Rouge, my_lcs, refs, hyps):
    gts = {i: [words(r) for r in image] for i, image in enumerate(refs)}
    res = {i: [words(h)] for i, h in enumerate(hyps)}
    mean, scores = Rouge().compute_score(gts, res)
    lcs = [my_lcs(r.split(" "), res[i][0].split(" ")) for i in range(len(refs)) for r in gts[i]]
    return np.asarray(lcs, dtype=np.int64), np.asarray(scores, dtype=np.float64), np.float64(mean)


def edges_corpus(rng):
    long_ref = [int(t) for t in rng.integers(10, 16, 128)]
    cases = [
        # the closest reference length is a tie (4 and 6 around 5): the shorter wins, whichever comes first
        ([[1, 2, 3, 4, 5, 6], [1, 2, 3, 4]], [1, 2, 3, 9, 5]),
        # unigram 5 is clipped by the first reference (3 of the row's 4), bigram (5, 6) by the second (2 of 2)
        ([[5, 5, 5, 7], [5, 6, 5, 6, 8]], [5, 5, 5, 6, 5, 6]),
        # longer than every reference: no brevity factor
        ([[1, 2, 3], [2, 3]], [1, 2, 3, 4, 5]),
        # shorter than every reference
        ([[1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8]], [1, 2, 3]),
        # equal to a reference
        ([[1, 2], [4, 5, 6, 7, 8]], [4, 5, 6, 7, 8]),
        # an empty hypothesis
        ([[1, 2], [3]], []),
        # an empty reference, with and without an empty hypothesis (ROUGE-L 1.0 for the first)
        ([[1, 2], []], []),
        ([[1, 2], []], [1, 3]),
        # 64 tokens
        ([long_ref[:40], long_ref[20:90]], long_ref[30:94]),
        # a 128-token reference, against a 64-token and a shorter hypothesis
        ([long_ref, [10, 11]], long_ref[5:25] + [99] + long_ref[60:103]),
        ([[12, 13], long_ref], long_ref[100:128] + long_ref[:2]),
        # no token of it occurs in the references
        ([[1, 2, 3], [4, 5]], [50, 51, 52, 50]),
        # the longest common subsequence (1 3 5) is no contiguous run
        ([[1, 2, 3, 4, 5, 6]], [1, 9, 3, 9, 5]),
    ]
    return [c[0] for c in cases], [c[1] for c in cases]


def main(out_dir=os.path.join(HERE, "langstats")):
    os.makedirs(out_dir, exist_ok=True)
    BleuScorer = load_reference_bleu()
    Rouge, my_lcs = load_reference_rouge()
    out = {}
    for name, make, seed in (("small", small_corpus, 1101), ("wide", wide_corpus, 1102), ("one", one_corpus, 1103),
                             ("edges", edges_corpus, 1204)):
        refs, hyps = make(np.random.Generator(np.random.PCG64(seed)))
        out[name + "_tokens"], out[name + "_ref_offsets"] = flat([r for image in refs for r in image])
        out[name + "_image_offsets"] = np.cumsum([0] + [len(image) for image in refs]).astype(np.int32)
        out[name + "_hyp_tokens"], out[name + "_hyp_offsets"] = flat(hyps)
        out[name + "_comps"], out[name + "_bleu_list"], out[name + "_bleus"] = reference_bleu(BleuScorer, refs, hyps)
        out[name + "_lcs"], out[name + "_rouge_scores"], out[name + "_rouge_mean"] = reference_rouge(Rouge, my_lcs, refs, hyps)
    np.savez_compressed(os.path.join(out_dir, NAME), **out)
    print("wrote", os.path.join(out_dir, NAME))


if __name__ == "__main__":
    main(*sys.argv[1:2])
