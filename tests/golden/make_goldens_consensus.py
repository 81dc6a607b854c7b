#!/usr/bin/env python3
"""Generate tests/golden/consensus/G13_consensus.npz: consensus utilities from the REFERENCE's own `CiderScorer`
(pycocoevalcap/cider/cider_scorer.py), loaded unmodified at generation time as make_goldens_cider.py loads it.

    python tests/golden/make_goldens_consensus.py [out_dir]

The utility of candidate i of an image is `compute_cider()` of i with the image's other K - 1 candidates as its reference set,
under the document frequencies of a corpus:
  1. a `CiderScorer` over the corpus, `compute_doc_freq()`;
  2. a second scorer with one entry (candidate i, [the other candidates of its image]) per candidate;
  3. the first scorer's `document_frequency` assigned to it, `compute_cider()` called directly.
`compute_cider` takes ref_len = log(len(crefs)), so the entry count must equal the corpus's image count: the `small` corpus of
make_goldens_cider.py has 40 images, and there are B * K = 8 * 5 = 40 candidates.  For the `one` corpus (a single image: ref_len =
log 1 = 0, every utility 0) every candidate gets a scorer of its own with that one entry.  Only inputs and recorded results are
written:

    <c>_tokens i64, <c>_ref_offsets i32, <c>_image_offsets i32      the corpus, flat, as in G11_cider.npz
    <c>_cand_tokens i64, <c>_cand_offsets i32, <c>_shape i64 [2]    the candidates back to back, image-major; (B, K)
    <c>_utility f64 [B, K]

Candidates of `small`: random ids in [0, 8) of 0..12 tokens (PCG64 seed 1301), then fixed cases: image 0 holds two identical
candidates (slots 1 and 3: a tie), image 1 an empty and a one-token candidate, image 2 two candidates that share n-grams the
corpus lacks, image 3 a clipping pair."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens_cider import flat, load_reference_scorer, one_corpus, small_corpus  # noqa: E402

NAME = "G13_consensus.npz"
B, K = 8, 5


def text(ids):
    return " ".join(str(t) for t in ids)


def corpus_scorer(CiderScorer, refs):
    scorer = CiderScorer(n=4, sigma=6.0)
    for image in refs:
        scorer += (None, [text(r) for r in image])
    scorer.compute_doc_freq()
    return scorer


def utilities(CiderScorer, corpus, entries):
    """compute_cider() of (candidate, other candidates) entries under the corpus's document frequencies"""
    scorer = CiderScorer(n=4, sigma=6.0)
    for cand, others in entries:
        scorer += (text(cand), [text(o) for o in others])
    assert len(scorer.crefs) == len(corpus.crefs)            # the same ref_len
    scorer.document_frequency = corpus.document_frequency
    return [float(s) for s in scorer.compute_cider()]


def small_candidates(rng):
    cands = [[[int(t) for t in rng.integers(0, 8, rng.integers(0, 13))] for _ in range(K)] for _ in range(B)]
    cands[0][3] = list(cands[0][1])                            # identical: equal utilities
    cands[1][0] = []
    cands[1][1] = [5]
    cands[2][0] = [100, 101, 102, 103, 104]                    # n-grams the corpus lacks, shared by two candidates
    cands[2][2] = [100, 101, 102, 103, 9]
    cands[3][1] = [3] * 8                                      # clipping
    cands[3][4] = [3, 3]
    return cands


def main(out_dir=os.path.join(HERE, "consensus")):
    os.makedirs(out_dir, exist_ok=True)
    CiderScorer = load_reference_scorer()
    out = {}

    refs, _ = small_corpus(np.random.Generator(np.random.PCG64(1101)))
    cands = small_candidates(np.random.Generator(np.random.PCG64(1301)))
    entries = [(image[i], image[:i] + image[i + 1:]) for image in cands for i in range(K)]
    small = np.asarray(utilities(CiderScorer, corpus_scorer(CiderScorer, refs), entries), dtype=np.float64).reshape(B, K)

    one_refs, _ = one_corpus(None)
    one_cands = [[[1, 2, 3, 9], [1, 2, 3, 4], [2, 6]]]
    corpus = corpus_scorer(CiderScorer, one_refs)
    one = np.asarray([[utilities(CiderScorer, corpus, [(c, one_cands[0][:i] + one_cands[0][i + 1:])])[0]
                       for i, c in enumerate(one_cands[0])]], dtype=np.float64)

    for name, r, c, u in (("small", refs, cands, small), ("one", one_refs, one_cands, one)):
        out[name + "_tokens"], out[name + "_ref_offsets"] = flat([ref for image in r for ref in image])
        out[name + "_image_offsets"] = np.cumsum([0] + [len(image) for image in r]).astype(np.int32)
        out[name + "_cand_tokens"], out[name + "_cand_offsets"] = flat([cand for image in c for cand in image])
        out[name + "_shape"] = np.asarray(u.shape, dtype=np.int64)
        out[name + "_utility"] = u
    np.savez_compressed(os.path.join(out_dir, NAME), **out)
    print("wrote", os.path.join(out_dir, NAME))


if __name__ == "__main__":
    main(*sys.argv[1:2])
