"""Consensus reranking (`sat_consensus_rerank`, include/sat_hip.h) restated in pure Python f64 for the tests, on top of
cider_reference's `precook` / `_counts2vec` / `_sim`: candidate i of an image is the hypothesis and every other candidate j of the
same image a single reference, with the corpus's document frequencies.  The uniform utility is `CiderScorer.compute_cider()` of
candidate i with the other K - 1 candidates as its reference set, operation for operation; the weighted form and the pairwise
matrix follow the header."""
import math

import cider_reference as R

N = 4


def tokens(row, as_reference):
    """an id outside [0, 2**31) is no token: -1 where the row is the hypothesis, -2 where it is the reference"""
    return [t if 0 <= t < 2 ** 31 else (-2 if as_reference else -1) for t in row]


def corpus_df(refs):
    """(document frequencies, log(images)) of a corpus given as per-image lists of id lists"""
    return R.document_frequency(refs, N), math.log(float(len(refs)))


def image(cands, df, log_images, sigma=6.0, weights=None):
    """cands: the K id lists of one image, already cut to their lengths.  Returns (utility [K], pair [K][K])."""
    K = len(cands)
    hyp = [R._counts2vec(R.precook(tokens(c, False), N), df, log_images, N) for c in cands]
    ref = [R._counts2vec(R.precook(tokens(c, True), N), df, log_images, N) for c in cands]
    utility, pair = [], []
    for i in range(K):
        vec, norm, length = hyp[i]
        tot, den, row = [0.0] * N, 0.0, []
        for j in range(K):
            if j == i:
                row.append(0.0)
                continue
            vr, nr, lr = ref[j]
            val = R._sim(vec, vr, norm, nr, length, lr, N, sigma)
            row.append((((val[0] + val[1]) + val[2]) + val[3]) / N * 10.0)
            if weights is None:
                tot = [a + b for a, b in zip(tot, val)]
            else:
                tot = [a + weights[j] * b for a, b in zip(tot, val)]
                den += weights[j]
        s = (((tot[0] + tot[1]) + tot[2]) + tot[3]) / N
        if weights is None:
            utility.append(s / (K - 1) * 10.0 if K > 1 else 0.0)
        else:
            utility.append(s / den * 10.0 if den != 0.0 else 0.0)
        pair.append(row)
    return utility, pair


def batch(cands, df, log_images, sigma=6.0, weights=None):
    """cands: [B][K] id lists.  Returns (utility [B][K], pair [B][K][K], best [B]: the first slot of maximal utility)."""
    out = [image(c, df, log_images, sigma, None if weights is None else weights[b]) for b, c in enumerate(cands)]
    utility, pair = [u for u, _ in out], [p for _, p in out]
    return utility, pair, [u.index(max(u)) for u in utility]
