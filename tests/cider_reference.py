"""`CiderScorer.compute_score()` (pycocoevalcap/cider/cider_scorer.py:93-181) restated in pure Python f64 on lists of token ids,
for the tests.  It does the reference's operations n-gram by n-gram in the reference's own order (dicts in insertion order), so
it can differ from the reference only where `math` and numpy round a `log`, an `exp` or a short sum differently."""
import math


def precook(ids, n=4):
    """cider_scorer.py:11-26: n-gram (tuple of ids) -> count, orders 1..n, in order of first occurrence"""
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(ids) - k + 1):
            g = tuple(ids[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return counts


def document_frequency(refs, n=4):
    """cider_scorer.py:93-103: n-gram -> number of images whose reference set holds it"""
    df = {}
    for image in refs:
        for g in set(g for ref in image for g in precook(ref, n)):
            df[g] = df.get(g, 0) + 1
    return df


def _counts2vec(counts, df, ref_len, n):
    vec = [dict() for _ in range(n)]
    norm = [0.0] * n
    length = 0
    for g, tf in counts.items():
        o = len(g) - 1
        vec[o][g] = float(tf) * (ref_len - math.log(max(1.0, float(df.get(g, 0)))))
        norm[o] += vec[o][g] * vec[o][g]
        if o == 1:                  # the reference's `length`: the bigrams' tf (cider_scorer.py:128)
            length += tf
    return vec, [math.sqrt(v) for v in norm], length


def _sim(vh, vr, nh, nr, lh, lr, n, sigma):
    delta = float(lh - lr)
    val = [0.0] * n
    for o in range(n):
        for g, w in vh[o].items():
            wr = vr[o].get(g, 0.0)
            val[o] += min(w, wr) * wr
        if nh[o] != 0 and nr[o] != 0:
            val[o] /= nh[o] * nr[o]
        val[o] *= math.exp(-(delta ** 2) / (2 * sigma ** 2))
    return val


class Corpus:
    """refs: per image, a list of id lists.  The document frequencies and the cooked references are computed once."""

    def __init__(self, refs, n=4, sigma=6.0):
        self.n, self.sigma = n, sigma
        self.df = document_frequency(refs, n)
        self.ref_len = math.log(float(len(refs)))
        self.refs = [[_counts2vec(precook(r, n), self.df, self.ref_len, n) for r in image] for image in refs]

    def score_one(self, hyp, image):
        vec, norm, length = _counts2vec(precook(hyp, self.n), self.df, self.ref_len, self.n)
        score = [0.0] * self.n
        for vr, nr, lr in self.refs[image]:
            val = _sim(vec, vr, norm, nr, length, lr, self.n, self.sigma)
            score = [a + b for a, b in zip(score, val)]
        s = 0.0
        for v in score:
            s += v
        return s / self.n / len(self.refs[image]) * 10.0

    def score(self, hyps, image_index):
        """(mean, scores) for hypothesis id lists against the references of image_index[b]"""
        scores = [self.score_one(h, i) for h, i in zip(hyps, image_index)]
        return math.fsum(scores) / len(scores), scores


def truncate(row, end_id):
    """eval.py:103-109: the ids in front of the first end_id"""
    row = list(row)
    return row[:row.index(end_id)] if end_id in row else row
