"""`BleuScorer.compute_score(option='closest')` (pycocoevalcap/bleu/bleu_scorer.py:23-83, 198-256) and `Rouge.calc_score`
(pycocoevalcap/rouge/rouge.py:13-75) restated in pure Python on lists of token ids, for the tests.  The integers (lengths, guess,
correct, LCS) are exact; the floats are the reference's operations in the reference's order, so they can differ from it only
where `**`, `math.exp` and numpy's mean round differently."""
import math

SMALL, TINY = 1e-9, 1e-15
EMPTY = object()            # rouge.py splits with split(" "): an empty caption is the one token ""


def precook(ids, n=4):
    """bleu_scorer.py:23-33: (length, n-gram -> count) for orders 1..n"""
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(ids) - k + 1):
            g = tuple(ids[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return len(ids), counts


def comps(hyp, refs, n=4):
    """cook_refs + cook_test(eff='closest'): [testlen, reflen, guess[0..n), correct[0..n)] -- ten integers for n = 4"""
    reflens, maxcounts = [], {}
    for ref in refs:
        rl, counts = precook(ref, n)
        reflens.append(rl)
        for g, c in counts.items():
            maxcounts[g] = max(maxcounts.get(g, 0), c)
    testlen, counts = precook(hyp, n)
    reflen = min((abs(l - testlen), l) for l in reflens)[1]
    guess = [max(0, testlen - k + 1) for k in range(1, n + 1)]
    correct = [0] * n
    for g, c in counts.items():
        correct[len(g) - 1] += min(maxcounts.get(g, 0), c)
    return [testlen, reflen] + guess + correct


def bleu_values(c, n=4):
    """bleu_scorer.py:231-239 and 247-256: the same arithmetic per image and on the corpus totals"""
    testlen, reflen, guess, correct = c[0], c[1], c[2:2 + n], c[2 + n:2 + 2 * n]
    out, bleu = [], 1.0
    for k in range(n):
        bleu *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(bleu ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [v * math.exp(1 - 1 / ratio) for v in out]
    return out


def bleu(hyps, refs, image_index, n=4):
    """(comps int [B][2 + 2n], sentence f64 [B][n], totals int [2 + 2n], corpus f64 [n]) of hypotheses against refs[image_index[b]]"""
    rows = [comps(h, refs[i], n) for h, i in zip(hyps, image_index)]
    totals = [sum(col) for col in zip(*rows)]
    return rows, [bleu_values(r, n) for r in rows], totals, bleu_values(totals, n)


def lcs(a, b):
    """rouge.py:13-34: the length of the longest common subsequence, by the full table"""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


def rouge_tokens(ids):
    return list(ids) if len(ids) else [EMPTY]


def rouge_l_one(hyp, refs, beta=1.2):
    """rouge.py:45-75; also returns the integers behind it: (score, [lcs per reference], len(hyp), [len per reference])"""
    c = rouge_tokens(hyp)
    ls, lens, prec, rec = [], [], [], []
    for ref in refs:
        r = rouge_tokens(ref)
        l = lcs(r, c)
        ls.append(l)
        lens.append(len(r))
        prec.append(l / float(len(c)))
        rec.append(l / float(len(r)))
    p, r = max(prec), max(rec)
    score = ((1 + beta ** 2) * p * r) / float(r + beta ** 2 * p) if p != 0 and r != 0 else 0.0
    return score, ls, len(c), lens


def rouge_l(hyps, refs, image_index, beta=1.2):
    """(mean, scores) of hypotheses against refs[image_index[b]]"""
    scores = [rouge_l_one(h, refs[i], beta)[0] for h, i in zip(hyps, image_index)]
    return math.fsum(scores) / len(scores), scores
