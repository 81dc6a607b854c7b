"""GPU: CIDEr on the device (cider.py, csrc/sat_cider.hip) against the scores recorded from the reference's own `CiderScorer`
(tests/golden/cider/G11_cider.npz) and, on random corpora, against the pure-Python restatement (tests/cider_reference.py).

The bound is 1e-9 absolute on scores <= 10, compared in f64: a score is fewer than 10^3 f64 operations of <= 2 ulp, i.e. an
expected rounding of ~2e-12, so the margin is ~500x -- and nine orders below a score difference that matters."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cider_reference as R  # noqa: E402
from test_cider_host import load_corpus  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
cider = importlib.import_module("show-and-tell_amd.cider")
TOL = 1e-9
END = 2


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cider", "G11_cider.npz"))


def rows_tensor(hyps, T, end_id=END, terminate=True):
    """hyps as an int64 [B, T] device matrix: each row its tokens, then end_id (when it fits and `terminate`), then junk ids"""
    ids = torch.full((len(hyps), T), 7, dtype=torch.int64)
    for b, h in enumerate(hyps):
        ids[b, :len(h)] = torch.tensor(h, dtype=torch.int64)
        if terminate and len(h) < T:
            ids[b, len(h)] = end_id
    return ids.cuda()


def check(mean, scores, want_mean, want_scores, what):
    got, gm = scores.cpu().numpy(), float(mean.cpu()[0])
    assert scores.dtype == torch.float64 and mean.dtype == torch.float64 and tuple(mean.shape) == (1,)
    err = np.abs(got - np.asarray(want_scores, dtype=np.float64)).max()
    print("%s: max |score - want| = %.3g, |mean - want| = %.3g" % (what, err, abs(gm - want_mean)))
    assert err <= TOL and abs(gm - want_mean) <= TOL


@pytest.mark.parametrize("c", ["small", "wide", "one"])
def test_golden_corpora(golden, c):
    refs, hyps = load_corpus(golden, c)
    scorer = sat.CiderScorer(refs)
    T = max(len(h) for h in hyps)
    ids = rows_tensor(hyps, T, terminate=False)              # the small corpus's ids include 2: the lengths come through `kept`
    kept = torch.tensor([len(h) for h in hyps], dtype=torch.int32).cuda()
    mean, scores = scorer.score(ids, list(range(len(refs))), end_id=END, kept=kept)
    check(mean, scores, float(golden[c + "_mean"]), golden[c + "_scores"], c)
    if c == "one":
        assert not scores.cpu().numpy().any() and float(mean.cpu()[0]) == 0.0


def random_refs(rng, images, per_image, vocab, lo=1, hi=13):
    return [[[int(t) for t in rng.integers(3, 3 + vocab, rng.integers(lo, hi))] for _ in range(per_image)] for _ in range(images)]


@pytest.fixture(scope="module")
def corpora():
    """(refs, restatement, device scorer) with 1 and with 7 references per image; one reference of the second has 128 tokens"""
    rng = np.random.Generator(np.random.PCG64(2024))
    out = {}
    for per_image, images in ((1, 50), (7, 30)):
        refs = random_refs(rng, images, per_image, vocab=10)
        if per_image == 7:
            refs[4][2] = [int(t) for t in rng.integers(3, 9, 128)]
            refs[5][0] = [int(t) for t in rng.integers(3, 13, 70)]
        out[per_image] = (refs, R.Corpus(refs), sat.CiderScorer(refs))
    return out


LENGTHS = (0, 1, 2, 3, 4, 20, 64)


def draw_hyps(rng, refs, idx, lengths):
    hyps = []
    for b, (i, n) in enumerate(zip(idx, lengths)):
        if b % 3 == 0 and n:                                  # a stretch of a reference, so that n-grams of every order match
            src = refs[i][(b + 2) % len(refs[i])]
            h = (src * (n // len(src) + 1))[:n]
        else:
            h = [int(t) for t in rng.integers(3, 13, n)]
        hyps.append(h)
    return hyps


@pytest.mark.parametrize("per_image", [1, 7])
@pytest.mark.parametrize("B", [1, 37])
def test_random_corpus_vs_restatement(corpora, per_image, B):
    """rows of 0, 1, 2, 3, 4, 20 and 64 tokens in one [B, 64] batch: the 64-token rows have no end_id, the empty ones start with
    it; one image index comes several times; `kept` given and `kept` derived from end_id give the same bits"""
    refs, ref, scorer = corpora[per_image]
    rng = np.random.Generator(np.random.PCG64(7 * B + per_image))
    idx = [4, 5, 4, 4] + [int(i) for i in rng.integers(0, len(refs), 33)]
    lengths = [64, 20] + [LENGTHS[b % 7] for b in range(35)]
    if B == 1:
        idx, lengths = [4], [20]
    hyps = draw_hyps(rng, refs, idx, lengths)
    ids = rows_tensor(hyps, 64)
    assert B == 1 or ((ids[:, 0] == END).any() and (ids != END).all(dim=1).any())
    want_mean, want = ref.score(hyps, idx)
    mean, scores = scorer.score(ids, idx, end_id=END)
    check(mean, scores, want_mean, want, "refs/image %d, B %d" % (per_image, B))
    assert B == 1 or max(want) > 1.0                          # the batch is not all zeros
    kept = sat.kept_tokens(ids, END)
    assert kept.cpu().tolist() == lengths
    mean_k, scores_k = scorer.score(ids, torch.tensor(idx, dtype=torch.int32).cuda(), end_id=END, kept=kept)
    assert torch.equal(scores_k.view(torch.int64), scores.view(torch.int64)) and torch.equal(mean_k.view(torch.int64), mean.view(torch.int64))


def test_rows_of_twenty_tokens_and_a_single_row(corpora):
    """T = 20, what `sample` returns; a 1-D row is one caption"""
    refs, ref, scorer = corpora[7]
    rng = np.random.Generator(np.random.PCG64(99))
    idx = [int(i) for i in rng.integers(0, len(refs), 16)]
    lengths = [20, 0, 19] + [int(n) for n in rng.integers(1, 20, 13)]
    hyps = draw_hyps(rng, refs, idx, lengths)
    ids = rows_tensor(hyps, 20)
    want_mean, want = ref.score(hyps, idx)
    check(*scorer.score(ids, idx), want_mean, want, "T = 20")
    mean1, scores1 = scorer.score(ids[3], [idx[3]])
    check(mean1, scores1, want[3], [want[3]], "one row")


def test_long_reference_under_a_wide_sigma(corpora):
    """at sigma = 6 a 64-token row against the 128-token reference is weighted exp(-64^2 / 72) ~ 0; sigma = 40 lets that
    reference's term frequencies and norm reach the score"""
    refs, _, _ = corpora[7]
    hyps = [refs[4][2][:64], refs[4][2][40:104], refs[5][0][:64], refs[4][2][:50]]
    idx = [4, 4, 5, 4]
    want_mean, want = R.Corpus(refs, sigma=40.0).score(hyps, idx)
    assert min(want) > 0.05
    check(*sat.CiderScorer(refs, sigma=40.0).score(rows_tensor(hyps, 64), idx), want_mean, want, "sigma 40")


def test_two_calls_give_the_same_bits(corpora):
    refs, ref, scorer = corpora[7]
    rng = np.random.Generator(np.random.PCG64(5))
    idx = [int(i) for i in rng.integers(0, len(refs), 37)]
    ids = rows_tensor(draw_hyps(rng, refs, idx, [LENGTHS[b % 7] for b in range(37)]), 64)
    a, b = scorer.score(ids, idx), scorer.score(ids, idx)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    again = sat.CiderScorer(refs).score(ids, idx)             # another table build: the slots may differ, the scores may not
    assert torch.equal(a[1].view(torch.int64), again[1].view(torch.int64))


def test_probing_wraps_round_the_end_of_the_table():
    """five unigram keys that all start at the last two slots of a 16-slot table (the minimum for five nodes): three of them
    can only land past the end, in slots 0.., and every one must be found again"""
    cand = np.arange(3, 4000, dtype=np.uint64)
    toks = [int(t) for t in cand[cider.table_slot(cand, 16) >= 14][:5]]
    assert len(toks) == 5
    refs = [[[toks[0]], [toks[1]], [toks[2]]], [[toks[3]], [toks[4]]]]
    scorer = sat.CiderScorer(refs)
    assert scorer.n_nodes == 5 and scorer.capacity == 16 == cider.min_capacity(5)
    keys = scorer.table_keys.cpu().numpy().view(np.uint64)
    used = np.nonzero(keys != np.uint64(2 ** 64 - 1))[0].tolist()
    assert used == [0, 1, 2, 14, 15] and sorted(keys[used].tolist()) == sorted(toks)
    nodes = scorer.table_nodes.cpu().numpy()
    assert sorted(nodes[used].tolist()) == [1, 2, 3, 4, 5]
    hyps, idx = [[t] for t in toks] + [[toks[3]], [3999]], [0, 0, 0, 1, 1, 0, 1]
    want_mean, want = R.Corpus(refs).score(hyps, idx)
    assert min(want[:5]) > 0.1 and want[5] == want[6] == 0.0
    check(*scorer.score(rows_tensor(hyps, 4), idx), want_mean, want, "wrapped table")


def test_a_duplicated_key_is_reported_not_inserted():
    with pytest.raises(RuntimeError, match="duplicate key"):
        cider.build_table(np.array([5, 9, 5, 11], dtype=np.uint64))
    tk, tn = cider.build_table(np.array([5, 9, 11], dtype=np.uint64))         # the same keys once each: fine
    assert tk.numel() == 8 and sorted(tn.cpu().tolist()) == [0, 0, 0, 0, 0, 1, 2, 3]


def test_validation_step_returns_cider_of_its_own_ids():
    from oracle import decoder as OD
    from oracle import encoder as OE
    tiny = dict(layers=(1, 1, 1, 1), width=8)
    E, H, V, Lh, B, T = 32, 64, 120, 1, 5, 9
    gen = torch.Generator().manual_seed(77)
    ep, eb = OE.init_encoder_params(E, tiny, generator=gen, randomize_bn=True)
    dp = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    model = sat.ShowAndTell(E, H, V, Lh, arch=tiny, compute_dtype="f32")
    model.encoder.load_state_dict({**ep, **eb})
    model.decoder.load_state_dict(dp)
    model.cuda().eval()
    images = torch.randn(B, 3, 64, 64, generator=gen).cuda()
    lengths = [9, 9, 7, 4, 2]
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, V, (max(l - 2, 0),), generator=gen)
        caps[b, l - 1] = 2
    caps = caps.cuda()
    plain = sat.validation_step(model, images, caps, lengths, end_id=END)
    assert sorted(plain) == ["ids", "kept", "loss"]
    decoded = [R.truncate(r, END) for r in plain["ids"].cpu().tolist()]
    rng = np.random.Generator(np.random.PCG64(3))
    refs = [[d[:6] + [int(t) for t in rng.integers(4, V, 3)], [int(t) for t in rng.integers(4, V, 8)]] for d in decoded] * 2
    scorer = sat.CiderScorer(refs)
    idx = [7, 1, 2, 8, 4]
    out = sat.validation_step(model, images, caps, lengths, end_id=END, scorer=scorer, image_index=idx)
    assert sorted(out) == ["cider", "cider_scores", "ids", "kept", "loss"]
    assert torch.equal(out["ids"], plain["ids"]) and torch.equal(out["kept"], plain["kept"]) and torch.equal(out["loss"], plain["loss"])
    mean, scores = scorer.score(out["ids"], idx, end_id=END, kept=out["kept"])
    assert torch.equal(out["cider"], mean) and torch.equal(out["cider_scores"], scores)
    assert out["cider"].dtype == torch.float64 and tuple(out["cider"].shape) == (1,) and tuple(out["cider_scores"].shape) == (B,)
    want_mean, want = R.Corpus(refs).score(decoded, idx)
    check(out["cider"], out["cider_scores"], want_mean, want, "validation_step")
