"""GPU: BLEU-1..4 and ROUGE-L on the device (langstats.py, csrc/sat_langstats.hip) against what was recorded from the reference's
own `BleuScorer` and `Rouge` (tests/golden/langstats/G12_bleu_rouge.npz) and, on a random corpus, against the pure-Python
restatement (tests/bleu_rouge_reference.py).

Integers (comps, totals) must be equal.  The floats are compared in f64 at 1e-12 absolute on values <= 1: a sentence or corpus
BLEU is under 40 f64 operations, the loosest of them `pow` and `exp` at <= 16 ulp (the OpenCL bound the device math library is
built to), so under 40 x 16 x 1.1e-16 ~ 7e-14; ROUGE-L is a dozen IEEE operations.  The kernel does not return the LCS itself:
prec_max = lcs / len(row) with len(row) <= 64, so an LCS off by one moves a non-zero score by far more than the bound, and the
scores that are exactly 0 or 1 in the reference must be exactly that here."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bleu_rouge_reference as R  # noqa: E402
import cider_reference as CR  # noqa: E402
from test_cider_host import load_corpus  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
TOL = 1e-12
END = 2


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "langstats", "G12_bleu_rouge.npz"))


def bits(t):
    return t.contiguous().view(torch.int64)


def close(got, want, what):
    got, want = got.cpu().numpy(), np.asarray(want, dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = np.abs(got - want).max()
    print("%s: max |device - want| = %.3g" % (what, err))
    assert err <= TOL, what
    return err


def rows_matrix(hyps, T, terminate, stride_pad=0):
    """hyps as int64 [B, T] rows of a wider device matrix (stride T + stride_pad): the tokens, then END (when it fits and
    `terminate`), then junk ids"""
    wide = torch.full((len(hyps), T + stride_pad), 7, dtype=torch.int64)
    off = stride_pad // 2
    for b, h in enumerate(hyps):
        wide[b, off:off + len(h)] = torch.tensor(h, dtype=torch.int64)
        if terminate and len(h) < T:
            wide[b, off + len(h)] = END
    return wide.cuda()[:, off:off + T]


@pytest.mark.parametrize("c", ["small", "wide", "one", "edges"])
def test_golden_corpora(golden, c):
    refs, hyps = load_corpus(golden, c)
    idx = list(range(len(refs)))
    T = max(len(h) for h in hyps)
    ids = rows_matrix(hyps, T, terminate=False)               # the small corpus's ids include 2: the lengths come through `kept`
    kept = torch.tensor([len(h) for h in hyps], dtype=torch.int32).cuda()
    bleu = sat.BleuScorer(refs)
    want_list = golden[c + "_bleu_list"].T
    for order in (1, 2, 3, 4):
        mean, scores = bleu.score(ids, idx, end_id=END, kept=kept, order=order)
        assert tuple(mean.shape) == (1,) and mean.dtype == torch.float64
        close(scores, want_list[:, order - 1], "%s Bleu_%d per image" % (c, order))
        close(mean, [want_list[:, order - 1].mean()], "%s Bleu_%d batch mean" % (c, order))
    assert np.array_equal(bleu.last_comps.cpu().numpy(), golden[c + "_comps"]) and bleu.last_comps.dtype == torch.int64
    close(bleu.last_sentence, want_list, c + " bleu_list")
    assert not bleu.totals.cpu().numpy().any()                # `score` leaves the totals alone
    sentence = bleu.update(ids, idx, end_id=END, kept=kept)
    assert torch.equal(bits(sentence), bits(bleu.last_sentence))
    assert np.array_equal(bleu.totals.cpu().numpy(), golden[c + "_comps"].sum(axis=0))
    close(bleu.compute(), golden[c + "_bleus"], c + " corpus Bleu_1..4")
    mean, scores = sat.RougeLScorer(refs).score(ids, idx, end_id=END, kept=kept)
    want = golden[c + "_rouge_scores"]
    close(scores, want, c + " ROUGE_L per image")
    close(mean, [float(golden[c + "_rouge_mean"])], c + " ROUGE_L mean")
    exact = (want == 0.0) | (want == 1.0)
    assert np.array_equal(scores.cpu().numpy()[exact], want[exact])
    if c == "edges":
        assert (want == 1.0).sum() >= 2 and (want == 0.0).sum() >= 2


@pytest.fixture(scope="module")
def random_corpus():
    """30 images of 1-6 references over 8 symbols (clipping and repeats occur; a few references are empty), on the device thrice"""
    rng = np.random.Generator(np.random.PCG64(1212))
    refs = [[[int(t) for t in rng.integers(3, 11, rng.integers(0, 13))] for _ in range(rng.integers(1, 7))] for _ in range(30)]
    refs[3][0] = []
    refs[7] = [[], [4, 5]]
    cider = sat.CiderScorer(refs)
    return refs, cider, sat.BleuScorer(refs), sat.RougeLScorer(refs)


def draw_rows(rng, refs, B, T):
    """image indices (one comes twice) and hypotheses of 0..T tokens: stretches of a reference, random ids, ids no corpus has
    and ids outside [0, 2^31)"""
    idx = [int(i) for i in rng.integers(0, len(refs), B)]
    if B > 2:
        idx[0], idx[1], idx[2] = 7, 3, 7
    lengths = [T, 0, T // 2 + 1] + [int(n) for n in rng.integers(0, T + 1, B)]
    hyps = []
    for b in range(B):
        n = min(lengths[b], T)
        src = [t for r in refs[idx[b]] for t in r]
        if b % 3 == 0 and src:
            h = (src * (n // len(src) + 1))[:n]
        else:
            h = [int(t) for t in rng.integers(3, 11, n)]
        if b % 5 == 4 and n > 2:
            h[1], h[n - 1] = 2 ** 31 + 4, -9                   # outside [0, 2^31): equal to no reference token, counted in lengths
        if b % 7 == 6 and n > 1:
            h[0] = 500                                        # in range, in no reference
        hyps.append(h)
    return idx, hyps


@pytest.mark.parametrize("T", [1, 20, 64])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_random_corpus_vs_restatement(random_corpus, B, T):
    refs, _, bleu, rouge = random_corpus
    idx, hyps = draw_rows(np.random.Generator(np.random.PCG64(100 * B + T)), refs, B, T)
    ids = rows_matrix(hyps, T, terminate=True, stride_pad=11)
    assert ids.stride(0) == T + 11 and ids.stride(1) == 1
    comps, sentence, _, _ = R.bleu(hyps, refs, idx)
    mean, scores = bleu.score(ids, idx, end_id=END)
    assert np.array_equal(bleu.last_comps.cpu().numpy(), np.asarray(comps, dtype=np.int64))
    close(bleu.last_sentence, sentence, "B %d T %d bleu_list" % (B, T))
    close(scores, [s[3] for s in sentence], "B %d T %d Bleu_4" % (B, T))
    close(mean, [np.mean([s[3] for s in sentence])], "B %d T %d Bleu_4 mean" % (B, T))
    want_mean, want = R.rouge_l(hyps, refs, idx)
    r_mean, r_scores = rouge.score(ids, idx, end_id=END)
    close(r_scores, want, "B %d T %d ROUGE_L" % (B, T))
    close(r_mean, [want_mean], "B %d T %d ROUGE_L mean" % (B, T))
    # the row ends given as `kept` are the ends found at END: the same bits
    kept = sat.kept_tokens(ids.contiguous(), END)
    assert kept.cpu().tolist() == [len(h) for h in hyps]
    index = torch.tensor(idx, dtype=torch.int32).cuda()
    mean_k, scores_k = bleu.score(ids, index, end_id=END, kept=kept)
    assert torch.equal(bits(scores_k), bits(scores)) and torch.equal(bits(mean_k), bits(mean))
    assert np.array_equal(bleu.last_comps.cpu().numpy(), np.asarray(comps, dtype=np.int64))
    rk_mean, rk_scores = rouge.score(ids, index, end_id=END, kept=kept)
    assert torch.equal(bits(rk_scores), bits(r_scores)) and torch.equal(bits(rk_mean), bits(r_mean))


def test_update_over_two_batches_is_one_update_of_both(random_corpus):
    refs, _, bleu, _ = random_corpus
    idx, hyps = draw_rows(np.random.Generator(np.random.PCG64(77)), refs, 40, 20)
    ids = rows_matrix(hyps, 20, terminate=True)
    _, _, totals, corpus = R.bleu(hyps, refs, idx)
    whole = sat.BleuScorer.from_scorer(bleu)
    s_all = whole.update(ids, idx, end_id=END)
    halves = sat.BleuScorer.from_scorer(bleu)
    s_a = halves.update(ids[:17], idx[:17], end_id=END)
    s_b = halves.update(ids[17:], idx[17:], end_id=END)
    assert torch.equal(bits(torch.cat([s_a, s_b])), bits(s_all))
    assert whole.totals.cpu().tolist() == totals == halves.totals.cpu().tolist()
    assert torch.equal(bits(whole.compute()), bits(halves.compute()))
    close(whole.compute(), corpus, "corpus Bleu_1..4 of 40 rows")
    assert not bleu.totals.cpu().numpy().any()                # from_scorer shares the corpus, not the totals
    halves.reset()
    assert not halves.totals.cpu().numpy().any()
    halves.update(ids[:17], idx[:17], end_id=END)
    close(halves.compute(), R.bleu(hyps[:17], refs, idx[:17])[3], "after reset")


def test_two_calls_and_a_shared_corpus_give_the_same_bits(random_corpus):
    refs, cider, bleu, rouge = random_corpus
    idx, hyps = draw_rows(np.random.Generator(np.random.PCG64(5)), refs, 37, 64)
    ids = rows_matrix(hyps, 64, terminate=True)
    a, b = bleu.score(ids, idx), bleu.score(ids, idx)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    ra, rb = rouge.score(ids, idx), rouge.score(ids, idx)
    assert torch.equal(bits(ra[0]), bits(rb[0])) and torch.equal(bits(ra[1]), bits(rb[1]))
    shared_b, shared_r = sat.BleuScorer.from_scorer(cider), sat.RougeLScorer.from_scorer(cider)
    assert shared_b.ref_tokens.data_ptr() == cider.ref_tokens.data_ptr() == shared_r.ref_tokens.data_ptr()
    c = shared_b.score(ids, idx)
    assert torch.equal(bits(a[0]), bits(c[0])) and torch.equal(bits(a[1]), bits(c[1]))
    assert torch.equal(shared_b.last_comps, bleu.last_comps) and torch.equal(bits(shared_b.last_sentence), bits(bleu.last_sentence))
    rc = shared_r.score(ids, idx)
    assert torch.equal(bits(ra[0]), bits(rc[0])) and torch.equal(bits(ra[1]), bits(rc[1]))
    other = sat.RougeLScorer.from_scorer(bleu, beta=2.0).score(ids, idx)[1]         # beta reaches the kernel
    close(other, R.rouge_l(hyps, refs, idx, beta=2.0)[1], "beta 2")
    assert not torch.equal(bits(other), bits(ra[1]))


def test_validation_step_returns_bleu_and_rouge_of_its_own_ids():
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
    decoded = [CR.truncate(r, END) for r in plain["ids"].cpu().tolist()]
    rng = np.random.Generator(np.random.PCG64(3))
    refs = [[d[:6] + [int(t) for t in rng.integers(4, V, 3)], [int(t) for t in rng.integers(4, V, 8)]] for d in decoded] * 2
    scorer = sat.CiderScorer(refs)
    bleu, rouge = sat.BleuScorer.from_scorer(scorer), sat.RougeLScorer.from_scorer(scorer)
    idx = [7, 1, 2, 8, 4]
    old = sat.validation_step(model, images, caps, lengths, end_id=END, scorer=scorer, image_index=idx)
    out = sat.validation_step(model, images, caps, lengths, end_id=END, scorer=scorer, image_index=idx, bleu=bleu, rouge=rouge)
    assert sorted(out) == ["bleu_scores", "cider", "cider_scores", "ids", "kept", "loss", "rouge_l", "rouge_l_scores"]
    assert sorted(old) == ["cider", "cider_scores", "ids", "kept", "loss"]
    for k in ("ids", "kept", "loss"):
        assert torch.equal(out[k], plain[k]) and torch.equal(old[k], plain[k])
    for k in ("cider", "cider_scores"):
        assert torch.equal(bits(out[k]), bits(old[k]))
    assert tuple(out["bleu_scores"].shape) == (B, 4) and tuple(out["rouge_l"].shape) == (1,) and tuple(out["rouge_l_scores"].shape) == (B,)
    assert all(out[k].dtype == torch.float64 for k in ("bleu_scores", "rouge_l", "rouge_l_scores"))
    direct = sat.BleuScorer.from_scorer(scorer)
    assert torch.equal(bits(direct.update(out["ids"], idx, end_id=END, kept=out["kept"])), bits(out["bleu_scores"]))
    assert torch.equal(direct.totals, bleu.totals) and bleu.totals[0].item() == sum(len(d) for d in decoded)
    mean, scores = rouge.score(out["ids"], idx, end_id=END, kept=out["kept"])
    assert torch.equal(bits(out["rouge_l"]), bits(mean)) and torch.equal(bits(out["rouge_l_scores"]), bits(scores))
    close(out["bleu_scores"], R.bleu(decoded, refs, idx)[1], "validation_step bleu_list")
    close(out["rouge_l_scores"], R.rouge_l(decoded, refs, idx)[1], "validation_step ROUGE_L")
    only = sat.validation_step(model, images, caps, lengths, end_id=END, image_index=idx, rouge=rouge)       # without a CiderScorer
    assert sorted(only) == ["ids", "kept", "loss", "rouge_l", "rouge_l_scores"]
    assert torch.equal(bits(only["rouge_l_scores"]), bits(scores))


def test_self_critical_with_a_mixed_cider_and_bleu_reward():
    import scst_reference as S
    from oracle import decoder as OD
    B, V, Lh = 4, 24, 1
    rng = np.random.Generator(np.random.PCG64(11))
    refs = [[[int(t) for t in rng.integers(3, 23, rng.integers(4, 9))] for _ in range(2)] for _ in range(4)]
    idx = [0, 1, 2, 3]
    params, feats = S.replay_inputs(OD, Lh, B, V)
    dec = sat.DecoderRNN(S.REPLAY_E, S.REPLAY_H, V, Lh)
    dec.load_state_dict(params)
    dec.cuda().train()
    cider = sat.CiderScorer(refs)
    bleu = sat.BleuScorer.from_scorer(cider)
    sc = sat.SelfCritical(sat.MixedReward([(cider, 1.0), (bleu, 0.5)]), END)
    f = feats.cuda().requires_grad_(True)
    torch.manual_seed(5)
    loss = sc(dec, f, idx)
    loss.backward()
    assert np.isfinite(float(loss)) and torch.isfinite(f.grad).all()
    assert all(torch.isfinite(p.grad).all() for p in dec.parameters() if p.grad is not None)
    for got, rows in ((sc.last_reward, sc.last_ids), (sc.last_baseline, sc.last_greedy_ids)):
        kept = sat.kept_tokens(rows, END)
        want = cider.score(rows, idx, end_id=END, kept=kept)[1] + 0.5 * bleu.score(rows, idx, end_id=END, kept=kept, order=4)[1]
        assert got.dtype == torch.float64 and tuple(got.shape) == (B,) and torch.equal(bits(got), bits(want))
        hyps = [CR.truncate(r, END) for r in rows.cpu().tolist()]
        b4 = [s[3] for s in R.bleu(hyps, refs, idx)[1]]
        ref = np.asarray(CR.Corpus(refs).score(hyps, idx)[1]) + 0.5 * np.asarray(b4)
        err = np.abs(got.cpu().numpy() - ref).max()
        print("max |mixed reward - restatements| = %.3g" % err)
        assert err <= 1e-9                                    # CIDEr's bound (tests/test_gpu_cider.py); the BLEU half is within 1e-12
    assert not bleu.totals.cpu().numpy().any()                # a reward does not accumulate a corpus score
