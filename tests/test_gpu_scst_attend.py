"""GPU (MI355X): self-critical training of the Show-Attend-Tell decoder -- `sat_rollout_attend_fwd` behind
`ShowAttendTellModel.rollout` (sampled and arg-max), `SelfCritical.attend` and `ShowAttendTellModel.scst_forward`.  Draws are
replayed in float64 from the returned logits and the seed (tests/scst_reference.replay, unchanged); the rest is parity with the CPU
oracle run teacher-forced on the tokens fed (oracle.attend) and with tests/scst_reference.py / tests/cider_reference.py.

Shapes: tests/test_gpu_ss_attend.py's SMALL (P 16, C 32, E 32, H 64, V 300), 6 steps, f32."""
import functools
import importlib

import numpy as np
import pytest
import torch

import cider_reference as CR
import scst_attend_reference as SA
import scst_reference as S

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import attend as OA  # noqa: E402

P, C, E, H, V = (SA.SMALL[k] for k in "PCEHV")
STEPS, START, END = SA.STEPS, SA.START, SA.END


def make_model(seed=0):
    params = SA.params(OA, seed)
    model = sat.ShowAttendTellModel(H, C, V, E, None, feature_size=(P, C), compute_dtype="f32", vgg_cfg=[8, "M", C])
    model.load_state_dict(params, strict=False)
    return model.cuda().train(), params


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def decoder_grads(model, f=None):
    out = {k: p.grad.detach().clone() for k, p in model.named_parameters() if k in sat.attend.PARAM_ORDER}
    assert set(out) == set(sat.attend.PARAM_ORDER)
    if f is not None:
        out["features"] = f.grad.detach().clone()
    return out


# ---- 1, 2: the sampled rollout ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rollout_case(case):
    B, rank, steps, ms = case
    model, params = make_model()
    feats = SA.features(B)
    model.ss_rank = rank
    model.ss_prob, model.alpha_c = 0.5, 1.0                   # neither acts on a rollout
    fd = feats.cuda()
    fm = fd.mean(1)
    torch.manual_seed(ms)
    ids, logits = model.rollout(fd, fm, steps)
    assert ids.shape == (B, steps) and ids.dtype == torch.int64 and logits.shape == (steps * B, V) and logits.requires_grad
    assert model.last_attention_penalty is None and model.last_ss_inputs is None
    fed, alphas, seed = model.last_rollout_inputs, model.last_alphas, model.last_rollout_seed
    assert fed.shape == (B, steps) and fed.dtype == torch.int64 and alphas.shape == (steps * B, P) and not alphas.requires_grad
    model.ss_prob, model.alpha_c = 0, 0
    with torch.no_grad():
        tf = model.decode(fd, fm, fed, [steps] * B)            # the teacher-forced forward on the tokens fed, same process
    return dict(params=params, feats=feats, ids=ids.cpu(), logits=logits.detach().cpu(), seed=seed, fed=fed.cpu(),
                alphas=alphas.cpu(), tf_logits=tf.cpu(), tf_alphas=model.last_alphas.cpu())


@pytest.mark.parametrize("case", SA.REPLAY_CASES)
def test_every_draw_is_the_float64_gumbel_max(case):
    B, rank, steps, ms = case
    r = rollout_case(case)
    torch.manual_seed(ms)
    assert r["seed"] == sat.models.draw_ss_seed()             # the seed is torch's: `torch.manual_seed` reproduces a run
    want, margin = S.replay(r["logits"].numpy(), B, steps, V, r["seed"], rank)
    close = margin < 1e-4
    print("draws %d, near ties skipped %d, smallest gap %.3g" % (close.size, close.sum(), margin.min()))
    assert 20 * int(close.sum()) <= close.size
    got = r["ids"].numpy()
    assert got.min() >= 0 and got.max() < V
    assert np.array_equal(got[~close], want[~close]), np.argwhere(got != want)


@pytest.mark.parametrize("case", SA.REPLAY_CASES)
def test_logits_and_tapes_are_the_teacher_forced_forward_on_the_tokens_fed(case):
    B, rank, steps, ms = case
    r = rollout_case(case)
    fed, ids = r["fed"], r["ids"]
    assert (fed[:, 0] == START).all() and torch.equal(fed[:, 1:], ids[:, :-1])
    ref = OA.attend_forward(r["params"], r["feats"], fed, [steps] * B)
    e_ref = float((r["logits"] - ref).abs().max())
    e_tf = float((r["logits"] - r["tf_logits"]).abs().max())
    e_al = float((r["alphas"] - r["tf_alphas"]).abs().max())
    print("max |logits - oracle| %.3g, |logits - decode(fed)| %.3g, |alphas - decode's| %.3g" % (e_ref, e_tf, e_al))
    np.testing.assert_allclose(r["logits"].numpy(), ref.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(r["logits"].numpy(), r["tf_logits"].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(r["alphas"].numpy(), r["tf_alphas"].numpy(), rtol=0, atol=1e-6)
    # where the model looked for each sampled word: a distribution over the P positions per (step, row)
    amap = r["alphas"].view(steps, B, P)
    assert (amap >= 0).all() and float((amap.sum(2) - 1).abs().max()) < 1e-5


# ---- 3: the arg-max mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,steps", [(5, STEPS), (65, 3)])
def test_greedy_rollout_is_the_argmax_of_its_own_logits_and_draws_nothing(B, steps):
    model, params = make_model()
    feats = SA.features(B)
    fd = feats.cuda()
    fm = fd.mean(1)
    model.last_rollout_seed = "kept"
    runs = []
    for ms in (1, 2):
        torch.manual_seed(ms)
        rng = torch.get_rng_state()
        ids, logits = model.rollout(fd, fm, steps, greedy=True)
        assert torch.equal(torch.get_rng_state(), rng)                   # no seed consumed
        assert not logits.requires_grad and logits.grad_fn is None and logits.shape == (steps * B, V)
        runs.append((ids.cpu(), logits.cpu(), model.last_rollout_inputs.cpu()))
    assert model.last_rollout_seed == "kept" and model.last_attention_penalty is None
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    ids, logits, fed = runs[0]
    assert (fed[:, 0] == START).all() and torch.equal(fed[:, 1:], ids[:, :-1])
    lg = logits.numpy().astype(np.float64)
    top = np.sort(lg, 1)[:, -2:]
    gap = (top[:, 1] - top[:, 0]).reshape(steps, B).T
    want = lg.argmax(1).reshape(steps, B).T
    print("arg-maxes %d, near ties skipped %d, smallest gap %.3g" % (gap.size, (gap < 1e-4).sum(), gap.min()))
    assert 20 * int((gap < 1e-4).sum()) <= gap.size
    assert np.array_equal(ids.numpy()[gap >= 1e-4], want[gap >= 1e-4])
    ref = OA.attend_forward(params, feats, fed, [steps] * B)
    np.testing.assert_allclose(logits.numpy(), ref.numpy(), rtol=0, atol=2e-5)


# ---- 4: the backward --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def backward_case():
    """one rollout (B 5, 6 steps), mixed-sign advantages, row 0 forced to end by step 2 so that masked rows exist.  Gradients (a)
    through scst_loss, (b) through the rollout's backward fed the gradient sat_ce_rows_weighted leaves when called on its own, (c)
    through `decode` on the tokens fed, back-propagating that same gradient, and (d) as (c) with the decode going through
    `sat_ss_attend_fwd` (ss_prob below the smallest uniform, 2^-25: the teacher's token is always kept; only its logits are used)."""
    B = 5
    model, params = make_model()
    feats = SA.features(B)
    rng = np.random.Generator(np.random.PCG64(3))
    reward, baseline = torch.from_numpy(rng.random(B) * 2).cuda(), torch.from_numpy(rng.random(B) * 2).cuda()
    runs = {}
    G = fed = ids = end = None
    for how in ("loss", "direct", "decode", "decode_ss"):
        f = feats.cuda().requires_grad_(True)
        model.zero_grad()
        torch.manual_seed(77)
        if how in ("loss", "direct"):
            ids, logits = model.rollout(f, f.mean(1), STEPS)
            fed = model.last_rollout_inputs
            end = int(ids[0, 2])                                # row 0 ends at step 2 at the latest: masked rows behind it
        else:
            model.ss_prob = 1e-30 if how == "decode_ss" else 0
            logits = model.decode(f, f.mean(1), fed, [STEPS] * B)
            model.ss_prob = 0
            if how == "decode_ss":
                assert torch.equal(model.last_ss_inputs, fed)   # it ran the sampled forward, and no token was replaced
        if how == "loss":
            loss = sat.scst_loss(logits, ids, reward, baseline, end)
            loss.backward()
        else:
            if G is None:
                G = L.logits_buffer(STEPS * B, V, logits.device)
                G[:, :V].copy_(logits.detach())
                w, _, _ = sat.scst_weights(ids, reward, baseline, end)
                _, loss = sat.ce_rows_weighted(G[:, :V], ids, w, write_grad=True)
            logits.backward(gradient=G[:, :V])
        runs[how] = (logits.detach().cpu(), loss.detach().cpu().reshape(-1), decoder_grads(model, f))
    return params, feats, reward.cpu().numpy(), baseline.cpu().numpy(), ids.cpu(), fed.cpu(), end, runs


def report_bit_differences(how, runs):
    lg_a, _, ga = runs["loss"]
    lg_c, _, gc = runs[how]
    diff = {k: float((ga[k] - gc[k]).abs().max()) for k in ga if not torch.equal(bits(ga[k]), bits(gc[k]))}
    print("%s(fed): max |logits - rollout's| %.3g; gradients that differ in bits (max abs difference): %s"
          % (how, float((lg_a - lg_c).abs().max()), diff or "none"))


def test_backward_is_the_existing_backward_bit_for_bit():
    """scst_loss's backward == the rollout's backward fed the standalone kernel's gradient; and the rollout's per-step launches are
    `sat_ss_attend_fwd`'s: a decode through that call with the teacher's token always kept gives the same logits bit for bit"""
    _, _, _, _, _, _, _, runs = backward_case()
    (lg_a, loss_a, ga), (lg_b, loss_b, gb) = runs["loss"], runs["direct"]
    assert torch.equal(bits(lg_a), bits(lg_b)) and torch.equal(bits(loss_a), bits(loss_b))
    report_bit_differences("decode_ss", runs)
    assert torch.equal(bits(lg_a), bits(runs["decode_ss"][0]))
    for k in ga:
        assert ga[k].abs().max() > 0, k
        assert torch.equal(bits(ga[k]), bits(gb[k])), k


def test_gradients_are_those_of_decode_on_the_tokens_fed_bit_for_bit():
    """the teacher-forced `decode(fed)`, back-propagating the same d(logits): every tape the backward reads is the one that forward
    leaves (Z, which the loop fills step by step for the draws, is rebuilt as decode's one batched output-layer GEMM)"""
    _, _, _, _, _, _, _, runs = backward_case()
    report_bit_differences("decode", runs)
    ga, gc = runs["loss"][2], runs["decode"][2]
    for k in ga:
        assert torch.equal(bits(ga[k]), bits(gc[k])), k


def test_gradients_match_the_float64_oracle():
    params, feats, reward, baseline, ids, fed, end, runs = backward_case()
    logits, loss, got = runs["loss"]
    B = feats.shape[0]
    w, ln, _ = S.weights(ids.numpy(), reward, baseline, end)
    assert ln[0] <= 3 and (w == 0).any() and (w > 0).any() and (w < 0).any()
    q = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    fq = feats.double().clone().requires_grad_(True)
    ref_logits = OA.attend_forward(q, fq, fed, [STEPS] * B)
    _, ref_loss, dlogits = S.loss_and_grad(ref_logits.detach(), ids, w)
    ref_logits.backward(gradient=dlogits)
    # |loss - oracle| <= sum|w| * 2 * max|logit error| <= 2 * 2 * 2e-5 (advantages below 2 in magnitude, logits within 2e-5)
    assert abs(float(loss[0]) - float(ref_loss)) < 8e-5
    ref = {k: v.grad for k, v in q.items()}
    ref["features"] = fq.grad
    assert set(ref) == set(got)
    for k in sorted(ref):
        r = ref[k].numpy()
        e = np.abs(got[k].cpu().double().numpy().reshape(r.shape) - r)
        tol = 2e-7 + 2e-3 * np.abs(r)
        print("%-22s max err %.3g (worst err/tol %.3g), max |ref| %.3g" % (k, e.max(), (e / tol).max(), np.abs(r).max()))
    for k in sorted(ref):
        r = ref[k].numpy()
        np.testing.assert_allclose(got[k].cpu().double().numpy().reshape(r.shape), r, rtol=2e-3, atol=2e-7, err_msg=k)


# ---- 5: semantics -----------------------------------------------------------------------------------------------------------------
def test_equal_reward_and_baseline_give_exact_zeros():
    B = 5
    model, _ = make_model()
    f = SA.features(B).cuda().requires_grad_(True)
    ids, logits = model.rollout(f, f.mean(1), STEPS)
    r = torch.rand(B, dtype=torch.float64).cuda()
    loss = sat.scst_loss(logits, ids, r, r.clone(), END)
    loss.backward()
    assert loss.dim() == 0 and float(loss) == 0.0
    for k, g in decoder_grads(model, f).items():
        assert not g.any(), k


def tiny_corpus():
    """4 images x 2 references over ids 3..22"""
    rng = np.random.Generator(np.random.PCG64(11))
    return [[[int(t) for t in rng.integers(3, 23, rng.integers(4, 9))] for _ in range(2)] for _ in range(4)]


def test_end_at_step_zero_trains_one_row_and_scores_finite():
    """bias +60 on <end>: every id, sampled or arg-max, is <end> from step 0 on (kept = 0), len = 1, M = B"""
    B = 4
    model, _ = make_model()
    with torch.no_grad():
        model.classifier.bias[END] = 60.0
    sc = sat.SelfCritical(sat.CiderScorer(tiny_corpus()), END)
    f = SA.features(B).cuda().requires_grad_(True)
    loss = sc.attend(model, f, f.mean(1), [0, 1, 2, 3], steps=STEPS)
    loss.backward()
    assert (sc.last_ids == END).all() and (sc.last_greedy_ids == END).all()
    assert torch.isfinite(sc.last_reward).all() and torch.isfinite(sc.last_baseline).all() and np.isfinite(float(loss))
    assert all(torch.isfinite(g).all() for g in decoder_grads(model, f).values())
    w, ln, M = sat.scst_weights(sc.last_ids, torch.ones(B, dtype=torch.float64).cuda(), None, END)
    assert ln.cpu().tolist() == [1] * B and float(M.cpu()[0]) == B
    w = w.cpu().view(STEPS, B)
    assert (w[0] == np.float32(1.0 / B)).all() and not w[1:].any()


def test_a_gradient_step_lowers_the_loss():
    """p - 1e-2 g lowers the same loss: the same ids and weights, re-evaluated through `decode` on the tokens fed"""
    B = 5
    model, _ = make_model()
    rng = np.random.Generator(np.random.PCG64(9))
    reward, baseline = torch.from_numpy(rng.random(B) * 2).cuda(), torch.from_numpy(rng.random(B) * 2).cuda()
    f = SA.features(B).cuda()
    fm = f.mean(1)
    model.zero_grad()
    ids, logits = model.rollout(f, fm, STEPS)
    fed = model.last_rollout_inputs
    loss = sat.scst_loss(logits, ids, reward, baseline, END)
    loss.backward()
    w, _, _ = sat.scst_weights(ids, reward, baseline, END)

    def evaluate():
        with torch.no_grad():
            tf = model.decode(f, fm, fed, [STEPS] * B).contiguous()
        return float(sat.ce_rows_weighted(tf, ids, w, write_grad=False)[1].cpu()[0])

    before = evaluate()
    assert abs(before - float(loss)) < 4e-5           # sum|w| <= 2, the two sets of logits within 1e-5 of each other
    with torch.no_grad():
        for p in model.parameters():
            if p.grad is not None:
                p -= 1e-2 * p.grad
    after = evaluate()
    print("loss %.8f -> %.8f" % (before, after))
    assert after < before


def test_one_step_rollout():
    """steps = 1: one token from <start>'s logits, nothing fed back"""
    B = 5
    model, params = make_model()
    feats = SA.features(B)
    f = feats.cuda().requires_grad_(True)
    for greedy in (False, True):
        ids, logits = model.rollout(f, f.mean(1), 1, greedy=greedy)
        fed = model.last_rollout_inputs.cpu()
        assert ids.shape == (B, 1) and logits.shape == (B, V) and (fed == START).all() and model.last_alphas.shape == (B, P)
        ref = OA.attend_forward(params, feats, fed, [1] * B)
        np.testing.assert_allclose(logits.detach().cpu().numpy(), ref.numpy(), rtol=0, atol=2e-5)
        if greedy:
            want, margin = logits.cpu().numpy().argmax(1).reshape(B, 1), None
            assert np.array_equal(ids.cpu().numpy(), want)
        else:
            want, margin = S.replay(logits.detach().cpu().numpy(), B, 1, V, model.last_rollout_seed, 0)
            assert np.array_equal(ids.cpu().numpy()[margin >= 1e-4], want[margin >= 1e-4])
            sat.scst_loss(logits, ids, torch.ones(B).cuda(), None, END).backward()
            assert all(g.abs().max() > 0 for g in decoder_grads(model, f).values())


# ---- 6: end to end ----------------------------------------------------------------------------------------------------------------
def peaked_model():
    """the corpus' 20 tokens carry nearly all of the probability, so sampled and arg-max captions score against it"""
    model, params = make_model()
    with torch.no_grad():
        model.classifier.bias[3:23] += 8.0
    return model


def test_self_critical_attend_is_its_composition_and_scores_with_cider():
    B = 6
    refs = tiny_corpus()
    idx = [0, 1, 2, 3, 1, 0]
    model = peaked_model()
    scorer = sat.CiderScorer(refs)
    f = SA.features(B).cuda()
    fm = f.mean(1)
    sc = sat.SelfCritical(scorer, END)
    torch.manual_seed(5)
    loss = sc.attend(model, f, fm, idx)
    assert sc.last_ids.shape == (B, 20) and sc.last_reward.dtype == torch.float64 and sc.last_reward.shape == (B,)
    assert torch.equal(model.last_rollout_inputs[:, 1:], sc.last_ids[:, :-1])        # the sampled rollout's, not the baseline's
    # by hand
    torch.manual_seed(5)
    ids, logits = model.rollout(f, fm)
    greedy, _ = model.rollout(f, fm, greedy=True)
    ks, kg = sat.kept_tokens(ids, END), sat.kept_tokens(greedy, END)
    _, reward = scorer.score(ids, idx, end_id=END, kept=ks)
    _, baseline = scorer.score(greedy, idx, end_id=END, kept=kg)
    manual = sat.scst_loss(logits, ids, reward, baseline, END)
    assert torch.equal(ids, sc.last_ids) and torch.equal(greedy, sc.last_greedy_ids)
    assert torch.equal(reward, sc.last_reward) and torch.equal(baseline, sc.last_baseline)
    assert torch.equal(bits(manual), bits(loss)) and np.isfinite(float(loss))
    assert float((reward - baseline).abs().max()) > 0
    # the rewards are CIDEr of the returned ids
    corpus = CR.Corpus(refs)
    for got, rows in ((sc.last_reward, sc.last_ids), (sc.last_baseline, sc.last_greedy_ids)):
        _, want = corpus.score([CR.truncate(r, END) for r in rows.cpu().tolist()], idx)
        err = np.abs(got.cpu().numpy() - np.asarray(want)).max()
        print("max |CIDEr - restatement| = %.3g (max CIDEr %.3g)" % (err, float(got.max())))
        assert err <= 1e-9
    # the same seed reproduces ids and loss bits, another seed draws other ids
    torch.manual_seed(5)
    again = sat.SelfCritical(scorer, END)
    loss2 = again.attend(model, f, fm, idx)
    assert torch.equal(again.last_ids, ids) and torch.equal(bits(loss2), bits(loss))
    torch.manual_seed(6)
    other = sat.SelfCritical(scorer, END)
    other.attend(model, f, fm, idx)
    assert not torch.equal(other.last_ids, ids)


@pytest.mark.parametrize("finetune", [False, True])
def test_scst_forward_through_the_conv_stack(finetune):
    """64 x 64 images through the tiny conv stack (P = 32 * 32): a finite loss, gradients on every decoder parameter, and with
    finetune(True) on the conv weights too; the baseline is the arg-max rollout of the same policy, not `sample`"""
    B = 4
    idx = [0, 1, 2, 3]
    model = peaked_model()
    model.finetune(allow=finetune)
    scorer = sat.CiderScorer(tiny_corpus())
    images = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    model.zero_grad()
    torch.manual_seed(8)
    loss = model.scst_forward(images, idx, scorer, end_id=END, steps=STEPS)
    loss.backward()
    sc = model.last_scst
    assert loss.dim() == 0 and np.isfinite(float(loss)) and sc.last_ids.shape == (B, STEPS)
    assert float((sc.last_reward - sc.last_baseline).abs().max()) > 0
    for k, g in decoder_grads(model).items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
    for k, p in model.encoder.named_parameters():
        if finetune:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
            if k.endswith("weight"):
                assert p.grad.abs().max() > 0, k
        else:
            assert p.grad is None, k
    with torch.no_grad():
        feats, fmean = model._encode(images)
    greedy, _ = model.rollout(feats, fmean, STEPS, greedy=True)
    assert torch.equal(sc.last_greedy_ids, greedy)
    lagging = model.sample_features(feats, steps=STEPS)
    print("rows whose arg-max rollout differs from sample_features: %d of %d" % (int((lagging != greedy).any(1).sum()), B))
