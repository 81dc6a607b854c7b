"""GPU (MI355X): self-critical sequence training -- the sampled rollout (`sat_rollout_decoder_fwd`), the reward weights
(`sat_scst_weights`), the weighted cross entropy (`sat_ce_rows_weighted`), `scst_loss` / `SelfCritical` and `TrainStep.scst_step`.
Draws are replayed in float64 from the returned logits and the seed; the rest is parity with the CPU oracle run teacher-forced on
the tokens drawn and with tests/scst_reference.py.

Oracle parity of the gradients (test_gradients_match_the_oracle) is asserted at the existing bound, rtol 1e-3 / atol 1e-7; the test
prints, per tensor, its error and the teacher-forced path's error against the same oracle gradient."""
import functools
import importlib

import numpy as np
import pytest
import torch

import cider_reference as CR
import scst_reference as S

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import decoder as OD  # noqa: E402

TINY = dict(layers=(1, 1, 1, 1), width=8)
END = 2
E, H, STEPS = S.REPLAY_E, S.REPLAY_H, S.REPLAY_STEPS


def decoder_of(params, V, Lh):
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    return dec.cuda().train()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- 1, 2: the rollout ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rollout_case(case):
    Lh, rank, B, V, ms = case
    params, feats = S.replay_inputs(OD, Lh, B, V)
    dec = decoder_of(params, V, Lh)
    dec.ss_rank = rank
    torch.manual_seed(ms)
    ids, logits = dec.rollout(feats.cuda(), STEPS)
    assert ids.shape == (B, STEPS) and ids.dtype == torch.int64 and logits.shape == (STEPS * B, V) and logits.requires_grad
    return params, feats, ids.cpu(), logits.detach().cpu(), dec.last_rollout_seed


@pytest.mark.parametrize("case", S.REPLAY_CASES)
def test_every_draw_is_the_float64_gumbel_max(case):
    Lh, rank, B, V, ms = case
    _, _, ids, logits, seed = rollout_case(case)
    torch.manual_seed(ms)
    assert seed == sat.models.draw_ss_seed()                  # the seed is torch's: `torch.manual_seed` reproduces a run
    want, margin = S.replay(logits.numpy(), B, STEPS, V, seed, rank)
    close = margin < 1e-4
    print("draws %d, near ties skipped %d, smallest gap %.3g" % (close.size, close.sum(), margin.min()))
    assert 20 * int(close.sum()) <= close.size
    got = ids.numpy()
    assert got.min() >= 0 and got.max() < V
    assert np.array_equal(got[~close], want[~close]), np.argwhere(got != want)


@pytest.mark.parametrize("case", S.REPLAY_CASES)
def test_logits_are_the_teacher_forced_forward_on_the_drawn_tokens(case):
    Lh, rank, B, V, ms = case
    params, feats, ids, logits, _ = rollout_case(case)
    ref = OD.decoder_forward(params, feats, ids[:, :STEPS - 1], [STEPS] * B, Lh)
    err = float((logits - ref).abs().max())
    print("max |logits - oracle| = %.3g" % err)
    np.testing.assert_allclose(logits.numpy(), ref.numpy(), rtol=0, atol=1e-5)


def test_one_step_rollout():
    """steps = 1: one draw from the features' logits, nothing fed back"""
    params, feats = S.replay_inputs(OD, 1, 5, 203)
    dec = decoder_of(params, 203, 1)
    ids, logits = dec.rollout(feats.cuda(), 1)
    ref = OD.decoder_forward(params, feats, torch.zeros(5, 0, dtype=torch.int64), [1] * 5, 1)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref.numpy(), rtol=0, atol=1e-5)
    want, margin = S.replay(logits.detach().cpu().numpy(), 5, 1, 203, dec.last_rollout_seed, 0)
    assert np.array_equal(ids.cpu().numpy()[margin >= 1e-4], want[margin >= 1e-4])


# ---- 3: sat_scst_weights -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(7, 5), (300, 3), (1, 20)])
@pytest.mark.parametrize("with_baseline,with_denom,f32", [(True, False, False), (False, False, True), (True, True, False)])
def test_scst_weights_bit_exact(B, T, with_baseline, with_denom, f32):
    rng = np.random.Generator(np.random.PCG64(B * 100 + T))
    ids = rng.integers(3, 9, (B, T))
    for b in range(B):                       # <end> at every position in turn, at column 0, twice in a row, and not at all
        if b % (T + 1) < T:
            ids[b, b % (T + 1)] = END
        if b % 5 == 0:
            ids[b, T - 1] = END
    reward, baseline = rng.random(B) * 3, rng.random(B) * 3
    if f32:
        reward = reward.astype(np.float32)
    denom = 1234.0 if with_denom else None
    w, ln, M = sat.scst_weights(torch.from_numpy(ids).cuda(), torch.from_numpy(reward).cuda(),
                                torch.from_numpy(baseline).cuda() if with_baseline else None, END,
                                torch.tensor([denom], dtype=torch.float64).cuda() if with_denom else None)
    w_ref, ln_ref, M_ref = S.weights(ids, reward, baseline if with_baseline else None, END, denom)
    assert w.dtype == torch.float32 and ln.dtype == torch.int32 and M.dtype == torch.float64
    assert np.array_equal(ln.cpu().numpy(), ln_ref) and float(M.cpu()[0]) == float(M_ref)
    assert np.array_equal(w.cpu().numpy().view(np.int32), w_ref.view(np.int32))


# ---- 4: sat_ce_rows_weighted ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(13, 1), (1, 13)])
@pytest.mark.parametrize("ldl", [204, 203])          # 204: rows of whole 16-byte chunks (the register path); 203: the strided path
def test_ce_rows_weighted(B, T, ldl):
    N, V = 13, 203
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, V, generator=g) * 3
    ids = torch.randint(0, V, (B, T), generator=g)
    w = torch.randn(N, generator=g)                    # mixed signs
    w[[2, 7, 12]] = 0.0
    w[7] = -0.0
    x[7, 100] = float("inf")                           # a dead row's non-finite logit must stay out of loss and gradient
    buf = torch.full((N, ldl), 7.0)
    buf[:, :V] = x
    d1, d2 = buf.cuda(), buf.cuda()
    row_loss, loss = sat.ce_rows_weighted(d1[:, :V], ids.cuda(), w.cuda(), write_grad=True)
    row_loss2, loss2 = sat.ce_rows_weighted(d2[:, :V], ids.cuda(), w.cuda(), write_grad=True)
    assert torch.equal(bits(d1), bits(d2)) and torch.equal(bits(loss), bits(loss2))        # two calls, the same bits
    live = (w != 0).numpy()
    assert torch.equal(bits(row_loss)[torch.from_numpy(live)], bits(row_loss2)[torch.from_numpy(live)])
    ref_rows, ref_loss, ref_grad = S.loss_and_grad(x, ids, w.numpy())
    got = d1.cpu()
    if ldl > V:
        assert (got[:, V:] == 7.0).all()                                                     # pad column untouched
    assert not got[~torch.from_numpy(live), :V].any()                                        # dead rows: exactly zero
    scale = float((w.double() * ref_rows).abs().sum())
    err_l = abs(float(loss.cpu()[0]) - float(ref_loss))
    err_g = float((got[:, :V].double() - ref_grad).abs().max())
    err_r = float((row_loss.cpu().double() - ref_rows)[torch.from_numpy(live)].abs().max())
    print("loss err %.3g (bound %.3g), grad err %.3g (bound %.3g), row-loss err %.3g"
          % (err_l, 1e-6 * scale + 1e-7, err_g, 2e-8 + 1e-6 * float(w.abs().max()), err_r))
    assert np.isfinite(float(loss.cpu()[0])) and err_l <= 1e-6 * scale + 1e-7
    assert err_g <= 2e-8 + 1e-6 * float(w.abs().max())
    # no gradient asked for: the logits stay, the loss is the same
    d3 = buf.cuda()
    _, loss3 = sat.ce_rows_weighted(d3[:, :V], ids.cuda(), w.cuda(), write_grad=False)
    assert torch.equal(bits(d3), bits(buf.cuda())) and torch.equal(bits(loss3), bits(loss))


# ---- 5, 6: the backward --------------------------------------------------------------------------------------------------------
def grads_of(dec, f):
    out = {k: p.grad.detach().clone() for k, p in dec.named_parameters()}
    out["features"] = f.grad.detach().clone()
    return out


@functools.lru_cache(maxsize=None)
def backward_case(Lh):
    """one rollout (B 5, V 203, 6 steps), mixed-sign advantages: gradients through scst_loss, and through the rollout's own
    backward fed the gradient sat_ce_rows_weighted leaves when called on its own"""
    B, V = 5, 203
    params, feats = S.replay_inputs(OD, Lh, B, V)
    dec = decoder_of(params, V, Lh)
    rng = np.random.Generator(np.random.PCG64(3))
    reward, baseline = torch.from_numpy(rng.random(B) * 2).cuda(), torch.from_numpy(rng.random(B) * 2).cuda()
    runs = []
    for via_loss in (True, False):
        f = feats.cuda().requires_grad_(True)
        dec.zero_grad()
        torch.manual_seed(77)
        ids, logits = dec.rollout(f, STEPS)
        end = int(ids[0, 2])                                  # row 0 ends at step 2 at the latest: masked rows behind it
        if via_loss:
            loss = sat.scst_loss(logits, ids, reward, baseline, end)
            loss.backward()
        else:
            G = L.logits_buffer(STEPS * B, V, logits.device)
            G[:, :V].copy_(logits.detach())
            w, _, _ = sat.scst_weights(ids, reward, baseline, end)
            _, loss = sat.ce_rows_weighted(G[:, :V], ids, w, write_grad=True)
            logits.backward(gradient=G[:, :V])
        runs.append((ids.cpu(), logits.detach().cpu(), loss.detach().cpu().reshape(-1), grads_of(dec, f)))
    return params, feats, reward.cpu().numpy(), baseline.cpu().numpy(), runs, dec, end


@pytest.mark.parametrize("Lh", [1, 2])
def test_backward_is_the_existing_backward_bit_for_bit(Lh):
    _, _, _, _, runs, _, _ = backward_case(Lh)
    (ids_a, lg_a, loss_a, ga), (ids_b, lg_b, loss_b, gb) = runs
    assert torch.equal(ids_a, ids_b) and torch.equal(bits(lg_a), bits(lg_b)) and torch.equal(bits(loss_a), bits(loss_b))
    for k in ga:
        assert torch.equal(bits(ga[k]), bits(gb[k])), k
        assert ga[k].abs().max() > 0, k


@pytest.mark.parametrize("Lh", [1, 2])
def test_gradients_match_the_oracle(Lh):
    params, feats, reward, baseline, runs, dec, end = backward_case(Lh)
    ids, logits, loss, got = runs[0]
    B = feats.shape[0]
    w, ln, _ = S.weights(ids.numpy(), reward, baseline, end)
    assert ln[0] <= 3 and (w == 0).any() and (w > 0).any() and (w < 0).any()
    fed = ids[:, :STEPS - 1]
    ref_logits, tape = OD.decoder_forward(params, feats, fed, [STEPS] * B, Lh, keep=True)
    _, ref_loss, dlogits = S.loss_and_grad(ref_logits, ids, w)
    # |loss - oracle| <= sum|w| * 2 * max|logit error| <= 2 * 2 * 1e-5 (advantages below 2 in magnitude, logits within 1e-5)
    assert abs(float(loss[0]) - float(ref_loss)) < 4e-5
    grads, d_feat = OD.decoder_backward(params, tape, fed, [STEPS] * B, dlogits.float(), Lh)
    grads["features"] = d_feat
    # the existing path's error against the same oracle, for comparison (printed only): teacher-forced on the same tokens
    f = feats.cuda().requires_grad_(True)
    dec.zero_grad()
    dec(f, fed.cuda(), [STEPS] * B).backward(gradient=dlogits.float().cuda())
    old = grads_of(dec, f)
    for k in sorted(grads):
        ref = grads[k].numpy()
        e_new = np.abs(got[k].cpu().numpy() - ref)
        e_old = np.abs(old[k].cpu().numpy() - ref)
        tol = 1e-7 + 1e-3 * np.abs(ref)
        print("%-22s scst max err %.3g (worst err/tol %.3g) | teacher-forced path max err %.3g (worst err/tol %.3g)"
              % (k, e_new.max(), (e_new / tol).max(), e_old.max(), (e_old / tol).max()))
    for k in sorted(grads):
        np.testing.assert_allclose(got[k].cpu().numpy(), grads[k].numpy(), rtol=1e-3, atol=1e-7, err_msg=k)


# ---- 7: semantics --------------------------------------------------------------------------------------------------------------
def test_equal_reward_and_baseline_give_exact_zeros():
    B, V = 5, 203
    params, feats = S.replay_inputs(OD, 2, B, V)
    dec = decoder_of(params, V, 2)
    f = feats.cuda().requires_grad_(True)
    ids, logits = dec.rollout(f, STEPS)
    r = torch.rand(B, dtype=torch.float64).cuda()
    loss = sat.scst_loss(logits, ids, r, r.clone(), END)
    loss.backward()
    assert loss.dim() == 0 and float(loss) == 0.0
    for k, g in grads_of(dec, f).items():
        assert not g.any(), k


def tiny_corpus():
    """4 images x 2 references over ids 3..22"""
    rng = np.random.Generator(np.random.PCG64(11))
    return [[[int(t) for t in rng.integers(3, 23, rng.integers(4, 9))] for _ in range(2)] for _ in range(4)]


def test_end_at_step_zero_trains_one_row_and_scores_finite():
    """bias +60 on <end>: every sampled row is <end> from step 0 on (kept = 0), len = 1, M = B, only step 0's rows carry weight"""
    B, V = 4, 24
    params, feats = S.replay_inputs(OD, 1, B, V)
    dec = decoder_of(params, V, 1)
    with torch.no_grad():
        dec.linear.bias[END] = 60.0
    refs = tiny_corpus()
    sc = sat.SelfCritical(sat.CiderScorer(refs), END)
    f = feats.cuda().requires_grad_(True)
    loss = sc(dec, f, [0, 1, 2, 3], steps=STEPS)
    loss.backward()
    assert (sc.last_ids == END).all()
    assert torch.isfinite(sc.last_reward).all() and torch.isfinite(sc.last_baseline).all() and np.isfinite(float(loss))
    assert all(torch.isfinite(g).all() for g in grads_of(dec, f).values())
    w, ln, M = sat.scst_weights(sc.last_ids, torch.ones(B, dtype=torch.float64).cuda(), None, END)
    assert ln.cpu().tolist() == [1] * B and float(M.cpu()[0]) == B
    w = w.cpu().view(STEPS, B)
    assert (w[0] == np.float32(1.0 / B)).all() and not w[1:].any()


def test_a_gradient_step_lowers_the_loss():
    """p - 1e-2 g lowers the same loss: the same ids and weights, re-evaluated teacher-forced on the ids"""
    B, V, Lh = 5, 203, 2
    params, feats = S.replay_inputs(OD, Lh, B, V)
    dec = decoder_of(params, V, Lh)
    rng = np.random.Generator(np.random.PCG64(9))
    reward, baseline = torch.from_numpy(rng.random(B) * 2).cuda(), torch.from_numpy(rng.random(B) * 2).cuda()
    f = feats.cuda()
    dec.zero_grad()
    ids, logits = dec.rollout(f, STEPS)
    loss = sat.scst_loss(logits, ids, reward, baseline, END)
    loss.backward()
    w, _, _ = sat.scst_weights(ids, reward, baseline, END)

    def evaluate():
        with torch.no_grad():
            tf = dec(f, ids[:, :STEPS - 1].contiguous(), [STEPS] * B).contiguous()
        return float(sat.ce_rows_weighted(tf, ids, w, write_grad=False)[1].cpu()[0])

    before = evaluate()
    assert abs(before - float(loss)) < 4e-5           # sum|w| <= 2, both sets of logits within 1e-5 of the oracle's
    with torch.no_grad():
        for p in dec.parameters():
            p -= 1e-2 * p.grad
    after = evaluate()
    print("loss %.8f -> %.8f" % (before, after))
    assert after < before


# ---- 8: end to end -------------------------------------------------------------------------------------------------------------
def test_self_critical_is_its_composition_and_scores_with_cider():
    B, V, Lh = 6, 24, 1
    refs = tiny_corpus()
    idx = [0, 1, 2, 3, 1, 0]
    params, feats = S.replay_inputs(OD, Lh, B, V)
    dec = decoder_of(params, V, Lh)
    scorer = sat.CiderScorer(refs)
    f = feats.cuda()
    sc = sat.SelfCritical(scorer, END)
    torch.manual_seed(5)
    loss = sc(dec, f, idx)
    assert sc.last_ids.shape == (B, 20) and sc.last_reward.dtype == torch.float64 and sc.last_reward.shape == (B,)
    # by hand, in SelfCritical's order
    torch.manual_seed(5)
    ids, logits = dec.rollout(f)
    greedy = dec.sample(f)
    ks, kg = sat.kept_tokens(ids, END), sat.kept_tokens(greedy, END)
    _, reward = scorer.score(ids, idx, end_id=END, kept=ks)
    _, baseline = scorer.score(greedy, idx, end_id=END, kept=kg)
    manual = sat.scst_loss(logits, ids, reward, baseline, END)
    assert torch.equal(ids, sc.last_ids) and torch.equal(greedy, sc.last_greedy_ids)
    assert torch.equal(reward, sc.last_reward) and torch.equal(baseline, sc.last_baseline)
    assert torch.equal(bits(manual), bits(loss)) and np.isfinite(float(loss))
    # the rewards are CIDEr of the returned ids
    corpus = CR.Corpus(refs)
    for got, rows in ((sc.last_reward, sc.last_ids), (sc.last_baseline, sc.last_greedy_ids)):
        _, want = corpus.score([CR.truncate(r, END) for r in rows.cpu().tolist()], idx)
        err = np.abs(got.cpu().numpy() - np.asarray(want)).max()
        print("max |CIDEr - restatement| = %.3g" % err)
        assert err <= 1e-9
    # the same seed reproduces ids and loss bits, another seed draws other ids
    torch.manual_seed(5)
    again = sat.SelfCritical(scorer, END)
    loss2 = again(dec, f, idx)
    assert torch.equal(again.last_ids, ids) and torch.equal(bits(loss2), bits(loss))
    torch.manual_seed(6)
    other = sat.SelfCritical(scorer, END)
    other(dec, f, idx)
    assert not torch.equal(other.last_ids, ids)


# ---- 9: the fused step ---------------------------------------------------------------------------------------------------------
def ts_model(V, Lh, dtype):
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY, compute_dtype=dtype)
    model.decoder.load_state_dict(OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(4)))
    return model.cuda().train()


@pytest.mark.parametrize("Lh", [1, 2])
def test_scst_step_equals_the_autograd_path(Lh):
    B, V = 6, 24
    idx = [0, 1, 2, 3, 1, 0]
    scorer = sat.CiderScorer(tiny_corpus())
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(2)).cuda()
    ma, mb = ts_model(V, Lh, "f32"), ts_model(V, Lh, "f32")
    opt = sat.FusedClampAdam(ma.decoder.parameters(), lr=1e-3, clip=0.1)
    ts = sat.TrainStep(mb, lr=1e-3, grad_clip=0.1)
    opt.zero_grad()
    torch.manual_seed(21)
    sc = sat.SelfCritical(scorer, END)
    loss_a = sc(ma.decoder, feats, idx)
    loss_a.backward()
    grads_a = {k: p.grad.detach().clone() for k, p in ma.decoder.named_parameters()}
    opt.step()
    torch.manual_seed(21)
    loss_b = ts.scst_step(feats, idx, scorer)
    assert torch.equal(ts.last_scst.last_ids, sc.last_ids) and torch.equal(ts.last_scst.last_reward, sc.last_reward)
    assert torch.equal(ts.last_scst.last_baseline, sc.last_baseline)
    assert loss_b.shape == (1,) and torch.equal(bits(loss_b), bits(loss_a.reshape(1)))
    slot = ts.flat.grads[ts.flat.loss_slot:ts.flat.loss_slot + 1]
    assert torch.equal(bits(slot), bits(loss_a.reshape(1)))
    for k, p in mb.decoder.named_parameters():          # (value equality: the autograd path accumulates into a zeroed buffer, 0 + -0 = +0)
        assert torch.equal(ts.flat.grad("decoder." + k), grads_a[k]), k
        assert grads_a[k].abs().max() > 0, k
    for (k, pa), (_, pb) in zip(ma.decoder.named_parameters(), mb.decoder.named_parameters()):
        assert torch.equal(pa, pb), k
    assert float(ts.fault_slot.cpu()[0]) == 0.0


def test_scst_step_bf16_mode_through_the_encoder():
    """compute_dtype bf16, images through the tiny encoder: the step runs (its decoder arithmetic stays exact f32), the loss is
    finite, the head and the decoder move"""
    B, V = 4, 24
    model = ts_model(V, 1, "bf16")
    ts = sat.TrainStep(model)
    images = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    before = ts.flat.params.clone()
    loss = ts.scst_step(images, [0, 1, 2, 3], sat.CiderScorer(tiny_corpus()))
    ts.check_ids()
    assert np.isfinite(float(loss.cpu()[0]))
    assert torch.isfinite(ts.flat.grads).all()
    assert not torch.equal(before, ts.flat.params)
    assert ts.flat.grad("encoder.resnet.fc.weight").abs().max() > 0
    f = model.scst_forward(images, [0, 1, 2, 3], ts.last_scst.scorer)          # the autograd form of the same thing
    assert f.dim() == 0 and np.isfinite(float(f))
