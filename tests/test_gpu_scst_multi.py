"""GPU (MI355X): self-critical training with S sampled captions per image and a leave-one-out baseline -- `sat_scst_weights_group`
and `sat_group_sum_rows` bit for bit against tests/scst_multi_reference.py, `rollout(num_samples=S)` of both models against the
rollout of inputs repeated by hand, `SelfCritical(num_samples=, baseline=)` against its composition, the collapsed policy, the
gradients against the CPU oracle (the bound tests/test_gpu_scst.py uses: rtol 1e-3 / atol 1e-7), and `TrainStep.scst_step`
against the autograd path.  Rows are image-major: row r = b * S + s."""
import importlib

import numpy as np
import pytest
import torch

import cider_reference as CR
import scst_attend_reference as SA
import scst_multi_reference as G
import scst_reference as S1

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import decoder as OD  # noqa: E402
from oracle import attend as OA  # noqa: E402

TINY = dict(layers=(1, 1, 1, 1), width=8)
END = 2
E, H, STEPS = S1.REPLAY_E, S1.REPLAY_H, S1.REPLAY_STEPS
ARG, UNSUPPORTED = 1001, 1003


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def bits64(t):
    return t.detach().contiguous().view(torch.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1: sat_scst_weights_group -------------------------------------------------------------------------------------------------
# the issue's table, and (2, 4, 3): S = 4, the division by S - 1 = 3 is inexact
GROUP_CASES = [(1, 2, 1), (3, 5, 4), (5, 64, 3), (300, 2, 2), (7, 3, 20), (2, 4, 3)]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("with_denom", [False, True], ids=["sum", "denom"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,S,T", GROUP_CASES)
def test_weights_group_bit_exact(B, S, T, mode, with_denom, f32):
    ids = G.group_ids(B, S, T, END, 10 * B + S)
    reward = G.group_rewards(B, S, B + T)
    if f32:
        reward = reward.astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(B))
    base_img = rng.random(B) * 2 - 0.5 if mode == 0 else None
    denom = 1234.0 if with_denom else None
    w, ln, M, adv, rows = sat.scst_weights_group(dev(ids), dev(reward), "sample_mean" if mode else dev(base_img), END,
                                                 torch.tensor([denom], dtype=torch.float64).cuda() if with_denom else None)
    w_ref, ln_ref, M_ref, adv_ref, rows_ref = G.weights_group(ids, reward, base_img, mode, END, denom)
    assert w.dtype == torch.float32 and ln.dtype == torch.int32 and M.dtype == adv.dtype == rows.dtype == torch.float64
    assert w.shape == (T * B * S,) and ln.shape == adv.shape == rows.shape == (B * S,)
    assert np.array_equal(ln.cpu().numpy(), ln_ref) and float(M.cpu()[0]) == float(M_ref)
    assert np.array_equal(adv.cpu().numpy().view(np.int64), adv_ref.view(np.int64))
    assert np.array_equal(rows.cpu().numpy().view(np.int64), rows_ref.view(np.int64))
    assert np.array_equal(w.cpu().numpy().view(np.int32), w_ref.view(np.int32))
    if T > 1 and B * S > 2:
        assert 1 in ln_ref and T in ln_ref                    # a row that ends at step 0, and rows that run to the end
    if mode == 1:                                             # the image whose samples all scored 0.1: exact zeros
        assert not w.view(T, B, S)[:, B // 2].any() and not adv.view(B, S)[B // 2].any()
    # a second call gives the same bits
    again = sat.scst_weights_group(dev(ids), dev(reward), "sample_mean" if mode else dev(base_img), END,
                                   torch.tensor([denom], dtype=torch.float64).cuda() if with_denom else None)
    assert torch.equal(bits(again[0]), bits(w)) and torch.equal(bits64(again[3]), bits64(adv))


@pytest.mark.parametrize("with_baseline,with_denom", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("B,S,T", [(7, 1, 5), (300, 1, 3), (3, 5, 4), (5, 64, 3)])
def test_mode_0_is_scst_weights_with_the_baseline_repeated(B, S, T, with_baseline, with_denom):
    ids = dev(G.group_ids(B, S, T, END, B + S))
    reward = dev(G.group_rewards(B, S, T))
    base = dev(np.random.Generator(np.random.PCG64(T)).random(B) * 3) if with_baseline else None
    denom = torch.tensor([77.0], dtype=torch.float64).cuda() if with_denom else None
    w, ln, M, adv, rows = sat.scst_weights_group(ids, reward, base, END, denom)
    w1, ln1, M1 = sat.scst_weights(ids.view(B * S, T), reward, base.repeat_interleave(S) if with_baseline else None, END, denom)
    assert torch.equal(bits(w), bits(w1)) and torch.equal(ln, ln1) and torch.equal(bits64(M), bits64(M1))
    assert torch.equal(rows, base.repeat_interleave(S) if with_baseline else torch.zeros_like(rows))


def test_the_result_does_not_depend_on_b():
    """an image's rows get the same advantage bits whatever else is in the batch (the weights differ only through M)"""
    S, T = 5, 4
    ids, reward = G.group_ids(6, S, T, END, 1), G.group_rewards(6, S, 1)
    one = torch.tensor([10.0], dtype=torch.float64).cuda()
    w6, _, _, adv6, rows6 = sat.scst_weights_group(dev(ids), dev(reward), "sample_mean", END, one)
    w2, _, _, adv2, rows2 = sat.scst_weights_group(dev(ids[4:]), dev(reward[4 * S:]), "sample_mean", END, one)
    assert torch.equal(bits64(adv6[4 * S:]), bits64(adv2)) and torch.equal(bits64(rows6[4 * S:]), bits64(rows2))
    assert torch.equal(bits(w6.view(T, 6, S)[:, 4:]), bits(w2.view(T, 2, S)))


def test_weights_group_refuses_with_the_outputs_untouched():
    lib = L.load()
    B, S, T = 3, 2, 4
    ids, reward, base = dev(G.group_ids(B, S, T, END, 0)), dev(G.group_rewards(B, S, 0)), torch.zeros(B, dtype=torch.float64).cuda()
    outs = dict(w=torch.full((T * B * S,), 7.0).cuda(), len=torch.full((B * S,), 7, dtype=torch.int32).cuda(),
                m=torch.full((1,), 7.0, dtype=torch.float64).cuda(), adv=torch.full((B * S,), 7.0, dtype=torch.float64).cuda(),
                base=torch.full((B * S,), 7.0, dtype=torch.float64).cuda())

    def call(**kw):
        a = dict(G.WEIGHTS_GROUP_VALID, ids=ids.data_ptr(), reward=reward.data_ptr(), **{k: v.data_ptr() for k, v in outs.items()})
        a.update(kw)
        if a["baseline"] == "PTR":
            a["baseline"] = base.data_ptr()
        return lib.sat_scst_weights_group(a["ids"], a["stride"], a["B"], a["S"], a["T"], END, a["reward"], a["baseline"], a["mode"],
                                          a["denom"], a["w"], a["len"], a["m"], a["adv"], a["base"], L.stream())

    for kw in G.WEIGHTS_GROUP_ARG_ERRORS:
        assert call(**kw) == ARG, kw
    for kw in G.WEIGHTS_GROUP_UNSUPPORTED:
        assert call(**kw) == UNSUPPORTED, kw
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert (v == 7).all(), k
    assert call() == 0 and call(base=None) == 0               # the valid call runs; baseline_out is optional
    torch.cuda.synchronize()
    assert not (outs["w"] == 7).any() and not (outs["len"] == 7).any()


# ---- 2: sat_group_sum_rows -----------------------------------------------------------------------------------------------------
def group_sum_raw(x, B, S, W, ld_in, out, ld_out):
    L.check(L.load().sat_group_sum_rows(x.data_ptr(), ld_in, B, S, W, out.data_ptr(), ld_out, L.stream()), "sat_group_sum_rows")


# (B, S, W, ld_in, ld_out, misaligned): dense strides first; (2, 4, 259) with rows padded to 260 is the vector body plus tail
SUM_CASES = [(1, 1, 1, 1, 1, False), (3, 5, 7, 7, 7, False), (2, 3, 256, 256, 256, False), (2, 4, 259, 259, 259, False),
             (2, 4, 259, 260, 260, False), (2, 3, 196 * 512, 196 * 512, 196 * 512, False), (2, 3, 256, 264, 256, False),
             (2, 3, 256, 256, 256, True), (3, 1, 259, 260, 264, False), (300, 2, 5, 5, 5, False)]


@pytest.mark.parametrize("B,S,W,ld_in,ld_out,misaligned", SUM_CASES)
def test_group_sum_rows_is_the_sequential_float32_sum(B, S, W, ld_in, ld_out, misaligned):
    g = torch.Generator().manual_seed(W + S)
    off = 1 if misaligned else 0
    src = torch.randn(off + B * S * ld_in, generator=g) * torch.tensor(10.0) ** torch.randint(-3, 4, (off + B * S * ld_in,), generator=g)
    dst = torch.full((off + B * ld_out,), 7.0)
    d_src, d_dst = src.cuda(), dst.cuda()
    x, out = d_src[off:].view(B * S, ld_in), d_dst[off:].view(B, ld_out)
    assert (x.data_ptr() % 16 != 0) == misaligned
    group_sum_raw(x, B, S, W, ld_in, out, ld_out)
    want = G.group_sum_rows(src[off:].view(B * S, ld_in)[:, :W].numpy(), S)
    got = d_dst.cpu()[off:].view(B, ld_out)
    assert np.array_equal(got[:, :W].numpy().view(np.int32), want.view(np.int32))
    assert (got[:, W:] == 7).all() and (d_dst.cpu()[:off] == 7).all()                    # nothing outside the W columns is written
    if S == 1:
        assert torch.equal(bits(got[:, :W]), bits(src[off:].view(B, ld_in)[:, :W]))       # a copy
    # the Python wrapper on the dense view gives the same bits
    if ld_in == W:
        assert torch.equal(bits(sat.group_sum_rows(x, S).cpu()), bits(got[:, :W]))


def test_group_sum_rows_refuses_with_the_output_untouched():
    lib = L.load()
    x, out = torch.randn(6, 8).cuda(), torch.full((2, 8), 7.0).cuda()
    big = torch.full((6 * 8 + 32,), 7.0).cuda()                                        # in and out inside one buffer

    def call(**kw):
        a = dict(G.GROUP_SUM_VALID, inp=x.data_ptr(), out=out.data_ptr())
        a.update(kw)
        if isinstance(a["out"], str):                                                  # "in+N" / "in-N": N bytes from the input
            a["inp"] = big.data_ptr() + 64
            a["out"] = a["inp"] + int(a["out"][2:])
        return lib.sat_group_sum_rows(a["inp"], a["ld_in"], a["B"], a["S"], a["W"], a["out"], a["ld_out"], L.stream())

    for kw in G.GROUP_SUM_ARG_ERRORS:
        assert call(**kw) == ARG, kw
    torch.cuda.synchronize()
    assert (out == 7).all() and (big == 7).all()


# ---- 3: rollout(num_samples=S) ---------------------------------------------------------------------------------------------------
def decoder_of(params, V, Lh):
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    return dec.cuda().train()


def grads_of(module, names=None):
    return {k: p.grad.detach().clone() for k, p in module.named_parameters() if p.grad is not None and (names is None or k in names)}


@pytest.mark.parametrize("Lh", [1, 2])
def test_decoder_rollout_of_s_rows_is_the_rollout_of_repeated_features(Lh):
    B, S, V = 5, 3, 203
    params, feats = S1.replay_inputs(OD, Lh, B, V)
    dec = decoder_of(params, V, Lh)
    G_out = torch.randn(STEPS * B * S, V, generator=torch.Generator().manual_seed(8)).cuda() * 1e-2
    f = feats.cuda().requires_grad_(True)
    torch.manual_seed(31)
    ids, logits = dec.rollout(f, STEPS, num_samples=S)
    assert ids.shape == (B, S, STEPS) and ids.dtype == torch.int64 and logits.shape == (STEPS * B * S, V)
    seed = dec.last_rollout_seed
    logits.backward(gradient=G_out)
    got, got_f = grads_of(dec), f.grad.clone()
    dec.zero_grad()
    fr = feats.cuda().repeat_interleave(S, 0).requires_grad_(True)
    torch.manual_seed(31)
    ids_r, logits_r = dec.rollout(fr, STEPS)
    assert dec.last_rollout_seed == seed
    logits_r.backward(gradient=G_out)
    assert torch.equal(ids.view(B * S, STEPS), ids_r) and torch.equal(bits(logits), bits(logits_r))
    want = grads_of(dec)
    for k in want:
        assert torch.equal(bits(got[k]), bits(want[k])), k
        assert want[k].abs().max() > 0, k
    assert got_f.shape == (B, E) and torch.equal(bits(got_f), bits(sat.group_sum_rows(fr.grad, S)))
    assert np.array_equal(got_f.cpu().numpy().view(np.int32), G.group_sum_rows(fr.grad.cpu().numpy(), S).view(np.int32))
    assert not torch.equal(ids[:, 0], ids[:, 1])              # the samples of an image are draws of their own


def attend_model(seed=0):
    P, C, Ea, Ha, V = (SA.SMALL[k] for k in "PCEHV")
    params = SA.params(OA, seed)
    model = sat.ShowAttendTellModel(Ha, C, V, Ea, None, feature_size=(P, C), compute_dtype="f32", vgg_cfg=[8, "M", C])
    model.load_state_dict(params, strict=False)
    return model.cuda().train(), params


@pytest.mark.parametrize("B", [5, 2])      # P = 16: B 5 encodes 80 rows once and repeats them to 240; B 2 (96 rows) encodes as it stands
def test_attend_rollout_of_s_rows_is_the_rollout_of_repeated_inputs(B):
    S, steps = 3, SA.STEPS
    P, C, V = SA.SMALL["P"], SA.SMALL["C"], SA.SMALL["V"]
    model, _ = attend_model()
    feats = SA.features(B)
    G_out = torch.randn(steps * B * S, V, generator=torch.Generator().manual_seed(8)).cuda() * 1e-2
    f = feats.cuda().requires_grad_(True)
    fm = f.detach().mean(1).requires_grad_(True)
    torch.manual_seed(41)
    ids, logits = model.rollout(f, fm, steps, num_samples=S)
    assert ids.shape == (B, S, steps) and logits.shape == (steps * B * S, V)
    assert model.last_rollout_inputs.shape == (B * S, steps) and model.last_alphas.shape == (steps * B * S, P)
    fed, alphas = model.last_rollout_inputs.clone(), model.last_alphas.clone()
    logits.backward(gradient=G_out)
    names = set(sat.attend.PARAM_ORDER)
    got, got_f, got_m = grads_of(model, names), f.grad.clone(), fm.grad.clone()
    model.zero_grad()
    fr = feats.cuda().repeat_interleave(S, 0).requires_grad_(True)
    fmr = fm.detach().repeat_interleave(S, 0).requires_grad_(True)
    torch.manual_seed(41)
    ids_r, logits_r = model.rollout(fr, fmr, steps)
    logits_r.backward(gradient=G_out)
    assert torch.equal(ids.view(B * S, steps), ids_r) and torch.equal(bits(logits), bits(logits_r))
    assert torch.equal(fed, model.last_rollout_inputs) and torch.equal(bits(alphas), bits(model.last_alphas))
    want = grads_of(model, names)
    assert set(want) == names
    for k in want:
        assert torch.equal(bits(got[k]), bits(want[k])), k
        assert want[k].abs().max() > 0, k
    assert got_f.shape == (B, P, C) and got_m.shape == (B, C)
    assert torch.equal(bits(got_f), bits(sat.group_sum_rows(fr.grad, S))) and got_f.abs().max() > 0
    assert torch.equal(bits(got_m), bits(sat.group_sum_rows(fmr.grad, S))) and got_m.abs().max() > 0
    with pytest.raises(ValueError, match="arg-max"):
        model.rollout(f, fm, steps, greedy=True, num_samples=S)


def test_context_encode_once_per_image_has_the_bits_of_encoding_every_row_across_gemm_tiles():
    """B 16, S 5, P 196, C 512: sat_gemm_f32 runs the B * P = 3 136 rows on 64 x 64 tiles and the R * P = 15 680 rows on 128 x 128
    (launch_f32_auto: 123 * 4 >= 384 workgroups) -- the encode-once shortcut rests on a row's bits not depending on the tile"""
    import types
    B, S, P, C = 16, 5, 196, 512
    gen = torch.Generator().manual_seed(12)
    m = types.SimpleNamespace(image_att_w=(torch.randn(C, C, generator=gen) / 16).cuda())
    src = torch.randn(B, P, C, generator=gen).cuda()
    f2 = src.repeat_interleave(S, 0).view(B * S * P, C)
    lib = L.load()
    assert not L.gemm_splits_k(0, 1, C, C, C, B * S * P, C, C)
    got = sat.attend._context_encode_group(lib, m, src, S, f2)
    want = sat.attend._context_encode(lib, m, f2)
    assert got.shape == want.shape == (B * S * P, C) and torch.equal(bits(got), bits(want))
    ref = src.view(B * P, C)[:64].double() @ m.image_att_w.double()
    assert torch.allclose(want.view(B, S, P * C)[:, 0].reshape(B * P, C)[:64].double(), ref, rtol=0, atol=1e-4)


# ---- 4: SelfCritical(num_samples=3, baseline="sample_mean") ----------------------------------------------------------------------
def tiny_corpus():
    """4 images x 2 references over ids 3..22"""
    rng = np.random.Generator(np.random.PCG64(11))
    return [[[int(t) for t in rng.integers(3, 23, rng.integers(4, 9))] for _ in range(2)] for _ in range(4)]


IDX = [0, 1, 2, 3, 1, 0]


def composition(roll, scorer, idx, S, V):
    """the loss by hand: rollout, `kept_tokens`, `scorer.score`, `scst_weights_group`, `ce_rows_weighted`"""
    ids, logits = roll()
    rows = ids.view(-1, ids.shape[2])
    kept = sat.kept_tokens(rows, END)
    _, reward = scorer.score(rows, [i for i in idx for _ in range(S)], end_id=END, kept=kept)
    w, _, _, adv, base = sat.scst_weights_group(ids, reward, "sample_mean", END)
    buf = L.logits_buffer(logits.shape[0], V, logits.device)
    buf[:, :V].copy_(logits.detach())
    _, loss = sat.ce_rows_weighted(buf[:, :V], rows, w, write_grad=True)
    return ids, reward, adv, base, loss


def check_self_critical(run, roll, scorer, refs, idx, S, V, T):
    B = len(idx)
    torch.manual_seed(5)
    sc = sat.SelfCritical(scorer, END, num_samples=S, baseline="sample_mean")
    loss = run(sc)
    assert loss.dim() == 0 and np.isfinite(float(loss.detach()))
    assert sc.last_ids.shape == (B, S, T) and sc.last_greedy_ids is None                  # no greedy decode ran
    for t in (sc.last_reward, sc.last_baseline, sc.last_advantage):
        assert t.dtype == torch.float64 and t.shape == (B * S,)
    torch.manual_seed(5)
    ids, reward, adv, base, manual = composition(roll, scorer, idx, S, V)
    assert torch.equal(ids, sc.last_ids) and torch.equal(bits64(reward), bits64(sc.last_reward))
    assert torch.equal(bits64(adv), bits64(sc.last_advantage)) and torch.equal(bits64(base), bits64(sc.last_baseline))
    assert torch.equal(bits(manual), bits(loss.reshape(1)))
    _, want = CR.Corpus(refs).score([CR.truncate(r, END) for r in ids.view(B * S, T).cpu().tolist()], [i for i in idx for _ in range(S)])
    err = np.abs(sc.last_reward.cpu().numpy() - np.asarray(want)).max()
    print("max |CIDEr - restatement| = %.3g" % err)
    assert err <= 1e-9
    torch.manual_seed(5)
    again = sat.SelfCritical(scorer, END, num_samples=S, baseline="sample_mean")
    loss2 = run(again)
    assert torch.equal(again.last_ids, ids) and torch.equal(bits(loss2), bits(loss))
    torch.manual_seed(6)
    other = sat.SelfCritical(scorer, END, num_samples=S, baseline="sample_mean")
    run(other)
    assert not torch.equal(other.last_ids, ids)


def test_self_critical_sample_mean_is_its_composition():
    B, S, V, Lh = 6, 3, 24, 1
    refs = tiny_corpus()
    params, feats = S1.replay_inputs(OD, Lh, B, V)
    dec = decoder_of(params, V, Lh)
    f = feats.cuda()
    check_self_critical(lambda sc: sc(dec, f, IDX), lambda: dec.rollout(f, num_samples=S), sat.CiderScorer(refs), refs, IDX, S, V, 20)


def test_self_critical_attend_sample_mean_is_its_composition():
    B, S, V = 6, 3, SA.SMALL["V"]
    refs = tiny_corpus()
    model, _ = attend_model()
    f = SA.features(B).cuda()
    fm = f.mean(1)
    check_self_critical(lambda sc: sc.attend(model, f, fm, IDX, SA.STEPS), lambda: model.rollout(f, fm, SA.STEPS, num_samples=S),
                        sat.CiderScorer(refs), refs, IDX, S, V, SA.STEPS)


def test_greedy_baseline_with_s_rows_decodes_once_per_image_and_mixed_reward_works():
    B, S, V = 6, 3, 24
    refs = tiny_corpus()
    params, feats = S1.replay_inputs(OD, 1, B, V)
    dec = decoder_of(params, V, 1)
    f = feats.cuda()
    scorer = sat.MixedReward([(sat.CiderScorer(refs), 1.0), (sat.RougeLScorer(refs), 0.5)])
    torch.manual_seed(9)
    sc = sat.SelfCritical(scorer, END, num_samples=S, baseline="greedy")
    loss = sc(dec, f, IDX)
    assert sc.last_greedy_ids.shape == (B, 20) and sc.last_ids.shape == (B, S, 20) and np.isfinite(float(loss))
    greedy = dec.sample(f)
    assert torch.equal(greedy, sc.last_greedy_ids)
    _, base = scorer.score(greedy, IDX, end_id=END, kept=sat.kept_tokens(greedy, END))
    assert torch.equal(bits64(sc.last_baseline), bits64(base.repeat_interleave(S)))       # mode 0: the image's baseline on its S rows
    assert torch.equal(bits64(sc.last_advantage), bits64(sc.last_reward - base.repeat_interleave(S)))


# ---- 5: the collapsed policy -----------------------------------------------------------------------------------------------------
def collapse(dec, token=7):
    with torch.no_grad():
        dec.linear.weight.zero_()
        dec.linear.bias.zero_()
        dec.linear.bias[token] = 80.0            # the Gumbel noise of a draw cannot bridge 80: every draw is `token`


def test_collapsed_policy_gives_an_exactly_zero_loss_and_gradient():
    B, S, V, Lh = 6, 3, 24, 2
    scorer = sat.CiderScorer(tiny_corpus())
    params, feats = S1.replay_inputs(OD, Lh, B, V)
    dec = decoder_of(params, V, Lh)
    collapse(dec)
    f = feats.cuda().requires_grad_(True)
    sc = sat.SelfCritical(scorer, END, num_samples=S, baseline="sample_mean")
    loss = sc(dec, f, IDX)
    loss.backward()
    assert (sc.last_ids == 7).all()
    assert float(loss) == 0.0 and not sc.last_advantage.any()
    for k, g in grads_of(dec).items():
        assert not g.any(), k
    assert not f.grad.any()
    # the fused step: loss slot, every gradient and the fault slot exactly 0
    model = ts_model(V, Lh)
    collapse(model.decoder)
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    before = ts.flat.params.clone()
    out = ts.scst_step(feats.cuda(), IDX, scorer, num_samples=S, baseline="sample_mean")
    ts.check_ids()
    assert float(out.cpu()[0]) == 0.0 and (ts.last_scst.last_ids == 7).all()
    assert not ts.flat.grads.any() and float(ts.fault_slot.cpu()[0]) == 0.0
    assert torch.equal(before, ts.flat.params)


# ---- 6: gradients against the CPU oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lh", [1, 2])
def test_gradients_match_the_oracle(Lh):
    """the oracle teacher-forced on the drawn tokens (R rows of repeated features) with the kernel's weights; its R-row feature
    gradient summed per image in float64"""
    B, S, V = 5, 3, 203
    params, feats = S1.replay_inputs(OD, Lh, B, V)
    dec = decoder_of(params, V, Lh)
    rng = np.random.Generator(np.random.PCG64(3))
    reward = torch.from_numpy(rng.random(B * S) * 2).cuda()
    f = feats.cuda().requires_grad_(True)
    torch.manual_seed(77)
    ids, logits = dec.rollout(f, STEPS, num_samples=S)
    end = int(ids[0, 0, 2])                                   # row 0 ends at step 2 at the latest: masked rows behind it
    loss = sat.scst_loss(logits, ids, reward, "sample_mean", end)
    loss.backward()
    got = grads_of(dec)
    got["features"] = f.grad.detach().clone()
    w, ln, _, adv, _ = sat.scst_weights_group(ids, reward, "sample_mean", end)
    w, rows = w.cpu().numpy(), ids.view(B * S, STEPS).cpu()
    assert ln[0] <= 3 and (w == 0).any() and (w > 0).any() and (w < 0).any()
    w_ref = G.weights_group(ids.cpu().numpy(), reward.cpu().numpy(), None, 1, end)[0]
    assert np.array_equal(w.view(np.int32), w_ref.view(np.int32))
    fed, R = rows[:, :STEPS - 1], B * S
    feats_r = feats.repeat_interleave(S, 0)
    ref_logits, tape = OD.decoder_forward(params, feats_r, fed, [STEPS] * R, Lh, keep=True)
    _, ref_loss, dlogits = S1.loss_and_grad(ref_logits, rows, w)
    # |loss - oracle| <= sum|w| * 2 * max|logit error|: |advantage| < 2, sum over rows of |w| <= max|advantage|, logits within 1e-5
    assert abs(float(loss) - float(ref_loss)) < 4e-5
    grads, d_feat = OD.decoder_backward(params, tape, fed, [STEPS] * R, dlogits.float(), Lh)
    grads["features"] = d_feat.double().view(B, S, E).sum(1).float()
    for k in sorted(grads):
        ref = grads[k].numpy()
        err = np.abs(got[k].cpu().numpy() - ref)
        tol = 1e-7 + 1e-3 * np.abs(ref)
        print("%-22s max err %.3g (worst err/tol %.3g)" % (k, err.max(), (err / tol).max()))
    for k in sorted(grads):
        np.testing.assert_allclose(got[k].cpu().numpy(), grads[k].numpy(), rtol=1e-3, atol=1e-7, err_msg=k)


# ---- 7: the fused step -----------------------------------------------------------------------------------------------------------
def ts_model(V, Lh, dtype="f32"):
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY, compute_dtype=dtype)
    model.decoder.load_state_dict(OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(4)))
    return model.cuda().train()


@pytest.mark.parametrize("baseline", ["sample_mean", "greedy"])
@pytest.mark.parametrize("Lh", [1, 2])
def test_scst_step_of_s_rows_equals_the_autograd_path(Lh, baseline):
    B, S, V = 6, 3, 24
    scorer = sat.CiderScorer(tiny_corpus())
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(2)).cuda()
    ma, mb = ts_model(V, Lh), ts_model(V, Lh)
    opt = sat.FusedClampAdam(ma.decoder.parameters(), lr=1e-3, clip=0.1)
    ts = sat.TrainStep(mb, lr=1e-3, grad_clip=0.1)
    opt.zero_grad()
    torch.manual_seed(21)
    sc = sat.SelfCritical(scorer, END, num_samples=S, baseline=baseline)
    loss_a = sc(ma.decoder, feats, IDX)
    loss_a.backward()
    grads_a = {k: p.grad.detach().clone() for k, p in ma.decoder.named_parameters()}
    opt.step()
    torch.manual_seed(21)
    loss_b = ts.scst_step(feats, IDX, scorer, num_samples=S, baseline=baseline)
    fs = ts.last_scst
    assert fs.last_ids.shape == (B, S, 20) and torch.equal(fs.last_ids, sc.last_ids)
    assert torch.equal(bits64(fs.last_reward), bits64(sc.last_reward)) and torch.equal(bits64(fs.last_baseline), bits64(sc.last_baseline))
    assert torch.equal(bits64(fs.last_advantage), bits64(sc.last_advantage))
    assert (fs.last_greedy_ids is None) == (baseline == "sample_mean") == (sc.last_greedy_ids is None)
    assert loss_b.shape == (1,) and torch.equal(bits(loss_b), bits(loss_a.reshape(1)))
    slot = ts.flat.grads[ts.flat.loss_slot:ts.flat.loss_slot + 1]
    assert torch.equal(bits(slot), bits(loss_a.reshape(1)))
    for k, p in mb.decoder.named_parameters():          # (value equality: the autograd path accumulates into a zeroed buffer, 0 + -0 = +0)
        assert torch.equal(ts.flat.grad("decoder." + k), grads_a[k]), k
        assert grads_a[k].abs().max() > 0, k
    for (k, pa), (_, pb) in zip(ma.decoder.named_parameters(), mb.decoder.named_parameters()):
        assert torch.equal(pa, pb), k
    assert float(ts.fault_slot.cpu()[0]) == 0.0


def test_scst_step_of_s_rows_through_the_encoder_trains_the_head_like_the_autograd_path():
    B, S, V = 4, 3, 24
    scorer = sat.CiderScorer(tiny_corpus())
    ma, mb = ts_model(V, 1), ts_model(V, 1)
    mb.load_state_dict(ma.state_dict())
    images = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    torch.manual_seed(23)
    loss_a = ma.scst_forward(images, [0, 1, 2, 3], scorer, num_samples=S, baseline="sample_mean")
    loss_a.backward()
    ts = sat.TrainStep(mb, lr=1e-3, grad_clip=0.1)
    torch.manual_seed(23)
    loss_b = ts.scst_forward_backward(images, [0, 1, 2, 3], scorer, num_samples=S, baseline="sample_mean")
    ts.check_ids()
    assert torch.equal(ts.last_scst.last_ids, ma.last_scst.last_ids) and torch.equal(bits(loss_b), bits(loss_a.reshape(1)))
    for name in ("encoder.resnet.fc.weight", "encoder.resnet.fc.bias", "encoder.bn.weight", "encoder.bn.bias"):
        ga = dict(ma.named_parameters())[name].grad
        assert torch.equal(ts.flat.grad(name), ga), name
    assert ts.flat.grad("encoder.resnet.fc.weight").abs().max() > 0
    assert ts.last_d_features.shape == (B, E) and float(ts.fault_slot.cpu()[0]) == 0.0


@pytest.mark.parametrize("first,second", [((2, 6), (3, 4)), ((3, 4), (2, 6)), ((1, 12), (3, 4)), ((3, 4), (1, 12))])
def test_one_engine_takes_another_s_at_the_same_packed_row_count(first, second):
    """(S, steps) pairs of equal S * steps: the step buffers of B images and B * S * steps packed rows must not be shared between
    two S (the R-row feature buffers differ in size): the second call gives what a fresh engine gives"""
    B, V = 4, 24
    scorer = sat.CiderScorer(tiny_corpus())
    feats = torch.randn(B, E, generator=torch.Generator().manual_seed(6)).cuda()
    idx = [0, 1, 2, 3]
    ma, mb = ts_model(V, 1), ts_model(V, 1)
    used, fresh = sat.TrainStep(ma, lr=1e-3, grad_clip=0.1), sat.TrainStep(mb, lr=1e-3, grad_clip=0.1)
    torch.manual_seed(30)
    used.scst_forward_backward(feats, idx, scorer, steps=first[1], num_samples=first[0], baseline="greedy")
    out = []
    for ts in (used, fresh):
        torch.manual_seed(31)
        S, steps = second
        loss = ts.scst_forward_backward(feats, idx, scorer, steps=steps, num_samples=S, baseline="greedy")
        ts.check_ids()
        assert ts.last_scst.last_ids.shape == ((B, S, steps) if S > 1 else (B, steps))
        assert ts.last_d_features.shape == (B, E) and float(ts.fault_slot.cpu()[0]) == 0.0
        out.append((ts.last_scst.last_ids, bits(loss), bits(ts.last_d_features), bits(ts.flat.grads)))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert out[0][2].ne(0).any()


def test_group_sum_rows_checks_its_out_tensor():
    x = torch.randn(12, 5, generator=torch.Generator().manual_seed(8)).cuda()
    out = torch.full((4, 5), 7.0).cuda()
    assert sat.group_sum_rows(x, 3, out=out) is out
    assert torch.equal(bits(out), bits(sat.group_sum_rows(x, 3)))
    guard = torch.full((6, 5), 7.0).cuda()
    # too few rows, too many, another width, another dtype, the host, rows that are not dense
    for bad in (guard[:3], guard, guard[:4, :4], guard[:4].double(), guard[:4].cpu(), torch.full((4, 10), 7.0).cuda()[:, ::2]):
        with pytest.raises(TypeError, match="out must be"):
            sat.group_sum_rows(x, 3, out=bad)
    assert torch.equal(guard, torch.full((6, 5), 7.0).cuda())


# ---- 8: the defaults are the calls without the keywords --------------------------------------------------------------------------
def test_defaults_give_the_bits_of_the_calls_without_the_keywords():
    B, V, Lh = 6, 24, 1
    scorer = sat.CiderScorer(tiny_corpus())
    params, feats = S1.replay_inputs(OD, Lh, B, V)
    f = feats.cuda()
    runs = []
    for kw in ({}, dict(num_samples=1, baseline="greedy")):
        dec = decoder_of(params, V, Lh)
        torch.manual_seed(5)
        sc = sat.SelfCritical(scorer, END, **kw)
        loss = sc(dec, f, IDX)
        loss.backward()
        assert sc.last_ids.shape == (B, 20) and sc.last_reward.shape == (B,)
        assert torch.equal(sc.last_advantage, sc.last_reward - sc.last_baseline)
        torch.manual_seed(5)
        ids, logits = dec.rollout(f, **({} if not kw else dict(num_samples=1)))
        assert ids.shape == (B, 20)
        manual = sat.scst_loss(logits, ids, sc.last_reward, sc.last_baseline, END, **({} if not kw else dict(num_samples=1)))
        runs.append((sc.last_ids, sc.last_greedy_ids, bits(loss), bits(manual), grads_of(dec)))
    (ids0, gr0, l0, m0, g0), (ids1, gr1, l1, m1, g1) = runs
    assert torch.equal(ids0, ids1) and torch.equal(gr0, gr1) and torch.equal(l0, l1) and torch.equal(m0, m1) and torch.equal(l0, m0)
    for k in g0:
        assert torch.equal(bits(g0[k]), bits(g1[k])), k
    # scst_forward and scst_step, images through the tiny encoder
    images = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    idx = [0, 1, 2, 3]
    outs = []
    for kw in ({}, dict(num_samples=1, baseline="greedy")):
        model = ts_model(V, 1)
        model.load_state_dict(outs[0][0] if outs else model.state_dict())
        state = {k: v.clone() for k, v in model.state_dict().items()}
        torch.manual_seed(7)
        lf = model.scst_forward(images, idx, scorer, **kw)
        ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
        torch.manual_seed(7)
        ls = ts.scst_step(images, idx, scorer, **kw)
        outs.append((state, bits(lf.reshape(1)), bits(ls), ts.last_scst.last_ids, ts.flat.grads.clone(), ts.flat.params.clone()))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3])
    assert torch.equal(bits(outs[0][4]), bits(outs[1][4])) and torch.equal(bits(outs[0][5]), bits(outs[1][5]))
