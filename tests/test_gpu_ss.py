"""GPU (MI355X): scheduled sampling in the decoder's training forward (`sat_ss_decoder_fwd`, `sat_vocab_sample`).  The draws are
replayed in numpy from the returned logits and the seed (tests/ss_reference.py); the rest is parity with the CPU oracle run
teacher-forced on the tokens actually fed, which is what the scheduled-sampling forward must equal."""
import importlib

import numpy as np
import pytest
import torch

import ss_reference as R

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import decoder as OD  # noqa: E402

TINY = dict(layers=(1, 1, 1, 1), width=8)


def make_decoder(E, H, V, Lh, seed=0):
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(seed))
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    return dec.cuda().train(), params


def inputs(B, E, V, width, seed=1):
    g = torch.Generator().manual_seed(seed)
    caps = torch.randint(4, V, (B, width), generator=g)
    caps[:, 0] = 1
    feats = torch.randn(B, E, generator=g)
    return feats, caps


def check_used_against_replay(out, used, caps_in, l1, ss_prob, seed, rank=0):
    """every decision of one forward, recomputed in float64 from its logits"""
    bs = OD.batch_sizes(l1)
    want, mask, margin = R.draws(out.detach().cpu().numpy(), bs, caps_in.cpu().numpy(), ss_prob, seed, rank)
    got = used.cpu().numpy()
    assert got.shape == want.shape
    close = margin < 1e-4
    assert np.array_equal(got[~close], want[~close]), np.argwhere(got != want)
    return mask


def test_peaked_bias_every_draw_is_the_peak():
    """ss_prob = 1 and logit bias +60 on token k: every fed token of step >= 2 is k, step 1 keeps <start>"""
    E, H, V, k = 32, 64, 200, 37
    dec, params = make_decoder(E, H, V, 1)
    with torch.no_grad():
        dec.linear.weight.mul_(0.01)
        dec.linear.bias.zero_()
        dec.linear.bias[k] = 60.0
    lengths = [10, 10, 9, 7, 4, 3]
    feats, caps = inputs(len(lengths), E, V, 10)
    l1 = [l - 1 for l in lengths]
    dec.ss_prob = 1.0
    dec(feats.cuda(), caps[:, :-1].cuda(), l1)
    used = dec.last_ss_inputs.cpu()
    assert used.shape == (len(lengths), max(l1) - 1)
    assert torch.equal(used[:, 0], caps[:, 0])
    for b, n in enumerate(l1):
        for t in range(2, max(l1)):
            want = k if t < n else int(caps[b, t - 1])
            assert int(used[b, t - 1]) == want, (b, t)


@pytest.mark.parametrize("rank", [0, 3])
def test_vocab_sample_mask_bits_and_draws_exact(rank):
    """the single step: every mask bit exact, every draw equal to the float64 Gumbel-max unless its top two are within 1e-4"""
    lib = L.load()
    B, H, V, t, prob, seed = 64, 64, 1003, 5, 0.5, 0x0123456789ABCDEF
    g = torch.Generator().manual_seed(3)
    h = torch.randn(B, H, generator=g).cuda()
    w = (torch.randn(V, H, generator=g) * 0.3).cuda()
    b = torch.randn(V, generator=g).cuda()
    logits = torch.zeros(B, 1004, device="cuda")
    teacher = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    wsb = lib.sat_ss_decoder_fwd_ws_bytes(B, V)
    ws = torch.empty(wsb // 4, device="cuda")
    for with_teacher in (True, False):
        L.check(lib.sat_vocab_sample(L.ptr(h), L.ptr(w), L.ptr(b), B, H, V, L.ptr(logits), 1004, prob, seed, t, rank,
                                     L.ptr(teacher) if with_teacher else None, 1, L.ptr(ids), 1, None, 0, None, L.ptr(ws), wsb,
                                     L.stream()), "sat_vocab_sample")
        got = ids.cpu().numpy()
        lg = logits.cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(lg[:, :V], (h.double() @ w.double().t() + b.double()).cpu().numpy(), rtol=0, atol=1e-4)
        assert np.all(lg[:, V:] == 0)
        n_close = 0
        for r in range(B):
            masked = R.mask_uniform(seed, rank, r, t) < prob
            if with_teacher and not masked:
                assert got[r] == -1, r
                continue
            assert 0 <= got[r] < V
            s = lg[r, :V] + R.noise(seed, rank, r, t, V)
            top = np.sort(s)[-2:]
            if top[1] - top[0] < 1e-4:
                n_close += 1
                continue
            assert got[r] == int(np.argmax(s)), r
        assert n_close <= 2
        if with_teacher:
            assert 16 < int((got != -1).sum()) < 48


def test_vocab_sample_frequencies_match_softmax():
    """20 000 rows with the same logits: the device's draws (one per row) pass a chi-square test against softmax"""
    lib = L.load()
    B, H, V = 20000, 4, 12
    logits_row = torch.tensor([1.5, 0.5, 0.0, -0.5, 1.0, 0.25, -1.0, 2.0, 0.0, -2.0, 0.75, 0.1])
    h = torch.zeros(B, H, device="cuda")
    w = torch.zeros(V, H, device="cuda")
    b = logits_row.cuda()
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    wsb = lib.sat_ss_decoder_fwd_ws_bytes(B, V)
    ws = torch.empty(wsb // 4, device="cuda")
    L.check(lib.sat_vocab_sample(L.ptr(h), L.ptr(w), L.ptr(b), B, H, V, None, 0, 1.0, 77, 2, 0, None, 0, L.ptr(ids), 1, None, 0, None,
                                 L.ptr(ws), wsb, L.stream()), "sat_vocab_sample")
    obs = np.bincount(ids.cpu().numpy(), minlength=V)
    p = torch.softmax(logits_row.double(), 0).numpy()
    chi2 = float(((obs - B * p) ** 2 / (B * p)).sum())
    assert chi2 < 31.26, (chi2, obs)          # chi-square, 11 degrees of freedom, p = 1e-3


@pytest.mark.parametrize("Lh", [1, 2])
def test_exact_replay_and_parity_on_used(Lh):
    """ss_prob = 0.5, ragged lengths, V = 1003: draws replayed exactly; logits, CE and every gradient equal the oracle's
    teacher-forced forward / backward on the tokens fed"""
    E, H, V = 32, 64, 1003
    dec, params = make_decoder(E, H, V, Lh, seed=4)
    lengths = [12, 12, 11, 9, 9, 7, 4, 3]
    feats, caps = inputs(len(lengths), E, V, 12, seed=5)
    targets, l1 = sat.pack_targets(caps.cuda(), lengths)
    dec.ss_prob = 0.5
    f = feats.cuda().requires_grad_(True)
    dec.zero_grad()
    out = dec(f, caps[:, :-1].cuda(), l1)
    used, seed = dec.last_ss_inputs, dec.last_ss_seed
    mask = check_used_against_replay(out, used, caps[:, :-1], l1, 0.5, seed)
    assert mask.sum() >= 5
    used_c = used.cpu()
    ref_logits, tape = OD.decoder_forward(params, feats, used_c, l1, Lh, keep=True)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_logits.numpy(), rtol=0, atol=1e-5)
    loss = torch.nn.CrossEntropyLoss()(out, targets)
    tc = targets.cpu()
    assert abs(loss.item() - OD.cross_entropy(ref_logits, tc).item()) < 1e-4
    loss.backward()
    grads, d_feat = OD.decoder_backward(params, tape, used_c, l1, OD.cross_entropy_grad(ref_logits, tc), Lh)
    np.testing.assert_allclose(f.grad.cpu().numpy(), d_feat.numpy(), rtol=1e-3, atol=1e-7)
    for k, p in dec.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), rtol=1e-3, atol=1e-7, err_msg=k)


def ts_model(E, H, V, Lh, dtype, seed=4):
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY, compute_dtype=dtype)
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(seed))
    model.decoder.load_state_dict(params)
    return model.cuda().train(), params


def oracle_on_used(params, feats, used, caps, lengths, Lh, denom):
    targets, l1 = sat.pack_targets(caps, lengths)
    tc = targets.cpu()
    ref_logits, tape = OD.decoder_forward(params, feats, used, l1, Lh, keep=True)
    loss = OD.cross_entropy(ref_logits, tc) * (ref_logits.shape[0] / denom)
    grads, d_feat = OD.decoder_backward(params, tape, used, l1, OD.cross_entropy_grad(ref_logits, tc, denom=denom), Lh)
    return loss, grads, d_feat


@pytest.mark.parametrize("Lh", [1, 2])
def test_trainstep_exact_mode_parity_on_used(Lh):
    E, H, V = 32, 64, 1003
    model, params = ts_model(E, H, V, Lh, "f32")
    model.decoder.ss_prob = 0.5
    lengths = [12, 12, 11, 9, 9, 7, 4, 3]
    feats, caps = inputs(len(lengths), E, V, 12, seed=6)
    ts = sat.TrainStep(model)
    n_tok = sum(l - 1 for l in lengths)
    loss = ts.forward_backward((feats.cuda(), caps.cuda(), lengths), 1.0 / n_tok)
    used = model.decoder.last_ss_inputs.cpu()
    assert not torch.equal(used, caps[:, :used.shape[1]])
    ref_loss, grads, d_feat = oracle_on_used(params, feats, used, caps.cuda(), lengths, Lh, n_tok)
    assert abs(loss.item() - ref_loss.item()) < 1e-4
    np.testing.assert_allclose(ts.last_d_features.cpu().numpy(), d_feat.numpy(), rtol=1e-3, atol=1e-7)
    for k, p in model.decoder.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), rtol=1e-3, atol=1e-7, err_msg=k)


def test_trainstep_bf16_cfg1_shape_reproducible_and_learns():
    """BASELINE configs[1]'s decoder (B 64, E 256, H 512, V 10 000, length-20 captions), bf16 throughput mode, ss_prob 0.25"""
    E, H, V, B = 256, 512, 10000, 64
    model, params = ts_model(E, H, V, 1, "bf16", seed=8)
    model.decoder.ss_prob = 0.25
    ts = sat.TrainStep(model)
    assert ts.decoder_gemm_dtype == "bf16"
    lengths = [20] * B
    feats, caps = inputs(B, E, V, 20, seed=9)
    fc, cc = feats.cuda(), caps.cuda()
    n_tok = sum(l - 1 for l in lengths)
    runs = []
    for s in (11, 11, 12):
        torch.manual_seed(s)
        loss = ts.forward_backward((fc, cc, lengths), 1.0 / n_tok).clone()
        runs.append((model.decoder.last_ss_inputs.clone(), loss, ts.flat_grad.clone()))
    (u0, l0, g0), (u1, l1_, g1), (u2, _, _) = runs
    assert torch.equal(u0, u1) and torch.equal(l0, l1_) and torch.equal(g0, g1)
    assert not torch.equal(u0, u2)
    frac = float((u0[:, 1:] != cc[:, 1:18]).float().mean())
    assert 0.15 < frac < 0.3, frac                    # ~ss_prob of the entries of steps >= 2 (a draw rarely equals the teacher)
    ref_loss, _, _ = oracle_on_used(params, feats, u0.cpu(), cc, lengths, 1, n_tok)
    assert abs(l0.item() - ref_loss.item()) < 2e-3, (l0.item(), ref_loss.item())
    losses = [ts.step(fc, cc, lengths).item() for _ in range(5)]
    assert losses[-1] < losses[0], losses


def test_eval_mode_and_zero_prob_are_todays_path():
    E, H, V = 32, 64, 203
    dec, _ = make_decoder(E, H, V, 2)
    lengths = [9, 8, 8, 5]
    feats, caps = inputs(len(lengths), E, V, 9)
    l1 = [l - 1 for l in lengths]
    f, c = feats.cuda(), caps[:, :-1].cuda()
    state = torch.get_rng_state()
    ref = dec(f, c, l1).detach().clone()                  # training mode, ss_prob 0
    assert torch.equal(torch.get_rng_state(), state) and dec.last_ss_inputs is None
    dec.ss_prob = 0.5
    dec.eval()
    got = dec(f, c, l1).detach()
    assert torch.equal(got, ref) and dec.last_ss_inputs is None
    assert torch.equal(torch.get_rng_state(), state)
    dec.train()
    dec(f, c, l1)
    assert not torch.equal(torch.get_rng_state(), state) and dec.last_ss_inputs is not None


def test_two_steps_and_batch_one():
    E, H, V = 32, 64, 150
    dec, params = make_decoder(E, H, V, 1)
    feats, caps = inputs(5, E, V, 3)
    ref = dec(feats.cuda(), caps[:, :-1].cuda(), [2] * 5).detach().clone()
    dec.ss_prob = 1.0
    out = dec(feats.cuda(), caps[:, :-1].cuda(), [2] * 5)         # T = 2: no step has a draw to take
    assert torch.equal(dec.last_ss_inputs.cpu(), caps[:, :1])
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=1e-5)
    feats, caps = inputs(1, E, V, 9, seed=3)
    out = dec(feats.cuda(), caps[:, :-1].cuda(), [8])
    used = dec.last_ss_inputs.cpu()
    check_used_against_replay(out, dec.last_ss_inputs, caps[:, :-1], [8], 1.0, dec.last_ss_seed)
    ref_logits = OD.decoder_forward(params, feats, used, [8], 1)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_logits.numpy(), rtol=0, atol=1e-5)
