"""GPU: dropout.  The kernel `sat_dropout_f32` against the numpy restatement of its contract bit for bit, and both
decoders in training mode against float64 references that are fed the masks of `last_dropout_seed` (tests/dropout_reference.py):
the autograd path of `DecoderRNN`, `TrainStep.forward_backward` in its exact-f32 and bf16 modes, and `ShowAttendTellModel`."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_reference as DR

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import attend as OA  # noqa: E402
from oracle import decoder as OD  # noqa: E402

TINY = dict(layers=(1, 1, 1, 1), width=8)
SEED = 0xC0FFEE1234567891              # bits set above 2^32
P_TOP = float(np.nextafter(np.float32(1), np.float32(0)))       # 1 - 2^-24: the largest float32 below 1
PROBS = [0.0, 2.0 ** -24, 0.1, 0.5, P_TOP]
SENTINEL = 12345.0


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


def offset_rows(rows, ld, fill=None, gen=None):
    """f32 [rows, ld] whose base pointer sits 4 bytes behind a 16-byte boundary"""
    buf = torch.empty(rows * ld + 1, device="cuda")
    v = buf[1:].view(rows, ld)
    assert v.data_ptr() % 16 == 4
    v.copy_(torch.randn(rows, ld, generator=gen) if fill is None else torch.full((rows, ld), fill))
    return v


# ------------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("rows,cols,ld", [(1, 1, 1), (3, 5, 5), (2, 4, 4), (7, 64, 64), (5, 7, 12), (65, 260, 264), (130, 516, 516)])
def test_kernel_bits_equal_the_reference(rows, cols, ld):
    """every element of y equals the restatement's float32 bit for bit -- 16-byte path, its scalar tail and the scalar path (base
    pointers 4 bytes off alignment) -- in place as out of place, and the padding columns [cols, ld) of y keep their contents"""
    lib = L.load()
    gen = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.randn(rows, ld, generator=gen)
    xa = x.cuda()
    xo = offset_rows(rows, ld)
    xo.copy_(x)
    for p in PROBS:
        for rank, site in ((0, 0), (3, 2)):
            want = torch.from_numpy(DR.apply(x[:, :cols].numpy(), p, SEED, rank, site))
            if p == 0:
                assert torch.equal(bits(want), bits(x[:, :cols]))
            for src, aligned in ((xa, True), (xo, False)):
                y = torch.full((rows, ld), SENTINEL, device="cuda") if aligned else offset_rows(rows, ld, fill=SENTINEL)
                L.check(lib.sat_dropout_f32(src.data_ptr(), ld, y.data_ptr(), ld, rows, cols, p, SEED, rank, site, st()), "sat_dropout_f32")
                assert torch.equal(bits(y[:, :cols].cpu()), bits(want)), (p, rank, site, aligned)
                assert bool((y[:, cols:] == SENTINEL).all())
                z = src.clone() if aligned else offset_rows(rows, ld)
                z.copy_(src)
                L.check(lib.sat_dropout_f32(z.data_ptr(), ld, z.data_ptr(), ld, rows, cols, p, SEED, rank, site, st()), "sat_dropout_f32")
                assert torch.equal(bits(z[:, :cols].cpu()), bits(want)), (p, rank, site, aligned, "in place")
                assert torch.equal(bits(z[:, cols:].cpu()), bits(x[:, cols:]))
    # another leading dimension on each side (and so a source the 16-byte path cannot take when ld is odd)
    y = torch.full((rows, ld + 3), SENTINEL, device="cuda")
    L.check(lib.sat_dropout_f32(xa.data_ptr(), ld, y.data_ptr(), ld + 3, rows, cols, 0.5, SEED, 1, 7, st()), "sat_dropout_f32")
    assert torch.equal(bits(y[:, :cols].cpu()), bits(torch.from_numpy(DR.apply(x[:, :cols].numpy(), 0.5, SEED, 1, 7))))
    assert bool((y[:, cols:] == SENTINEL).all())


def test_kernel_bad_arguments_write_nothing():
    lib = L.load()
    x = torch.randn(4, 8, device="cuda")
    y = torch.full((4, 8), SENTINEL, device="cuda")
    a, b = x.data_ptr(), y.data_ptr()
    for p in (-0.1, 1.0, float("nan"), float("inf")):
        assert lib.sat_dropout_f32(a, 8, b, 8, 4, 8, p, SEED, 0, 0, st()) == 1001
    for args in ((a, 8, b, 8, -1, 8), (a, 8, b, 8, 4, -1), (a, 7, b, 8, 4, 8), (a, 8, b, 7, 4, 8), (None, 8, b, 8, 4, 8), (a, 8, None, 8, 4, 8)):
        assert lib.sat_dropout_f32(*args, 0.5, SEED, 0, 0, st()) == 1001, args
    assert lib.sat_dropout_f32(a, 8, b, 8, 4, 8, 0.5, SEED, -1, 0, st()) == 1001
    assert lib.sat_dropout_f32(a, 8, b, 8, 4, 8, 0.5, SEED, 0, -1, st()) == 1001
    assert lib.sat_dropout_f32(a, 8, b, 8, 0, 8, 0.5, SEED, 0, 0, st()) == 0
    assert lib.sat_dropout_f32(a, 8, b, 8, 4, 0, 0.5, SEED, 0, 0, st()) == 0
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ 2, 3. Show-and-Tell
B, E, H, V = 5, 12, 20, 37
CAP_LENGTHS = [7, 5, 5, 3, 2]          # captions <start> .. <end>: the decoder's lengths are [6, 4, 4, 2, 1] (train.py:134)
DEC_CASES = {1: (0.5, 0.0), 2: (0.5, 0.3)}          # num_layers -> (dropout_p, lstm_dropout_p)
_REF = {}


def dec_inputs():
    g = torch.Generator().manual_seed(21)
    caps = torch.zeros(B, CAP_LENGTHS[0], dtype=torch.long)
    for b, l in enumerate(CAP_LENGTHS):
        caps[b, 0], caps[b, l - 1] = 1, 2
        if l > 2:
            caps[b, 1:l - 1] = torch.randint(4, V, (l - 2,), generator=g)
    return torch.randn(B, E, generator=g), caps


def dec_params(Lh):
    return OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(40 + Lh))


def dec_reference(Lh, seed):
    """the float64 reference of case Lh for the masks of `seed` (computed once: the autograd and TrainStep tests draw the same
    seed from the same torch.manual_seed)"""
    if (Lh, seed) not in _REF:
        feats, caps = dec_inputs()
        l1 = [l - 1 for l in CAP_LENGTHS]
        targets = OD.pack_time_major(caps[:, 1:], l1)
        masks = DR.decoder_masks(seed, 0, sum(l1), H, Lh, *DEC_CASES[Lh])
        _REF[(Lh, seed)] = DR.decoder_loss_and_grads(dec_params(Lh), feats, caps[:, :-1], l1, targets, Lh, masks)
    return _REF[(Lh, seed)]


def check_decoder_grads(ref, d_feat, grads):
    np.testing.assert_allclose(d_feat.cpu().numpy(), ref["d_features"].numpy(), rtol=2e-3, atol=2e-7, err_msg="features")
    for k, g in grads.items():
        np.testing.assert_allclose(g.cpu().numpy(), ref["grads"][k].numpy(), rtol=2e-3, atol=2e-7, err_msg=k)


@pytest.mark.parametrize("Lh", [1, 2])
def test_decoder_autograd_path_vs_reference_fed_the_masks(Lh):
    """logits, features.grad and every parameter gradient at test_decoder_odd_shapes_ragged_vs_oracle's tolerances"""
    feats, caps = dec_inputs()
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(dec_params(Lh))
    dec.cuda().train()
    dec.dropout_p, dec.lstm_dropout_p = DEC_CASES[Lh]
    fd, cd = feats.cuda().requires_grad_(True), caps.cuda()
    targets, l1 = sat.pack_targets(cd, CAP_LENGTHS)
    torch.manual_seed(77)
    out = dec(fd, cd[:, :-1], l1)
    ref = dec_reference(Lh, dec.last_dropout_seed)
    assert float((ref["tapes"][Lh] == 0).double().mean()) > 0.3             # the mask did drop
    print("logits: max abs error %.3g" % (out.detach().cpu().double() - ref["logits"]).abs().max().item())
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref["logits"].numpy(), rtol=0, atol=2e-5)
    loss = F.cross_entropy(out, targets)
    assert abs(loss.item() - ref["loss"].item()) < 1e-4
    loss.backward()
    check_decoder_grads(ref, fd.grad, {k: p.grad for k, p in dec.named_parameters()})


def test_rows_the_mask_zeroed_send_exactly_zero_back():
    """one-step captions, H = 4: about one row in 16 loses all four hidden units.  Its logits are the bias alone, and its dH --
    and with it the row's d(gates) and features.grad -- must be EXACTLY zero: the backward masked dH = dlogits W with the forward's
    mask.  (Without the backward's call those rows carry the full gradient.)"""
    Bq, Eq, Hq, Vq = 64, 8, 4, 11
    g = torch.Generator().manual_seed(3)
    dec = sat.DecoderRNN(Eq, Hq, Vq, 1)
    dec.load_state_dict(OD.init_decoder_params(Eq, Hq, Vq, 1, generator=g))
    dec.cuda().train()
    dec.dropout_p = 0.5
    fd = torch.randn(Bq, Eq, generator=g).cuda().requires_grad_(True)
    caps = torch.ones(Bq, 1, dtype=torch.long, device="cuda")
    torch.manual_seed(5)
    out = dec(fd, caps, [1] * Bq)
    keep = torch.from_numpy(DR.keep(dec.last_dropout_seed, 0, 1, Bq, Hq, 0.5))
    gone = ~keep.any(1)
    assert 1 <= int(gone.sum()) < Bq // 2, int(gone.sum())
    assert torch.equal(out.detach().cpu()[gone], dec.linear.bias.detach().cpu().expand(int(gone.sum()), Vq))
    F.cross_entropy(out, torch.randint(0, Vq, (Bq,), generator=g).cuda()).backward()
    gf = fd.grad.cpu()
    assert bool((gf[gone] == 0).all())
    assert bool((gf[~gone].abs().sum(1) > 0).all())


def ts_model(Lh, dtype):
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY, compute_dtype=dtype)
    model.decoder.load_state_dict(dec_params(Lh))
    model.cuda().train()
    model.decoder.dropout_p, model.decoder.lstm_dropout_p = DEC_CASES[Lh]
    return model


@pytest.mark.parametrize("Lh", [1, 2])
def test_trainstep_f32_vs_the_same_reference(Lh):
    """`TrainStep.forward_backward` on cached [B, E] features: the same torch.manual_seed draws the same masks as the autograd
    path's forward, and loss and flat-buffer gradients meet the same reference at the same tolerances"""
    feats, caps = dec_inputs()
    model = ts_model(Lh, "f32")
    ts = sat.TrainStep(model)
    assert ts.decoder_gemm_dtype == "f32"
    n_tok = sum(l - 1 for l in CAP_LENGTHS)
    torch.manual_seed(77)
    loss = ts.forward_backward((feats.cuda(), caps.cuda(), CAP_LENGTHS), 1.0 / n_tok).clone()
    seed = model.decoder.last_dropout_seed
    torch.manual_seed(77)
    assert seed == sat.models.draw_ss_seed()
    ref = dec_reference(Lh, seed)
    assert abs(loss.item() - ref["loss"].item()) < 1e-4
    check_decoder_grads(ref, ts.last_d_features, {k: ts.flat.grad("decoder." + k) for k, _ in model.decoder.named_parameters()})
    assert torch.equal(ts.last_dropped_tape.cpu() == 0, ref["tapes"][Lh] == 0)


@pytest.mark.parametrize("Lh", [1, 2])
def test_trainstep_bf16_mode_has_the_same_masks(Lh):
    """decoder_gemm_dtype = "bf16": the masks depend on the seed only, so the zero pattern of the dropped top tape equals the
    reference mask.  The loss: no existing test compares the two modes at these shapes, so both bounds the suite applies to the
    bf16 mode at dropout 0 hold here -- within 1e-4 of the same engine's exact-f32 loss under the same masks
    (tests/test_gpu_parity.py::test_cfg2_full_size_properties: "the CE moves by < 1e-4") and within 2e-3 of the exact reference
    (tests/test_gpu_ss.py::test_trainstep_bf16_cfg1_shape_reproducible_and_learns)."""
    feats, caps = dec_inputs()
    model = ts_model(Lh, "bf16")
    ts = sat.TrainStep(model)
    assert ts.decoder_gemm_dtype == "bf16"
    n_tok = sum(l - 1 for l in CAP_LENGTHS)
    batch = (feats.cuda(), caps.cuda(), CAP_LENGTHS)
    torch.manual_seed(77)
    loss = ts.forward_backward(batch, 1.0 / n_tok).clone()
    seed = model.decoder.last_dropout_seed
    ref = dec_reference(Lh, seed)
    keep = torch.from_numpy(DR.keep(seed, 0, Lh, n_tok, H, DEC_CASES[Lh][0]))
    assert torch.equal(ts.last_dropped_tape.cpu() != 0, keep)
    ts.decoder_gemm_dtype = "f32"
    torch.manual_seed(77)
    l32 = ts.forward_backward(batch, 1.0 / n_tok).clone()
    assert model.decoder.last_dropout_seed == seed
    print("bf16 loss %.7f, f32 loss %.7f, reference %.7f" % (loss.item(), l32.item(), ref["loss"].item()))
    assert abs(loss.item() - l32.item()) < 1e-4
    assert abs(loss.item() - ref["loss"].item()) < 2e-3


# ------------------------------------------------------------------------------------------------------ 4. Show-Attend-Tell
# (the issue's sizes with hidden = embed + context = 20: the LSTMCell input is cat[embedding, context], model2.py:57-58)
AB, AP, AC, AE, AH, AV = 4, 6, 8, 12, 20, 29
A_CAP_LENGTHS = [6, 4, 4, 2]           # the decoder's lengths are [5, 3, 3, 1]


def attend_case():
    g = torch.Generator().manual_seed(31)
    params = OA.init_attend_params(AH, AC, AV, AE, generator=g, feat=AC)
    feats = torch.randn(AB, AP, AC, generator=g)
    caps = torch.randint(0, AV, (AB, A_CAP_LENGTHS[0]), generator=g)
    l1 = [l - 1 for l in A_CAP_LENGTHS]
    return params, feats, caps, l1, OD.pack_time_major(caps[:, 1:], l1)


def attend_model(params):
    model = sat.ShowAttendTellModel(AH, AC, AV, AE, None, feature_size=(AP, AC), compute_dtype="f32", vgg_cfg=[AC])
    model.load_state_dict(params, strict=False)
    return model.cuda().train()


@pytest.mark.parametrize("alpha_c", [0.0, 1.0])
def test_attend_model_vs_reference_fed_the_mask(alpha_c):
    """logits and all decoder gradients at the tolerances of tests/test_gpu_attend.py::test_attend_decoder_matches_reference_goldens
    (logits atol 2e-5, CE 1e-4, gradients rtol 2e-3 / atol 2e-7), the decoder fed features directly; once more with the doubly
    stochastic penalty, whose value and `last_alphas` must not notice the mask's presence"""
    params, feats, caps, l1, targets = attend_case()
    model = attend_model(params)
    model.dropout_p, model.alpha_c = 0.5, alpha_c
    fd = feats.cuda()
    torch.manual_seed(99)
    out = model.decode(fd, fd.mean(1), caps[:, :-1].cuda(), l1)
    N = sum(l1)
    mask = DR.multiplier(model.last_dropout_seed, 0, 0, N, AE, 0.5)
    assert 0.25 < float((mask == 0).double().mean()) < 0.75
    ref = DR.attend_loss_and_grads(params, feats, caps[:, :-1], l1, targets, mask, alpha_c)
    print("logits: max abs error %.3g" % (out.detach().cpu().double() - ref["logits"]).abs().max().item())
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref["logits"].numpy(), rtol=0, atol=2e-5)
    ce = F.cross_entropy(out, targets.cuda())
    assert abs(ce.item() - ref["ce"].item()) < 1e-4
    np.testing.assert_allclose(model.last_alphas.cpu().numpy(), ref["alphas"].numpy(), rtol=0, atol=2e-5)
    pen = model.last_attention_penalty
    if alpha_c:
        assert abs(pen.item() - ref["penalty"].item()) <= 1e-5 * ref["penalty"].item()
        (ce + pen).backward()
    else:
        assert pen is None
        ce.backward()
    named = dict(model.named_parameters())
    for k in params:
        np.testing.assert_allclose(named[k].grad.cpu().numpy(), ref["grads"][k].numpy(), rtol=2e-3, atol=2e-7, err_msg=k)
    assert all(p.grad is None for p in model.encoder.parameters())


def test_attend_finetune_gets_feature_gradients_with_dropout_on():
    """finetune(allow=True) hands the conv stack a gradient through the dropped output layer: the features' gradient (what the
    stack's backward starts from) equals float64 autograd on the reference fed the mask"""
    params, feats, caps, l1, targets = attend_case()
    model = attend_model(params)
    model.dropout_p = 0.5
    fd = feats.cuda().requires_grad_(True)
    torch.manual_seed(99)
    out = model.decode(fd, fd.mean(1), caps[:, :-1].cuda(), l1)
    F.cross_entropy(out, targets.cuda()).backward()
    mask = DR.multiplier(model.last_dropout_seed, 0, 0, sum(l1), AE, 0.5)
    f64 = feats.double().requires_grad_(True)
    p64 = {k: v.double() for k, v in params.items()}
    emb, h_c = p64["embedding.weight"][caps[:, :-1]], OA.init_lstm(p64, f64)
    h, c = h_c
    enc, outs, r0 = f64 @ p64["image_att_w"], [], 0
    for t, bs in enumerate(OA.batch_sizes(l1)):
        context, _ = OA.attention_layer(p64, f64[:bs], enc[:bs], h[:bs])
        h, c = OA.lstmcell(p64, torch.cat([emb[:bs, t], context], 1), h[:bs], c[:bs])
        z = context @ p64["context2out.weight"].t() + p64["context2out.bias"] + h @ p64["hidden2tout.weight"].t() + p64["hidden2tout.bias"]
        outs.append((z * mask[r0:r0 + bs]) @ p64["classifier.weight"].t() + p64["classifier.bias"])
        r0 += bs
    F.cross_entropy(torch.cat(outs, 0), targets).backward()
    np.testing.assert_allclose(fd.grad.cpu().numpy(), f64.grad.numpy(), rtol=2e-3, atol=2e-7)


# ------------------------------------------------------------------------------------------------------ 5. switches
def test_switches_decoder():
    feats, caps = dec_inputs()
    params = dec_params(2)
    fd, cd = feats.cuda(), caps.cuda()
    targets, l1 = sat.pack_targets(cd, CAP_LENGTHS)

    def run(dec, seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        f = fd.clone().requires_grad_(True)
        dec.zero_grad()
        out = dec(f, cd[:, :-1], l1)
        F.cross_entropy(out, targets).backward()
        return [out.detach().clone(), f.grad.clone()] + [p.grad.clone() for p in dec.parameters()]

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    fresh = sat.DecoderRNN(E, H, V, 2)
    fresh.load_state_dict(params)
    base = run(fresh.cuda().train())
    dec = sat.DecoderRNN(E, H, V, 2)
    dec.load_state_dict(params)
    dec.cuda()
    state = torch.get_rng_state()
    dec.dropout_p, dec.lstm_dropout_p = 0.5, 0.5
    assert same(run(dec.eval()), base)                                 # eval mode with 0.5 is probability 0
    dec.dropout_p = dec.lstm_dropout_p = 0.0
    assert same(run(dec.train()), base)                                # train mode with zeros is a model that never had them
    assert torch.equal(torch.get_rng_state(), state) and dec.last_dropout_seed is None
    dec.dropout_p, dec.lstm_dropout_p = 0.5, 0.3
    a, b, c = run(dec, 11), run(dec, 11), run(dec, 12)
    assert same(a, b) and not torch.equal(a[0], c[0]) and not torch.equal(a[0], base[0])
    assert not torch.equal(torch.get_rng_state(), state)
    ids = dec.eval().sample(fd)
    assert torch.equal(ids, fresh.eval().sample(fd))                   # the decode paths never drop


def test_switches_attend_model_and_trainstep():
    params, feats, caps, l1, targets = attend_case()
    fd, cd = feats.cuda(), caps[:, :-1].cuda()
    fresh, model = attend_model(params), attend_model(params)
    base = fresh.decode(fd, fd.mean(1), cd, l1).detach().clone()
    state = torch.get_rng_state()
    model.dropout_p = 0.5
    assert torch.equal(model.eval().decode(fd, fd.mean(1), cd, l1).detach(), fresh.eval().decode(fd, fd.mean(1), cd, l1).detach())
    model.dropout_p = 0.0
    assert torch.equal(model.train().decode(fd, fd.mean(1), cd, l1).detach(), base)
    assert torch.equal(torch.get_rng_state(), state) and model.last_dropout_seed is None
    model.dropout_p = 0.5
    outs = []
    for s in (11, 11, 12):
        torch.manual_seed(s)
        outs.append(model.decode(fd, fd.mean(1), cd, l1).detach().clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], base)
    assert torch.equal(model.eval().sample_features(fd), fresh.eval().sample_features(fd))
    # TrainStep: zeros launch and draw what a model without the attributes does
    dfeats, dcaps = dec_inputs()
    n_tok = sum(l - 1 for l in CAP_LENGTHS)
    batch = (dfeats.cuda(), dcaps.cuda(), CAP_LENGTHS)
    ts0, ts1 = sat.TrainStep(ts_model(1, "f32")), sat.TrainStep(ts_model(1, "f32"))
    ts0.model.decoder.dropout_p = 0.0
    state = torch.get_rng_state()
    l0 = ts0.forward_backward(batch, 1.0 / n_tok).clone()
    assert torch.equal(torch.get_rng_state(), state) and ts0.last_dropped_tape is None
    torch.manual_seed(11)
    l1a, g1a = ts1.forward_backward(batch, 1.0 / n_tok).clone(), ts1.flat_grad.clone()
    torch.manual_seed(11)
    l1b, g1b = ts1.forward_backward(batch, 1.0 / n_tok).clone(), ts1.flat_grad.clone()
    assert torch.equal(l1a, l1b) and torch.equal(g1a, g1b) and not torch.equal(l1a, l0)
    ts1.model.decoder.dropout_p = 0.0
    l1c = ts1.forward_backward(batch, 1.0 / n_tok).clone()
    assert torch.equal(l1c, l0) and torch.equal(ts1.flat_grad[:ts1.flat.n], ts0.flat_grad[:ts0.flat.n])
