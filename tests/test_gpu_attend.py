"""GPU (MI355X): Show-Attend-Tell (`/root/reference/model2.py`, the model train.py:37 constructs) on the HIP path against
(a) goldens produced by the reference class's own methods (tests/golden/G6, G7), (b) the CPU oracle (`oracle/attend.py`),
kernel by kernel and end to end."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import attend as OA  # noqa: E402


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def st():
    return L.stream()


def test_attention_fwd_bwd_kernels_vs_fp64():
    lib = L.load()
    g = torch.Generator().manual_seed(3)
    B, P, C = 5, 196, 512
    ce, fe = torch.randn(B, P, C, generator=g) * 0.5, torch.randn(B, P, C, generator=g).clamp(min=0)
    proj, w = torch.randn(B, C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.1
    dctx = torch.randn(B, C, generator=g)
    ce64, fe64, pj64, w64 = (t.double().requires_grad_(True) for t in (ce, fe, proj, w))
    hatt = torch.tanh(ce64 + pj64[:, None, :])
    alpha = torch.softmax(hatt @ w64, dim=1)
    ctx = (fe64 * alpha[:, :, None]).mean(1)
    ctx.backward(dctx.double())
    d = [t.cuda() for t in (ce, fe, proj, w, dctx)]
    al, co = torch.empty(B, P, device="cuda"), torch.full((B, C + 8), float("nan"), device="cuda")
    ws = torch.empty(lib.sat_attention_ws_bytes(B, P) // 4, device="cuda")
    L.check(lib.sat_attention_fwd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), C, d[3].data_ptr(), B, P, C, al.data_ptr(),
                                  co.data_ptr() + 16, C + 8, ws.data_ptr(), ws.numel() * 4, st()))
    torch.cuda.synchronize()
    np.testing.assert_allclose(al.cpu().numpy(), alpha.detach().numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose(co[:, 4:4 + C].cpu().numpy(), ctx.detach().numpy(), rtol=0, atol=2e-7)
    assert torch.isnan(co[:, :4]).all() and torch.isnan(co[:, 4 + C:]).all()          # strided destination: nothing else written
    dce = torch.ones(B, P, C, device="cuda")                                           # accumulates INTO the buffer
    dpj, dwp = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
    dfe = torch.zeros(B, P, C, device="cuda")
    half = (d[4] * 0.25).contiguous()                                                   # d_ctx arrives as the sum of two addends
    rest = (d[4] - half).contiguous()
    L.check(lib.sat_attention_bwd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), C, d[3].data_ptr(), al.data_ptr(), half.data_ptr(), C,
                                  rest.data_ptr(), C, B, P, C, dce.data_ptr(), dpj.data_ptr(), dwp.data_ptr(), dfe.data_ptr(), ws.data_ptr(),
                                  ws.numel() * 4, st()))
    torch.cuda.synchronize()
    np.testing.assert_allclose(dce.cpu().numpy() - 1.0, ce64.grad.numpy(), rtol=0, atol=3e-7)
    np.testing.assert_allclose(dpj.cpu().numpy(), pj64.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dwp.sum(0).cpu().numpy(), w64.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dfe.cpu().numpy(), fe64.grad.numpy(), rtol=1e-4, atol=1e-8)       # fine-tuning: gradient into the features
    assert lib.sat_attention_fwd(None, None, None, C, None, B, P, C, None, None, C, None, 0, st()) == 1001
    assert lib.sat_attention_fwd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), C, d[3].data_ptr(), B, P, C, None, co.data_ptr(), C + 8,
                                 None, 0, st()) == 1002        # workspace missing


@pytest.mark.parametrize("dtype", [L.SAT_F32, L.SAT_BF16])
def test_maxpool2_and_row_utilities(dtype):
    lib = L.load()
    td = torch.bfloat16 if dtype == L.SAT_BF16 else torch.float32
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 6, 10, 16, generator=g).to(td)
    xd, out = x.cuda(), torch.empty(3, 3, 5, 16, device="cuda", dtype=td)
    o = L.SatOp()
    o.kind, o.dtype = L.OP_MAXPOOL2, dtype
    o.in0, o.out = xd.data_ptr(), out.data_ptr()
    o.N, o.Hin, o.Win, o.Cout = 3, 6, 10, 16
    import ctypes as C
    L.check(lib.sat_run_ops(C.pointer(o), 1, st()))
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(out.float().cpu(), ref)
    if dtype == L.SAT_BF16:
        return
    table, ids = torch.randn(50, 12, generator=g), torch.randint(0, 50, (7, 3), generator=g)
    td_, idd = table.cuda(), ids.cuda()
    dst = torch.zeros(7, 20, device="cuda")
    L.check(lib.sat_rows_copy(td_.data_ptr(), 12, idd.data_ptr() + 8, 3, 50, 7, 12, dst.data_ptr() + 16, 20, st()))
    assert torch.equal(dst[:, 4:16].cpu(), table[ids[:, 1]]) and float(dst[:, :4].abs().sum()) == 0
    a, b = torch.randn(7, 12, generator=g), torch.randn(7, 12, generator=g)
    ad, bd, od = a.cuda(), b.cuda(), torch.empty(7, 12, device="cuda")
    L.check(lib.sat_rows_add(ad.data_ptr(), 12, bd.data_ptr(), 12, 7, 12, od.data_ptr(), 12, st()))
    assert torch.equal(od.cpu(), a + b)
    acc = torch.ones(12, device="cuda")
    L.check(lib.sat_rows_sum(ad.data_ptr(), 12, 7, 12, acc.data_ptr(), 1, st()))
    np.testing.assert_allclose(acc.cpu().numpy(), (1 + a.double().sum(0)).numpy(), rtol=1e-5, atol=2e-6)
    rows, tok = torch.randn(40, 8, generator=g), torch.randint(0, 9, (40,), generator=g)
    rd, tkd, tab = rows.cuda(), tok.cuda(), torch.full((9, 8), float("nan"), device="cuda")
    L.check(lib.sat_scatter_rows_add(rd.data_ptr(), tkd.data_ptr(), 40, 8, 9, tab.data_ptr(), st()))
    np.testing.assert_allclose(tab.cpu().double().numpy(), torch.zeros(9, 8, dtype=torch.float64).index_add_(0, tok, rows.double()).numpy(), atol=1e-5)


def _model_from_golden(g):
    hidden, context, vocab, embed, B, T, P, feat = [int(x) for x in g["dims"]]
    params = OA.init_attend_params(hidden, context, vocab, embed, generator=torch.Generator().manual_seed(int(g["seed"])), feat=feat)
    cfg = [8, "M", feat]                     # a tiny stand-in conv stack ending in `feat` channels (the goldens pin the decoder half)
    model = sat.ShowAttendTellModel(hidden, context, vocab, embed, None, feature_size=(P, feat), compute_dtype="f32", vgg_cfg=cfg)
    model.load_state_dict(params, strict=False)
    return model.cuda(), params, (hidden, context, vocab, embed, B, T, P, feat)


@pytest.mark.parametrize("name", ["G6_attend_small.npz", "G7_attend_vgg_dims.npz"])
def test_attend_decoder_matches_reference_goldens(golden_dir, name):
    """train.py:134-144 on the decoder half: logits, CE (within 1e-4), every gradient, and the 20-step greedy ids bit-exact"""
    g = load(golden_dir, name)
    model, params, (hidden, context, vocab, embed, B, T, P, feat) = _model_from_golden(g)
    feats = torch.from_numpy(g["features"]).cuda()
    caps = torch.from_numpy(g["captions"]).cuda()
    lengths = [int(x) for x in g["lengths"]]
    targets, l1 = sat.pack_targets(caps, lengths)
    assert np.array_equal(targets.cpu().numpy(), g["targets"])
    model.zero_grad()
    out = model.decode(feats, feats.mean(1), caps[:, :-1], l1)
    if "argmax" in g:
        np.testing.assert_allclose(out[:, :64].detach().cpu().numpy(), g["logits"], rtol=0, atol=2e-5)
        assert np.array_equal(out.argmax(1).cpu().numpy(), g["argmax"])
    else:
        np.testing.assert_allclose(out.detach().cpu().numpy(), g["logits"], rtol=0, atol=2e-5)
    loss = torch.nn.CrossEntropyLoss()(out, targets)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    named = dict(model.named_parameters())
    for k in params:
        got = named[k].grad.cpu()
        if "grad." + k in g:
            np.testing.assert_allclose(got.numpy(), g["grad." + k], rtol=2e-3, atol=2e-7, err_msg=k)
        else:
            assert abs(got.double().norm().item() - float(g["gradnorm." + k])) < 2e-3 * float(g["gradnorm." + k]) + 1e-8, k
            gk = got.flatten()
            np.testing.assert_allclose(gk[::max(1, gk.numel() // 512)][:512].numpy(), g["gradsample." + k], rtol=2e-3, atol=2e-7, err_msg=k)
    assert all(p.grad is None for p in model.encoder.parameters())           # frozen (model2.py:17)
    ids0 = model.sample_features(feats, None)
    assert np.array_equal(ids0.cpu().numpy(), g["sample_ids_zero_state"])
    h0, c0 = OA.init_lstm(params, torch.from_numpy(g["features"]))
    ids1 = model.sample_features(feats, (h0.cuda(), c0.cuda()))
    assert np.array_equal(ids1.cpu().numpy(), g["sample_ids_init_state"])
    assert np.array_equal(model.sample_features(feats, torch.stack([h0, c0]).cuda()).cpu().numpy(), g["sample_ids_init_state"])   # eval.py:89


SMALL_VGG = [16, 16, "M", 32, "M", 64, 64, "M", 64]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_vgg_stack_vs_oracle(dtype):
    g = torch.Generator().manual_seed(9)
    vp = OA.init_vgg_params(g, cfg=SMALL_VGG)
    model = sat.ShowAttendTellModel(64 + 32, 64, 100, 32, None, feature_size=(16, 64), compute_dtype=dtype, vgg_cfg=SMALL_VGG)
    model.load_state_dict(vp, strict=False)
    model.cuda()
    x = torch.randn(5, 3, 32, 32, generator=g)
    feats, fmean = model._encode(x.cuda())
    ref = OA.vgg_forward(vp, x, cfg=SMALL_VGG)
    assert feats.shape == ref.shape == (5, 16, 64)
    if dtype == "f32":
        np.testing.assert_allclose(feats.cpu().numpy(), ref.numpy(), rtol=0, atol=2e-5)
    else:
        ref_bf = OA.vgg_forward(vp, x, cfg=SMALL_VGG, bf16_storage=True)
        assert ((feats.cpu() - ref_bf).norm() / ref_bf.norm()).item() < 0.01
        assert ((feats.cpu() - ref).norm() / ref.norm()).item() < 0.03
    np.testing.assert_allclose(fmean.cpu().numpy(), feats.mean(1).cpu().numpy(), rtol=0, atol=1e-5)


@pytest.mark.timeout(900)
def test_vgg16_full_stack_f32_and_bf16_vs_oracle_224():
    """the real 12-conv `features[:-3]` at 224x224 (batch 2): [B,196,512] features, f32 MFMA vs the CPU oracle; bf16 vs the
    bf16-storage oracle"""
    g = torch.Generator().manual_seed(10)
    vp = OA.init_vgg_params(g)
    x = torch.randn(2, 3, 224, 224, generator=g)
    ref = OA.vgg_forward(vp, x)
    ref_bf = OA.vgg_forward(vp, x, bf16_storage=True)
    for dtype in ("f32", "bf16"):
        model = sat.ShowAttendTellModel(1024, 512, 1000, 512, None, compute_dtype=dtype)
        model.load_state_dict(vp, strict=False)
        model.cuda()
        feats, _ = model._encode(x.cuda())
        assert feats.shape == (2, 196, 512)
        if dtype == "f32":
            assert (feats.cpu() - ref).abs().max().item() < 2e-3 * max(1.0, ref.abs().max().item())
        else:
            r = ((feats.cpu() - ref_bf).norm() / ref_bf.norm()).item()
            print("VGG16 bf16 vs bf16-storage oracle rel-L2 %.4f (vs f32 oracle %.4f)" % (r, ((feats.cpu() - ref).norm() / ref.norm()).item()))
            assert r < 0.02


def test_full_model_drop_in_training_loop_and_sample():
    """model(images, captions, lengths) / CE / loss.backward() / clamp / torch Adam exactly as train.py:134-146 drives the model
    it constructs at train.py:37, then model.sample(images, state) as eval.py:99; f32 mode against the oracle end to end"""
    g = torch.Generator().manual_seed(12)
    hidden, embed, vocab, B, T = 64 + 32, 32, 120, 6, 9
    vp = OA.init_vgg_params(g, cfg=SMALL_VGG)
    dp = OA.init_attend_params(hidden, 64, vocab, embed, generator=g, feat=64)
    model = sat.ShowAttendTellModel(hidden, 64, vocab, embed, None, feature_size=(16, 64), compute_dtype="f32", vgg_cfg=SMALL_VGG)
    sd = dict(vp)
    sd.update(dp)
    model.load_state_dict(sd)
    model.cuda()
    assert sorted(model.state_dict().keys()) == sorted(sd.keys())
    images = torch.randn(B, 3, 32, 32, generator=g)
    lengths = [9, 9, 7, 6, 4, 3]
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, vocab, (l - 2,), generator=g)
        caps[b, l - 1] = 2
    feats = OA.vgg_forward(vp, images, cfg=SMALL_VGG)
    ref_loss, ref_grads, ref_logits = OA.attend_loss_and_grads(dp, feats, caps, lengths)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)      # train.py:55-56
    assert len(opt.param_groups[0]["params"]) == 19
    di, dc = images.cuda(), caps.cuda()
    targets, l1 = sat.pack_targets(dc, lengths)
    losses = []
    for it in range(4):
        model.zero_grad()
        out = model(di, dc[:, :-1], l1)
        loss = torch.nn.CrossEntropyLoss()(out, targets)
        loss.backward()
        if it == 0:
            np.testing.assert_allclose(out.detach().cpu().numpy(), ref_logits.numpy(), rtol=0, atol=5e-5)
            assert abs(loss.item() - ref_loss.item()) < 1e-4
            named = dict(model.named_parameters())
            for k in dp:
                np.testing.assert_allclose(named[k].grad.cpu().numpy(), ref_grads[k].numpy(), rtol=5e-3, atol=5e-7, err_msg=k)
        for p in opt.param_groups[0]["params"]:
            p.grad.data.clamp_(-0.1, 0.1)
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0]
    ids = model.eval().sample(di, None)
    assert ids.shape == (B, 20) and ids.dtype == torch.int64 and int(ids.min()) >= 0 and int(ids.max()) < vocab
    cur = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith("encoder.")}
    assert torch.equal(ids.cpu(), OA.attend_sample(cur, feats, None))
    with pytest.raises(ValueError):
        sat.ShowAttendTellModel(100, 512, 50, 32)           # hidden != embed + 512


def test_collate_on_device_equals_the_reference_collate_contract():
    """data_loader.py:48-62: sort by caption length (longest first, ties in dataset order), stack, zero-pad -- with the
    permute / pad done by HIP kernels on tensors already in HBM; must equal the host `collate_batch`"""
    g = torch.Generator().manual_seed(21)
    lens = [5, 9, 3, 9, 1, 7, 5]
    samples = [(torch.randn(3, 8, 10, generator=g), torch.randint(1, 50, (l,), generator=g), "img%d" % i) for i, l in enumerate(lens)]
    ref_im, ref_caps, ref_len, ref_ids = sat.collate_batch(samples)
    images = torch.stack([s[0] for s in samples]).cuda()
    flat = torch.cat([s[1] for s in samples]).cuda()
    im, caps, ln, ids = sat.collate_on_device(images, flat, lens, [s[2] for s in samples])
    assert ln == ref_len and ids == ref_ids
    assert torch.equal(caps.cpu(), ref_caps) and torch.equal(im.cpu(), ref_im)
    with pytest.raises(ValueError):
        sat.collate_on_device(images, flat, lens[:-1] + [2])


def test_finetune_conv_stack_backward_vs_oracle_autograd():
    """`finetune(allow=True)` (model2.py:87-89): gradients of every conv weight / bias of the stack (dgrad through the forward conv
    kernel on flipped weights, wgrad as split-K GEMMs over the flat zero-bordered pixel index, ReLU mask, max-pool routing,
    the three paths by which the decoder reaches the features) against torch autograd through the CPU oracle"""
    g = torch.Generator().manual_seed(31)
    hidden, embed, vocab, B, T = 64 + 32, 32, 90, 5, 8
    vp = OA.init_vgg_params(g, cfg=SMALL_VGG)
    dp = OA.init_attend_params(hidden, 64, vocab, embed, generator=g, feat=64)
    model = sat.ShowAttendTellModel(hidden, 64, vocab, embed, None, feature_size=(16, 64), compute_dtype="f32", vgg_cfg=SMALL_VGG)
    sd = dict(vp)
    sd.update(dp)
    model.load_state_dict(sd)
    model.cuda()
    model.finetune(allow=True)
    assert all(p.requires_grad for p in model.encoder.parameters())
    images = torch.randn(B, 3, 32, 32, generator=g)
    lengths = [8, 8, 6, 5, 3]
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, vocab, (l - 2,), generator=g)
        caps[b, l - 1] = 2
    # oracle: autograd through vgg_forward -> attend_forward -> CE
    from oracle import decoder as OD
    q = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    l1 = [l - 1 for l in lengths]
    tg = OD.pack_time_major(caps[:, 1:], l1)
    ref_logits = OA.attend_forward(q, OA.vgg_forward(q, images, cfg=SMALL_VGG), caps[:, :-1], l1)
    ref_loss = F.cross_entropy(ref_logits, tg)
    ref_loss.backward()
    di, dc = images.cuda(), caps.cuda()
    targets, _ = sat.pack_targets(dc, lengths)
    model.zero_grad()
    out = model(di, dc[:, :-1], l1)
    loss = torch.nn.CrossEntropyLoss()(out, targets)
    assert abs(loss.item() - ref_loss.item()) < 1e-4
    loss.backward()
    named = dict(model.named_parameters())
    for k in sd:
        got, ref = named[k].grad.cpu(), q[k].grad
        scale = ref.abs().max().item() + 1e-12
        assert (got - ref).abs().max().item() < 3e-3 * scale + 1e-8, (k, (got - ref).abs().max().item(), scale)
    # a second forward before the backward would overwrite the tapes: refused, not silently wrong
    out1 = model(di, dc[:, :-1], l1)
    model(di, dc[:, :-1], l1)
    with pytest.raises(RuntimeError):
        out1.sum().backward()
    model.finetune(allow=False)
    assert not any(p.requires_grad for p in model.encoder.parameters())
    # bf16 fine-tuning (mixed precision, f32 master weights): same loss to bf16 tolerance; decoder gradients within 3 % rel-L2 of
    # the f32 oracle, conv gradients aligned with it (cosine > 0.97; their rel-L2 grows towards the input -- bf16 activations flip
    # ReLU masks near zero and every input-gradient conv rounds once more: 16 % at the first conv of this He-init stack)
    bf = sat.ShowAttendTellModel(hidden, 64, vocab, embed, None, feature_size=(16, 64), compute_dtype="bf16", vgg_cfg=SMALL_VGG)
    bf.load_state_dict(sd)
    bf.cuda()
    bf.finetune(allow=True)
    bf.zero_grad()
    out16 = bf(di, dc[:, :-1], l1)
    loss16 = torch.nn.CrossEntropyLoss()(out16, targets)
    assert abs(loss16.item() - ref_loss.item()) < 2e-2
    loss16.backward()
    named16 = dict(bf.named_parameters())
    for k in sd:
        got, ref = named16[k].grad.cpu(), q[k].grad
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        rel = ((got - ref).norm() / (ref.norm() + 1e-12)).item()
        cos = torch.nn.functional.cosine_similarity(got.flatten().double(), ref.flatten().double(), dim=0).item()
        print("bf16 fine-tune grad %-28s rel-L2 %.4f cos %.5f" % (k, rel, cos))
        if k.startswith("encoder."):
            assert rel < 0.25 and cos > 0.97, (k, rel, cos)
        else:
            assert rel < 0.03, (k, rel)


def test_prefetched_features_are_the_features():
    """ShowAttendTellModel.prefetch_features: the frozen stack of a later batch on a side stream gives bit-identical logits."""
    torch.manual_seed(3)
    m = sat.ShowAttendTellModel(96, 64, 50, 32, None, feature_size=(16, 64), compute_dtype="bf16", vgg_cfg=SMALL_VGG).cuda()
    g = torch.Generator().manual_seed(1)
    xs = [torch.rand(3, 3, 32, 32, generator=g).cuda() for _ in range(2)]
    caps = torch.randint(1, 50, (3, 6), generator=g).cuda()
    lengths = [6, 4, 3]
    want = [m(x, caps, lengths).detach().clone() for x in xs]
    assert m.prefetch_features(xs[0])
    got0 = m(xs[0], caps, lengths).detach().clone()
    assert m.prefetch_features(xs[1])
    got_other = m(xs[0], caps, lengths).detach().clone()       # not the prefetched tensor: computed for xs[0] ...
    assert len(m._pf_list) == 1                                 # ... and the batch in flight is left alone
    got1 = m(xs[1], caps, lengths).detach().clone()
    assert not m._pf_list
    assert m.prefetch_features(xs[0]) and m.prefetch_features(xs[1]) and not m.prefetch_features(xs[0])   # two in flight
    got1b = m(xs[1], caps, lengths).detach().clone()            # consumed out of order
    got0b = m(xs[0], caps, lengths).detach().clone()
    with torch.no_grad():
        assert m.prefetch_features(xs[0])
        next(iter(m.encoder.parameters())).mul_(0.5)            # weights rewritten: the batch in flight is recomputed
        got_new = m(xs[0], caps, lengths).clone()
        want_new = m(xs[0], caps, lengths).clone()
    torch.cuda.synchronize()
    assert torch.equal(got0, want[0]) and torch.equal(got_other, want[0]) and torch.equal(got1, want[1])
    assert torch.equal(got0b, want[0]) and torch.equal(got1b, want[1]) and torch.equal(got_new, want_new)


@pytest.mark.parametrize("model_zero_grad", [False, True])
def test_fused_clamp_adam_equals_torch_clamp_plus_adam(model_zero_grad):
    """sat.FusedClampAdam = clip_gradient + optim.Adam (train.py:88-91, 145-146) in one launch: same parameters after 3 steps of
    the Show-Attend-Tell drop-in loop as torch's clamp_ + Adam, with `opt.zero_grad()` (gradients accumulate into the flat
    buffer) and with train.py:137's `model.zero_grad()` (fresh gradient tensors, copied in); state dict in torch.optim.Adam layout."""
    def build():
        torch.manual_seed(8)
        return sat.ShowAttendTellModel(96, 64, 50, 32, None, feature_size=(16, 64), compute_dtype="f32", vgg_cfg=SMALL_VGG).cuda()
    g = torch.Generator().manual_seed(2)
    x = torch.rand(4, 3, 32, 32, generator=g).cuda()
    caps = torch.randint(1, 50, (4, 7), generator=g).cuda()
    lengths = [7, 6, 4, 3]
    targets, l1 = sat.pack_targets(caps, lengths)
    crit = torch.nn.CrossEntropyLoss()
    ma, mb = build(), build()
    oa = torch.optim.Adam([p for p in ma.parameters() if p.requires_grad], lr=1e-3)
    ob = sat.FusedClampAdam([p for p in mb.parameters() if p.requires_grad], lr=1e-3, clip=0.1)
    for _ in range(3):
        ma.zero_grad()
        crit(ma(x, caps[:, :-1], l1), targets).backward()
        for p in oa.param_groups[0]["params"]:
            p.grad.data.clamp_(-0.1, 0.1)
        oa.step()
        if model_zero_grad:
            mb.zero_grad()
        else:
            ob.zero_grad()
        crit(mb(x, caps[:, :-1], l1), targets).backward()
        ob.step()
    torch.cuda.synchronize()
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert (pa - pb).abs().max().item() <= 2e-6, n
    sd = ob.state_dict()
    oc = torch.optim.Adam([p for p in build().parameters() if p.requires_grad], lr=1e-3)
    oc.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})      # torch accepts the layout
    ref = oa.state_dict()["state"]
    for i, st in sd["state"].items():
        assert (st["exp_avg"].cpu() - ref[i]["exp_avg"].cpu()).abs().max().item() <= 1e-7
        assert float(st["step"]) == 3.0
    ob2 = sat.FusedClampAdam([p for p in build().parameters() if p.requires_grad], lr=5e-4, clip=0.1)
    ob2.load_state_dict(sd)
    assert ob2.step_count == 3 and ob2.param_groups[0]["lr"] == 1e-3 and torch.equal(ob2.exp_avg, ob.exp_avg)


def test_finetune_with_fused_clamp_adam_sees_every_weight_update():
    """`finetune(allow=True)` + `FusedClampAdam` (parameters re-homed, updated through raw pointers, version counters
    once untouched) trained against the FIRST step's kernel-layout conv weights.  Three steps of the drop-in loop with the fused
    optimizer equal three steps with torch's clamp_ + Adam: losses, conv weights, biases (model2.py:87-89, train.py:145-146)."""
    def build():
        torch.manual_seed(12)
        m = sat.ShowAttendTellModel(96, 64, 50, 32, None, feature_size=(16, 64), compute_dtype="f32", vgg_cfg=SMALL_VGG).cuda()
        m.finetune(allow=True)
        return m
    g = torch.Generator().manual_seed(4)
    x = torch.rand(4, 3, 32, 32, generator=g).cuda()
    caps = torch.randint(1, 50, (4, 7), generator=g).cuda()
    lengths = [7, 6, 4, 3]
    targets, l1 = sat.pack_targets(caps, lengths)
    crit = torch.nn.CrossEntropyLoss()
    ma, mb = build(), build()
    oa = sat.FusedClampAdam(ma.parameters(), lr=1e-3, clip=0.1)
    ob = torch.optim.Adam(mb.parameters(), lr=1e-3)
    la, lb = [], []
    progs = set()
    for step in range(3):
        oa.zero_grad()
        loss = crit(ma(x, caps[:, :-1], l1), targets)
        loss.backward()
        oa.step()
        la.append(loss.item())
        progs.add(id(ma._program_for(x)))
        mb.zero_grad()
        loss = crit(mb(x, caps[:, :-1], l1), targets)
        loss.backward()
        for p in mb.parameters():
            p.grad.clamp_(-0.1, 0.1)
        ob.step()
        lb.append(loss.item())
    assert len(progs) == 1                                      # the op program is refreshed in place, not rebuilt per step
    assert la[0] == lb[0] and la[2] != la[0]
    for a, b in zip(la, lb):
        assert abs(a - b) < 2e-5, (la, lb)
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.allclose(pa, pb, rtol=0, atol=3e-6), (k, (pa - pb).abs().max().item())
    # the stale-weights failure mode itself: a forward after the steps uses the CURRENT weights
    with torch.no_grad():
        fresh = build()
        fresh.load_state_dict(ma.state_dict())
        assert torch.allclose(ma(x, caps[:, :-1], l1), fresh(x, caps[:, :-1], l1), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["G6_attend_small.npz", "G7_attend_vgg_dims.npz"])
def test_attend_beam_search_width_one_is_golden_greedy_and_wider_matches_oracle(golden_dir, name):
    """`ShowAttendTellModel.sample_beam` (the reference leaves a stub, model2.py:113-114; BASELINE configs[4] asks beam 5):
    width 1 == the golden greedy ids of `sample` (both state conventions); width 3 / 5 with and without an end token == the
    CPU oracle's beam search: ids bit-exact, scores to 1e-4."""
    g = load(golden_dir, name)
    model, params, (hidden, context, vocab, embed, B, T, P, feat) = _model_from_golden(g)
    feats_c = torch.from_numpy(g["features"])
    feats = feats_c.cuda()
    assert np.array_equal(model.sample_beam_features(feats, 1).cpu().numpy(), g["sample_ids_zero_state"])
    h0, c0 = OA.init_lstm(params, feats_c)
    assert np.array_equal(model.sample_beam_features(feats, 1, (h0.cuda(), c0.cuda())).cpu().numpy(), g["sample_ids_init_state"])
    for K, end_id, states in ((3, None, None), (5, 2, None), (4, None, (h0, c0))):
        ref_ids, ref_sc = OA.attend_beam_search(params, feats_c, K, states, end_id=end_id)
        st = None if states is None else (states[0].cuda(), states[1].cuda())
        ids, sc = model.sample_beam_features(feats, K, st, end_id, return_all=True)
        assert ids.shape == (B, K, 20)
        np.testing.assert_allclose(sc.cpu().numpy(), ref_sc.numpy(), rtol=0, atol=2e-4)
        # hypotheses whose scores tie to f32 rounding may swap; everything else is bit-exact
        same = (ids.cpu() == ref_ids).all(2)
        gap = (ref_sc[:, :-1] - ref_sc[:, 1:]).abs().min().item() if K > 1 else 1.0
        assert same.all() or gap < 1e-4, (K, end_id, same, gap)
    with pytest.raises(ValueError):
        model.sample_beam_features(feats, 9)


def test_greedy_and_width_one_beam_agree_from_a_given_state_and_leave_it_alone():
    """The decode step `sample_features` and `sample_beam_features` share, from a NON-zero (h, c), at the smallest legal dims
    (E 4, C 8, H 12, P 5, V 11; B 3): width-1 beam == greedy, ids and attention maps bit for bit (the token comes from different
    kernels: `sat_vocab_argmax` / `sat_vocab_logits_fwd` + `sat_beam_step`); the caller's tensors are not written; a `states` of
    the wrong shape is a ValueError from both, before anything runs on it.  Seed: picked from 0..299 by a float64 replay -- its
    decode changes token 36 times over three tokens, and the smallest top-two log-probability gap is 1.2e-3, far above f32 rounding,
    so the two selections cannot legitimately disagree."""
    torch.manual_seed(179)
    B, P, C, E, H, V = 3, 5, 8, 4, 12, 11
    model = sat.ShowAttendTellModel(H, C, V, E, None, feature_size=(P, C), compute_dtype="f32", vgg_cfg=[C]).cuda().eval()
    feats = torch.randn(B, P, C).cuda()
    h, c = torch.randn(B, H).cuda(), torch.randn(B, H).cuda()
    h_was, c_was = h.clone(), c.clone()
    ids, alphas = model.sample_features(feats, (h, c), return_alphas=True)
    ids_b, alphas_b = model.sample_beam_features(feats, 1, (h, c), return_alphas=True)
    assert ids.shape == (B, 20) and alphas.shape == (B, 20, P)
    assert torch.equal(ids, ids_b) and torch.equal(alphas, alphas_b)
    assert torch.equal(h, h_was) and torch.equal(c, c_was)
    for bad in ((h[:2], c[:2]), (h, c[:, :8]), (h, c, c), (h,)):
        with pytest.raises(ValueError):
            model.sample_features(feats, bad)
        with pytest.raises(ValueError):
            model.sample_beam_features(feats, 1, bad)
