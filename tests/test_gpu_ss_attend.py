"""GPU (MI355X): scheduled sampling in the Show-Attend-Tell training forward (`ShowAttendTellModel.ss_prob`, `sat_ss_attend_fwd`).
Every mask bit and draw is replayed in numpy from the returned logits and the seed (tests/ss_reference.py, the t >= 1 rule of the
attention model); the rest is parity with the CPU oracle run teacher-forced on the tokens actually fed, with the cross entropy taken
against the TEACHER's targets, which is what the scheduled-sampling forward and its backward must equal."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ss_reference as R

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
from oracle import attend as OA  # noqa: E402

SMALL = dict(P=16, C=32, E=32, H=64, V=300)
DEFAULT = dict(P=196, C=512, E=512, H=1024, V=10000)     # config.py defaults (hidden 1024, embed 512), vocab 10 000


def make_model(P, C, E, H, V, seed=0):
    params = OA.init_attend_params(H, C, V, E, generator=torch.Generator().manual_seed(seed), feat=C)
    model = sat.ShowAttendTellModel(H, C, V, E, None, feature_size=(P, C), compute_dtype="f32", vgg_cfg=[8, "M", C])
    model.load_state_dict(params, strict=False)
    return model.cuda().train(), params


def inputs(lengths, P, C, V, seed=1):
    """features [B,P,C] (post-ReLU like the conv stack's), the full captions [B, T+1] (<start> first) and the model's lengths"""
    g = torch.Generator().manual_seed(seed)
    B, T = len(lengths), max(lengths)
    feats = torch.randn(B, P, C, generator=g).clamp(min=0)
    caps = torch.randint(4, V, (B, T + 1), generator=g)
    caps[:, 0] = 1
    return feats, caps


def run(model, feats, caps, lengths):
    """train.py:134-144 on the decoder half: targets = pack(captions[:, 1:]), decode(captions[:, :-1]), mean CE, backward"""
    targets, l1 = sat.pack_targets(caps.cuda(), [l + 1 for l in lengths])
    assert l1 == list(lengths)
    fd = feats.cuda()
    model.zero_grad()
    out = model.decode(fd, fd.mean(1), caps[:, :-1].cuda(), lengths)
    loss = F.cross_entropy(out, targets)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return out.detach(), loss.detach(), grads, targets


def replay(logits, lengths, caps_in, ss_prob, seed, rank):
    """Every decision of one forward, recomputed in float64 from its packed logits: for t >= 1 and b < batch_sizes[t], with
    u(b, t) < ss_prob the token fed to step t is argmax_v(logit[t-1][b][v] + G(b, t, v)), else captions[b][t].  Returns (used [B, T],
    mask, margin = gap between the best and second-best perturbed score of a draw)."""
    bs = OA.batch_sizes(lengths)
    T = len(bs)
    prefix = np.concatenate([[0], np.cumsum(bs)])
    used = np.array(caps_in[:, :T], dtype=np.int64, copy=True)
    mask = np.zeros(used.shape, dtype=bool)
    margin = np.full(used.shape, np.inf)
    V = logits.shape[1]
    p = np.float64(np.float32(ss_prob))
    for t in range(1, T):
        for b in range(bs[t]):
            if not R.mask_uniform(seed, rank, b, t) < p:
                continue
            mask[b, t] = True
            s = logits[prefix[t - 1] + b].astype(np.float64) + R.noise(seed, rank, b, t, V)
            top = np.argsort(-s, kind="stable")[:2]
            used[b, t] = int(np.argmax(s))
            margin[b, t] = s[top[0]] - s[top[1]] if V > 1 else np.inf
    return used, mask, margin


def check_replay(model, out, caps_in, lengths, ss_prob, rank):
    used = model.last_ss_inputs
    assert used.dtype == torch.int64 and tuple(used.shape) == (len(lengths), max(lengths))
    want, mask, margin = replay(out.cpu().numpy(), lengths, caps_in.numpy(), ss_prob, model.last_ss_seed, rank)
    got = used.cpu().numpy()
    close = margin < 1e-4
    assert np.array_equal(got[~close], want[~close]), np.argwhere(got != want)
    return mask


def oracle(params, feats, used, lengths, targets):
    """the oracle teacher-forced on the tokens fed, CE against the teacher's targets, float64"""
    q = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    logits = OA.attend_forward(q, feats.double(), used, lengths)
    loss = F.cross_entropy(logits, targets)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in q.items()}


def check_parity(model, params, feats, lengths, out, loss, grads, targets, elementwise=True):
    """logits / loss / all 19 gradients within test_attend_decoder_matches_reference_goldens' tolerances"""
    ref_logits, ref_loss, ref_grads = oracle(params, feats, model.last_ss_inputs.cpu(), lengths, targets.cpu())
    np.testing.assert_allclose(out.cpu().numpy(), ref_logits.numpy(), rtol=0, atol=2e-5)
    assert abs(loss.item() - ref_loss.item()) < 1e-4
    assert set(grads) == set(sat.attend.PARAM_ORDER) == set(ref_grads)
    for k in sat.attend.PARAM_ORDER:
        got, ref = grads[k].cpu().double(), ref_grads[k]
        if elementwise:
            np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=2e-3, atol=2e-7, err_msg=k)
        else:                      # the goldens' form for large tensors: the norm, and here also the whole difference
            assert abs(got.norm().item() - ref.norm().item()) < 2e-3 * ref.norm().item() + 1e-8, k
            assert (got - ref).norm().item() < 2e-3 * ref.norm().item() + 1e-8, k


@pytest.mark.parametrize("ss_prob,rank", [(0.25, 0), (0.25, 3), (1.0, 0), (1.0, 3)])
def test_draws_replay_exactly_and_match_oracle_on_tokens_fed(ss_prob, rank):
    lengths = [9, 9, 7, 4, 2]
    model, params = make_model(**SMALL)
    feats, caps = inputs(lengths, SMALL["P"], SMALL["C"], SMALL["V"])
    model.ss_prob, model.ss_rank = ss_prob, rank
    torch.manual_seed(17)
    out, loss, grads, targets = run(model, feats, caps, lengths)
    mask = check_replay(model, out, caps[:, :-1], lengths, ss_prob, rank)
    assert mask[:, 0].sum() == 0                          # <start> is never replaced
    if ss_prob == 1.0:
        bs = OA.batch_sizes(lengths)
        assert all(mask[b, t] for t in range(1, len(bs)) for b in range(bs[t]))
    else:
        assert 0 < mask.sum() < sum(lengths) - len(lengths)
    used = model.last_ss_inputs.cpu()
    for b, n in enumerate(lengths):                       # columns a row does not reach keep the teacher's tokens
        assert torch.equal(used[b, n:], caps[b, n:-1])
    check_parity(model, params, feats, lengths, out, loss, grads, targets)


def test_peaked_classifier_bias_every_draw_is_the_peak():
    """ss_prob = 1 and logit bias +60 on token k: every fed token of step t >= 1 is k, step 0 keeps <start>"""
    k = 37
    lengths = [9, 9, 7, 4, 2]
    model, _ = make_model(**SMALL)
    with torch.no_grad():
        model.classifier.weight.mul_(0.01)
        model.classifier.bias.zero_()
        model.classifier.bias[k] = 60.0
    feats, caps = inputs(lengths, SMALL["P"], SMALL["C"], SMALL["V"])
    model.ss_prob = 1.0
    run(model, feats, caps, lengths)
    used = model.last_ss_inputs.cpu()
    assert torch.equal(used[:, 0], caps[:, 0])
    for b, n in enumerate(lengths):
        for t in range(1, max(lengths)):
            want = k if t < n else int(caps[b, t])
            assert int(used[b, t]) == want, (b, t)


def test_ss_prob_zero_and_eval_are_the_teacher_forced_path_bit_for_bit():
    lengths = [9, 9, 7, 4, 2]
    feats, caps = inputs(lengths, SMALL["P"], SMALL["C"], SMALL["V"])
    base, _ = make_model(**SMALL)
    out0, loss0, g0, _ = run(base, feats, caps, lengths)
    for mode in ("zero", "eval"):
        model, _ = make_model(**SMALL)
        if mode == "zero":
            model.ss_prob = 0
        else:
            model.ss_prob = 0.5
            model.eval()
        torch.manual_seed(11)
        rng = torch.get_rng_state()
        out, loss, g, _ = run(model, feats, caps, lengths)
        assert torch.equal(torch.get_rng_state(), rng), mode
        assert model.last_ss_inputs is None and model.last_ss_seed is None
        assert torch.equal(out, out0) and torch.equal(loss, loss0), mode
        assert set(g) == set(g0) and all(torch.equal(g[k], g0[k]) for k in g0), mode


def test_same_seed_same_draws_other_rank_other_draws():
    lengths = [9, 9, 7, 4, 2]
    model, _ = make_model(**SMALL)
    feats, caps = inputs(lengths, SMALL["P"], SMALL["C"], SMALL["V"])
    model.ss_prob = 1.0
    res = []
    for rank in (0, 0, 1):
        model.ss_rank = rank
        torch.manual_seed(2024)
        out = run(model, feats, caps, lengths)[0]
        res.append((model.last_ss_inputs.clone(), out.clone(), model.last_ss_seed))
    assert res[0][2] == res[1][2] == res[2][2]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    assert not torch.equal(res[0][0], res[2][0])
    torch.manual_seed(2025)
    model.ss_rank = 0
    run(model, feats, caps, lengths)
    assert model.last_ss_seed != res[0][2]


@pytest.mark.parametrize("lengths", [[1, 1, 1], [2, 1], [5]], ids=["T1", "T2", "B1"])
def test_edge_shapes(lengths):
    model, params = make_model(**SMALL)
    feats, caps = inputs(lengths, SMALL["P"], SMALL["C"], SMALL["V"], seed=3)
    model.ss_prob = 1.0
    out, loss, grads, targets = run(model, feats, caps, lengths)
    assert out.shape == (sum(lengths), SMALL["V"])
    check_replay(model, out, caps[:, :-1], lengths, 1.0, 0)
    check_parity(model, params, feats, lengths, out, loss, grads, targets)


def default_lengths(B=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    return sorted((int(x) for x in torch.randint(3, 20, (B,), generator=g)), reverse=True)


@pytest.mark.timeout(900)
def test_config_default_dims_replay_and_parity():
    lengths = default_lengths()
    model, params = make_model(**DEFAULT)
    feats, caps = inputs(lengths, DEFAULT["P"], DEFAULT["C"], DEFAULT["V"])
    model.ss_prob = 0.25
    torch.manual_seed(19)
    out, loss, grads, targets = run(model, feats, caps, lengths)
    mask = check_replay(model, out, caps[:, :-1], lengths, 0.25, 0)
    assert mask.sum() > 0
    check_parity(model, params, feats, lengths, out, loss, grads, targets, elementwise=False)


def test_fused_clamp_adam_step_with_sampling_at_default_dims():
    lengths = default_lengths(seed=6)
    model, _ = make_model(**DEFAULT)
    feats, caps = inputs(lengths, DEFAULT["P"], DEFAULT["C"], DEFAULT["V"], seed=7)
    opt = sat.FusedClampAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3, clip=0.1)
    before = {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    model.ss_prob = 0.25
    targets, l1 = sat.pack_targets(caps.cuda(), [l + 1 for l in lengths])
    fd = feats.cuda()
    opt.zero_grad()
    loss = F.cross_entropy(model.decode(fd, fd.mean(1), caps[:, :-1].cuda(), l1), targets)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    assert model.last_ss_inputs is not None
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert torch.isfinite(p).all(), k
            assert not torch.equal(p.detach(), before[k]), k


SMALL_VGG = [16, 16, "M", 32, "M", 64, 64, "M", 64]


def test_finetune_with_sampling_conv_stack_gradients_vs_oracle():
    """`finetune(allow=True)` (model2.py:87-89) with ss_prob 1: the features' gradient comes out of the same backward, run on the
    tokens fed; every conv and decoder gradient against autograd through the CPU oracle on those tokens"""
    g = torch.Generator().manual_seed(31)
    hidden, embed, vocab, B = 64 + 32, 32, 90, 5
    vp = OA.init_vgg_params(g, cfg=SMALL_VGG)
    dp = OA.init_attend_params(hidden, 64, vocab, embed, generator=g, feat=64)
    model = sat.ShowAttendTellModel(hidden, 64, vocab, embed, None, feature_size=(16, 64), compute_dtype="f32", vgg_cfg=SMALL_VGG)
    sd = dict(vp)
    sd.update(dp)
    model.load_state_dict(sd)
    model.cuda().train()
    model.finetune(allow=True)
    images = torch.randn(B, 3, 32, 32, generator=g)
    lengths = [8, 8, 6, 5, 3]
    caps = torch.randint(4, vocab, (B, max(lengths)), generator=g)
    caps[:, 0] = 1
    l1 = [l - 1 for l in lengths]
    di, dc = images.cuda(), caps.cuda()
    targets, _ = sat.pack_targets(dc, lengths)
    model.ss_prob = 1.0
    torch.manual_seed(23)
    model.zero_grad()
    out = model(di, dc[:, :-1], l1)
    loss = F.cross_entropy(out, targets)
    loss.backward()
    used = model.last_ss_inputs.cpu()
    bs = OA.batch_sizes(l1)
    assert any(int(used[b, t]) != int(caps[b, t]) for t in range(1, len(bs)) for b in range(bs[t]))
    q = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref_logits = OA.attend_forward(q, OA.vgg_forward(q, images, cfg=SMALL_VGG), used, l1)
    ref_loss = F.cross_entropy(ref_logits, targets.cpu())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-4
    named = dict(model.named_parameters())
    for k in sd:
        got, ref = named[k].grad.cpu(), q[k].grad
        scale = ref.abs().max().item() + 1e-12
        assert (got - ref).abs().max().item() < 3e-3 * scale + 1e-8, (k, (got - ref).abs().max().item(), scale)
