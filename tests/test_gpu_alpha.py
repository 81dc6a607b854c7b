"""GPU (MI355X): the attention maps of Show-Attend-Tell reach the caller (`last_alphas`, `return_alphas`) and doubly stochastic
attention (`alpha_c`, Xu et al. 2015 section 4.2.1) trains -- the three kernels through the C ABI against float64, and the model
against the maps of the reference class's own `attention_layer` (tests/golden/alpha/G10) and the f64 restatement
(tests/alpha_reference.py)."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alpha_reference as AR

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import attend as OA  # noqa: E402
from oracle import decoder as OD  # noqa: E402

ALPHA_C = AR.MODEL_TEST_ALPHA_C          # tests/test_alpha_host.py: the weight at which a dropped injection is 100 x out of tolerance
G10 = os.path.join("alpha", "G10_attend_alphas.npz")


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def st():
    return L.stream()


# ---------------------------------------------------------------------------------------------- kernels through the C ABI

@pytest.mark.parametrize("P", [196, 13])
def test_attention_coverage_vs_fp64(P):
    lib = L.load()
    lengths = [6, 6, 4, 2, 1]
    B, T = len(lengths), max(lengths)
    pi = sat.PackInfo(lengths, "cuda")
    g = torch.Generator().manual_seed(40 + P)
    alpha = torch.softmax(torch.randn(pi.N, P, generator=g) * 2, dim=1)
    coef = 0.37 / (B * P)
    cov64 = torch.zeros(B, P, dtype=torch.float64)
    for t, bs in enumerate(pi.batch_sizes):
        cov64[:bs] += alpha[pi.prefix[t]:pi.prefix[t] + bs].double()
    pen64 = coef * ((cov64 - 1) ** 2).sum().item()
    ad = alpha.cuda()
    wsb = lib.sat_attention_coverage_ws_bytes(B, P)
    assert wsb > 0

    def run():
        cov, grad = torch.full((B, P), float("nan"), device="cuda"), torch.full((B, P), float("nan"), device="cuda")
        pen, ws = torch.full((1,), float("nan"), device="cuda"), torch.empty(wsb // 4, device="cuda")
        L.check(lib.sat_attention_coverage(ad.data_ptr(), pi.prefix_dev.data_ptr(), T, B, P, coef, cov.data_ptr(), grad.data_ptr(),
                                           pen.data_ptr(), ws.data_ptr(), wsb, st()))
        torch.cuda.synchronize()
        return cov.cpu(), grad.cpu(), pen.cpu()
    cov, grad, pen = run()
    tol = T * T * 2.0 ** -24            # T f32 additions of values <= T
    ecov = (cov.double() - cov64).abs().max().item()
    egrad = (grad.double() / (2 * coef) - (cov64 - 1)).abs().max().item()
    print("P %d: cov err %.3g, grad/(2 coef) err %.3g (tol %.3g), penalty %.8g vs %.8g" % (P, ecov, egrad, tol, pen.item(), pen64))
    assert ecov <= tol and egrad <= tol
    assert abs(pen.item() - pen64) <= 1e-5 * abs(pen64)
    cov2, grad2, pen2 = run()
    assert torch.equal(cov.view(torch.int32), cov2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    assert torch.equal(pen.view(torch.int32), pen2.view(torch.int32))
    # cov is optional
    grad3, pen3, ws = torch.empty(B, P, device="cuda"), torch.empty(1, device="cuda"), torch.empty(wsb // 4, device="cuda")
    L.check(lib.sat_attention_coverage(ad.data_ptr(), pi.prefix_dev.data_ptr(), T, B, P, coef, None, grad3.data_ptr(), pen3.data_ptr(),
                                       ws.data_ptr(), wsb, st()))
    assert torch.equal(grad3.cpu(), grad) and torch.equal(pen3.cpu(), pen)
    bad = (lib.sat_attention_coverage(None, pi.prefix_dev.data_ptr(), T, B, P, coef, None, grad3.data_ptr(), pen3.data_ptr(), ws.data_ptr(), wsb, st()),
           lib.sat_attention_coverage(ad.data_ptr(), None, T, B, P, coef, None, grad3.data_ptr(), pen3.data_ptr(), ws.data_ptr(), wsb, st()),
           lib.sat_attention_coverage(ad.data_ptr(), pi.prefix_dev.data_ptr(), T, B, 0, coef, None, grad3.data_ptr(), pen3.data_ptr(), ws.data_ptr(), wsb, st()),
           lib.sat_attention_coverage(ad.data_ptr(), pi.prefix_dev.data_ptr(), 0, B, P, coef, None, grad3.data_ptr(), pen3.data_ptr(), ws.data_ptr(), wsb, st()),
           lib.sat_attention_coverage(ad.data_ptr(), pi.prefix_dev.data_ptr(), T, B, P, coef, None, None, pen3.data_ptr(), ws.data_ptr(), wsb, st()))
    assert bad == (1001,) * 5
    assert lib.sat_attention_coverage(ad.data_ptr(), pi.prefix_dev.data_ptr(), T, B, P, coef, None, grad3.data_ptr(), pen3.data_ptr(),
                                      None, 0, st()) == 1002
    assert lib.sat_attention_coverage(ad.data_ptr(), pi.prefix_dev.data_ptr(), T, B, P, coef, None, grad3.data_ptr(), pen3.data_ptr(),
                                      ws.data_ptr(), wsb - 4, st()) == 1002


def test_attention_bwd_ex_vs_fp64_and_plain_bwd():
    lib = L.load()
    g = torch.Generator().manual_seed(3)
    B, P, C = 5, 196, 512
    ce, fe = torch.randn(B, P, C, generator=g) * 0.5, torch.randn(B, P, C, generator=g).clamp(min=0)
    proj, w = torch.randn(B, C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.1
    dctx, extra = torch.randn(B, C, generator=g), torch.randn(B, P, generator=g)
    SCALE = 0.37
    ce64, fe64, pj64, w64 = (t.double().requires_grad_(True) for t in (ce, fe, proj, w))
    hatt = torch.tanh(ce64 + pj64[:, None, :])
    alpha = torch.softmax(hatt @ w64, dim=1)
    ctx = (fe64 * alpha[:, :, None]).mean(1)
    ((ctx * dctx.double()).sum() + SCALE * (extra.double() * alpha).sum()).backward()
    d = [t.cuda() for t in (ce, fe, proj, w, dctx)]
    al, co = torch.empty(B, P, device="cuda"), torch.empty(B, C, device="cuda")
    ws = torch.empty(lib.sat_attention_ws_bytes(B, P) // 4, device="cuda")
    L.check(lib.sat_attention_fwd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), C, d[3].data_ptr(), B, P, C, al.data_ptr(),
                                  co.data_ptr(), C, ws.data_ptr(), ws.numel() * 4, st()))
    half = (d[4] * 0.25).contiguous()                                                   # d_ctx arrives as the sum of two addends
    rest = (d[4] - half).contiguous()
    ex_d = torch.full((B, P + 3), float("nan"), device="cuda")                           # strided extra: ld_extra = P + 3
    ex_d[:, :P] = extra.cuda()

    def run(mode, scale=None):
        dce = torch.ones(B, P, C, device="cuda")                                        # accumulates INTO the buffer
        dpj, dwp = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
        dfe = torch.zeros(B, P, C, device="cuda")
        head = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), C, d[3].data_ptr(), al.data_ptr(), half.data_ptr(), C, rest.data_ptr(), C)
        tail = (B, P, C, dce.data_ptr(), dpj.data_ptr(), dwp.data_ptr(), dfe.data_ptr(), ws.data_ptr(), ws.numel() * 4, st())
        if mode == "plain":
            L.check(lib.sat_attention_bwd(*head, *tail))
        elif mode == "null":
            L.check(lib.sat_attention_bwd_ex(*head, None, 0, None, *tail))
        else:
            sc = torch.tensor([scale], device="cuda")
            L.check(lib.sat_attention_bwd_ex(*head, ex_d.data_ptr(), P + 3, sc.data_ptr(), *tail))
        torch.cuda.synchronize()
        return dce, dpj, dwp, dfe
    plain, null = run("plain"), run("null")
    assert all(torch.equal(a, b) for a, b in zip(plain, null))
    zero = run("extra", 0.0)
    assert all(torch.equal(a, b) for a, b in zip(null, zero))
    dce, dpj, dwp, dfe = run("extra", SCALE)
    assert not torch.equal(dpj, plain[1])
    # the tolerances of test_attention_fwd_bwd_kernels_vs_fp64 for the same outputs
    np.testing.assert_allclose(dce.cpu().numpy() - 1.0, ce64.grad.numpy(), rtol=0, atol=3e-7)
    np.testing.assert_allclose(dpj.cpu().numpy(), pj64.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dwp.sum(0).cpu().numpy(), w64.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dfe.cpu().numpy(), fe64.grad.numpy(), rtol=1e-4, atol=1e-8)
    sc = torch.tensor([SCALE], device="cuda")
    head = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), C, d[3].data_ptr(), al.data_ptr(), half.data_ptr(), C, rest.data_ptr(), C)
    tail = (B, P, C, dce.data_ptr(), dpj.data_ptr(), dwp.data_ptr(), dfe.data_ptr(), ws.data_ptr(), ws.numel() * 4, st())
    assert lib.sat_attention_bwd_ex(*head, ex_d.data_ptr(), P + 3, None, *tail) == 1001          # one extra without the other
    assert lib.sat_attention_bwd_ex(*head, None, 0, sc.data_ptr(), *tail) == 1001
    assert lib.sat_attention_bwd_ex(*head, ex_d.data_ptr(), P - 1, sc.data_ptr(), *tail) == 1001  # ld_extra < P
    assert lib.sat_attention_bwd_ex(*head, ex_d.data_ptr(), P + 3, sc.data_ptr(), *tail[:7], None, 0, st()) == 1002


def test_beam_backtrack_rows_equals_a_python_walk():
    lib = L.load()
    steps, B, K, cols = 5, 3, 4, 13
    g = torch.Generator().manual_seed(5)
    parents = torch.randint(0, K, (steps, B * K), generator=g, dtype=torch.int32)
    rows = torch.randn(steps, B * K, cols, generator=g)
    want = torch.empty(B, K, steps, cols)
    for b in range(B):
        for k in range(K):
            cur = k
            for t in reversed(range(steps)):
                cur = int(parents[t, b * K + cur])
                want[b, k, t] = rows[t, b * K + cur]
    pd, rd = parents.cuda(), rows.cuda()
    out = torch.full((B, K, steps, cols), float("nan"), device="cuda")
    L.check(lib.sat_beam_backtrack_rows(pd.data_ptr(), rd.data_ptr(), steps, B, K, cols, out.data_ptr(), st()))
    assert torch.equal(out.cpu(), want)
    assert lib.sat_beam_backtrack_rows(None, rd.data_ptr(), steps, B, K, cols, out.data_ptr(), st()) == 1001
    assert lib.sat_beam_backtrack_rows(pd.data_ptr(), rd.data_ptr(), steps, B, K, 0, out.data_ptr(), st()) == 1001


# ---------------------------------------------------------------------------------------------- the model, G6 configuration

_CASE = {}


def g6(golden_dir):
    """G6's model inputs, its parameters in f32 and f64, and the f64 restatement's CE + penalty results (computed once)"""
    if not _CASE:
        g = load(golden_dir, "G6_attend_small.npz")
        dims = [int(x) for x in g["dims"]]
        hidden, context, vocab, embed, B, T, P, feat = dims
        params = OA.init_attend_params(hidden, context, vocab, embed, generator=torch.Generator().manual_seed(int(g["seed"])), feat=feat)
        feats, caps = torch.from_numpy(g["features"]), torch.from_numpy(g["captions"])
        l1 = [int(x) - 1 for x in g["lengths"]]
        targets = OD.pack_time_major(caps[:, 1:], l1)
        p64 = {k: v.double() for k, v in params.items()}
        ref = AR.loss_and_grads(p64, feats.double(), caps[:, :-1], l1, targets, ALPHA_C, feature_grad=True)
        _CASE.update(g=g, z=load(golden_dir, G10), dims=dims, params=params, p64=p64, feats=feats, caps=caps, l1=l1, targets=targets, ref=ref)
    return _CASE


def make_model(c):
    hidden, context, vocab, embed, B, T, P, feat = c["dims"]
    model = sat.ShowAttendTellModel(hidden, context, vocab, embed, None, feature_size=(P, feat), compute_dtype="f32", vgg_cfg=[8, "M", feat])
    model.load_state_dict(c["params"], strict=False)
    return model.cuda().train()


def train_once(model, c, alpha_c, with_penalty=True, feature_grad=False, ss_prob=0):
    """train.py:134-144 on the decoder half with the two-line change: loss = CE + model.last_attention_penalty"""
    model.alpha_c, model.ss_prob = alpha_c, ss_prob
    fd = c["feats"].cuda().requires_grad_(feature_grad)
    model.zero_grad()
    out = model.decode(fd, fd.mean(1), c["caps"][:, :-1].cuda(), c["l1"])
    ce = F.cross_entropy(out, c["targets"].cuda())
    pen = model.last_attention_penalty
    loss = ce + pen if (with_penalty and pen is not None) else ce
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return out.detach(), ce.detach(), pen, grads, fd.grad


def check_grads(grads, d_feats, ref):
    assert set(grads) == set(sat.attend.PARAM_ORDER) == set(ref["grads"])
    for k in sat.attend.PARAM_ORDER:
        np.testing.assert_allclose(grads[k].cpu().double().numpy(), ref["grads"][k].numpy(), rtol=AR.GRAD_RTOL, atol=AR.GRAD_ATOL, err_msg=k)
    if d_feats is not None:
        np.testing.assert_allclose(d_feats.cpu().double().numpy(), ref["d_features"].numpy(), rtol=AR.GRAD_RTOL, atol=AR.GRAD_ATOL,
                                   err_msg="d_features")


def test_model_alphas_penalty_and_gradients_vs_golden_and_restatement(golden_dir):
    c = g6(golden_dir)
    z, ref = c["z"], c["ref"]
    B, P = c["dims"][4], c["dims"][6]
    model = make_model(c)
    out, ce, pen, grads, d_feats = train_once(model, c, ALPHA_C, feature_grad=True)
    al = model.last_alphas
    assert tuple(al.shape) == (sum(c["l1"]), P) == tuple(out.shape[:1]) + (P,) and not al.requires_grad and al.grad_fn is None
    got = al.cpu().numpy()
    print("alphas vs G10: step 0 %.3g, overall %.3g; row sums off by %.3g" % (np.abs(got[:B] - z["alphas_train"][:B]).max(),
          np.abs(got - z["alphas_train"]).max(), np.abs(got.astype(np.float64).sum(1) - 1).max()))
    np.testing.assert_allclose(got[:B], z["alphas_train"][:B], rtol=0, atol=2e-7)
    np.testing.assert_allclose(got, z["alphas_train"], rtol=0, atol=2e-5)
    assert np.abs(got.astype(np.float64).sum(1) - 1).max() < 1e-6
    want = ALPHA_C * float(z["penalty_alpha_c_1"])
    assert pen.dim() == 0 and pen.requires_grad
    print("penalty %.8g vs G10 %.8g (restatement %.8g)" % (pen.item(), want, ref["penalty"].item()))
    assert abs(pen.item() - want) <= 1e-5 * want
    assert abs(ce.item() - float(c["g"]["loss"])) < 1e-4
    check_grads(grads, d_feats, ref)


def test_model_with_scheduled_sampling_matches_restatement_on_the_tokens_fed(golden_dir):
    c = g6(golden_dir)
    assert len(set(c["l1"])) > 1                                  # ragged
    model = make_model(c)
    torch.manual_seed(29)
    out, ce, pen, grads, d_feats = train_once(model, c, ALPHA_C, feature_grad=True, ss_prob=0.5)
    used = model.last_ss_inputs.cpu()
    assert not torch.equal(used, c["caps"][:, :used.shape[1]])    # something was drawn
    ref = AR.loss_and_grads(c["p64"], c["feats"].double(), used, c["l1"], c["targets"], ALPHA_C, feature_grad=True)
    np.testing.assert_allclose(model.last_alphas.cpu().numpy(), ref["alphas"].numpy(), rtol=0, atol=2e-5)
    print("ss penalty %.8g vs restatement %.8g" % (pen.item(), ref["penalty"].item()))
    assert abs(pen.item() - ref["penalty"].item()) <= 1e-5 * ref["penalty"].item()
    assert abs(ce.item() - ref["ce"].item()) < 1e-4
    check_grads(grads, d_feats, ref)


def test_defaults_are_inert(golden_dir):
    c = g6(golden_dir)
    model = make_model(c)
    out0, ce0, pen0, g0, _ = train_once(model, c, 0)
    assert pen0 is None and model.last_attention_penalty is None and model.last_alphas is not None
    out1, ce1, pen1, g1, _ = train_once(model, c, ALPHA_C, with_penalty=False)         # the penalty exists but the loss ignores it
    assert pen1 is not None and torch.equal(out0, out1) and torch.equal(ce0, ce1)
    assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    out2, _, pen2, g2, _ = train_once(model, c, ALPHA_C)                                # ... and with it the gradients move
    assert torch.equal(out0, out2) and torch.equal(pen1.detach(), pen2.detach())
    assert not torch.equal(g0["weight_att"], g2["weight_att"])
    model.eval()
    with torch.no_grad():
        model.alpha_c = 0
        model.decode(c["feats"].cuda(), c["feats"].cuda().mean(1), c["caps"][:, :-1].cuda(), c["l1"])
    assert model.last_attention_penalty is None and model.last_alphas.shape[0] == sum(c["l1"])


def test_decode_returns_the_maps_greedy_and_beam(golden_dir):
    c = g6(golden_dir)
    g, z, p64 = c["g"], c["z"], c["p64"]
    hidden, context, vocab, embed, B, T, P, feat = c["dims"]
    model = make_model(c).eval()
    feats = c["feats"].cuda()
    h0, c0 = OA.init_lstm(c["params"], c["feats"])
    for key, states in (("zero_state", None), ("init_state", (h0.cuda(), c0.cuda()))):
        ids, al = model.sample_features(feats, states, return_alphas=True)
        assert torch.equal(ids, model.sample_features(feats, states)) and np.array_equal(ids.cpu().numpy(), g["sample_ids_" + key])
        assert tuple(al.shape) == (B, 20, P) and al.is_contiguous()
        print("greedy alphas (%s) vs G10: %.3g" % (key, np.abs(al.cpu().numpy() - z["alphas_greedy_" + key]).max()))
        np.testing.assert_allclose(al.cpu().numpy(), z["alphas_greedy_" + key], rtol=0, atol=2e-5)
        ids1, al1 = model.sample_beam_features(feats, 1, states, return_alphas=True)
        assert torch.equal(ids1, ids) and torch.equal(al1, al)
    ref_ids, ref_sc, ref_al = AR.beam(p64, c["feats"].double(), 3)
    ids3, sc3, al3 = model.sample_beam_features(feats, 3, return_all=True, return_alphas=True)
    ids3b, sc3b = model.sample_beam_features(feats, 3, return_all=True)
    assert torch.equal(ids3, ids3b) and torch.equal(sc3, sc3b)
    assert tuple(al3.shape) == (B, 3, 20, P)
    assert torch.equal(ids3.cpu(), ref_ids)                       # tie-free inputs (tests/test_gpu_attend.py's beam test, K = 3)
    print("beam-3 alphas vs restatement: %.3g" % (al3.cpu().double() - ref_al).abs().max().item())
    np.testing.assert_allclose(al3.cpu().numpy(), ref_al.numpy(), rtol=0, atol=2e-5)
    best_ids, best_al = model.sample_beam_features(feats, 3, return_alphas=True)
    assert torch.equal(best_ids, ids3[:, 0]) and torch.equal(best_al, al3[:, 0])
    # through the images: sample / sample_beam hand the maps on
    images = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(6)).cuda()
    ids, al = model.sample(images, return_alphas=True)
    assert torch.equal(ids, model.sample(images)) and tuple(al.shape) == (2, 20, P)
    assert (al.sum(2) - 1).abs().max().item() < 1e-6
    bi, ba = model.sample_beam(images, 2, return_alphas=True)
    assert torch.equal(bi, model.sample_beam(images, 2)) and tuple(ba.shape) == (2, 20, P)
