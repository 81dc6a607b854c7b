"""GPU (MI355X): label smoothing for the cross entropy -- `sat_ce_rows_ls`, `sat_vocab_ce_fwd_bf16_ls`, `sat.CrossEntropy` and
`TrainStep(label_smoothing=)` -- against float64 (tests/label_smoothing_reference.py, validated on the CPU by
tests/test_label_smoothing_host.py), torch's own criterion and the CPU oracle.

Edges of sat_ce_rows_ls (the paths of sat_ce_rows, tests/test_gpu_elementwise_edges.py): V = 1, 3 the scalar tail only; 4, 5 one chunk
(+ 1 tail element); 255, 1003 tails of 3; 1024 one chunk per thread; 12288 all 12 register chunks full; 12289 + 1 tail element; 12292
one chunk past the register path: strided path.  ldl = pad4(V), V, V + 4 (NaN pad columns that must survive); a base misaligned by one
float (strided path).  Rows equal / dominant / low (-80) / shifted (+60) / random with targets placed at 0, V - 1, 4 * (V / 4), 1023,
1024, -1, V (clamped).  Gradient in place, out of place with ldg = pad4(V) + 4 (the path the logits choose) and V + 1, and none.

Tolerances (the rule of tests/test_gpu_elementwise_edges.py).  An f32 output passes when it meets the tolerance the existing tests
use for it -- gradient 2e-8 + 1e-6 inv_denom, loss and nll 1e-5 relative -- OR lies within 8 x the error of the float32 restatement
of the same formula against float64 at that shape and seed (label_smoothing_reference.F32_ERR, frozen from the host test's
measurement).  Row losses and row NLLs have the second rule only.  Bitwise where the arithmetic is pinned: in place against out of
place, NULL outputs, smoothing = 0 against sat_ce_rows / sat_vocab_ce_fwd_bf16, pads, guards and untouched logits, replays.  The
bf16 form, the criterion and the steps carry the tolerances of the tests they extend, named at each.  Nothing here is set from a
kernel's output."""
import importlib

import numpy as np
import pytest
import torch

import elementwise_reference as R
import label_smoothing_reference as LR

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import attend as OA  # noqa: E402
from oracle import decoder as OD  # noqa: E402

NAN = float("nan")
GUARD = 64
TINY = dict(layers=(1, 1, 1, 1), width=8)
SMALL_VGG = [16, 16, "M", 32, "M", 64, 64, "M", 64]
LENGTHS = [12, 12, 11, 9, 9, 7, 4, 3]
GRAD_TOL = 2e-8 + 1e-6 * R.CE_INV


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    return L.load()


def st():
    return L.stream()


def sync():
    torch.cuda.synchronize()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def bits(t):
    return t.contiguous().cpu().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def all_nan(t):
    return bool(torch.isnan(t).all())


def close(tag, got, ref, e32, rtol=0.0, atol=0.0):
    """got against ref (f64): the existing tolerance |err| <= atol + rtol |ref| where there is one, or 8 x the f32 restatement's
    error e32; prints the figures before it asserts"""
    got = got.detach().float().cpu().double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert torch.isfinite(got).all(), tag + ": inf or NaN in the output"
    err = (got - ref).abs()
    legacy = (atol > 0 or rtol > 0) and bool((err <= atol + rtol * ref.abs()).all())
    second = bool((err <= R.TOL_FACTOR * e32).all())
    worst = err.max().item() if err.numel() else 0.0
    print("%-60s err %.3g   f32 restatement %.3g   existing tolerance %s" % (tag, worst, e32, "met" if legacy else "not met"))
    assert legacy or second, "%s: err %.3g > %g x %.3g" % (tag, worst, R.TOL_FACTOR, e32)


_REF = {}


def cached(key, fn):
    """float64 references are computed once, shared, and never modified"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def ls_call(lib, logits, targets, V, ldl, eps, grad="inplace", ldg=None, offset=0, row_nll=True, loss=True, nll=True, inv=R.CE_INV):
    """logits [N, V] into a NaN buffer of pitch ldl starting `offset` floats into an aligned allocation.  grad: "inplace", "out"
    (a NaN buffer of pitch ldg) or "none".  Returns a dict: the logits buffer before and after, the gradient rows [N, :V], the whole
    gradient buffer, and the four outputs with NaN guards behind them"""
    N = logits.shape[0]
    buf = nans(offset + N * ldl + GUARD)
    view = buf[offset:offset + N * ldl].view(N, ldl)
    view[:, :V] = logits.cuda()
    before = buf.clone()
    rl, rn, lo, nl, tg = nans(N + 1), nans(N + 1), nans(2), nans(2), targets.cuda()
    gbuf = gview = None
    if grad == "inplace":
        gptr, ldg, gview = buf.data_ptr() + 4 * offset, ldl, view
    elif grad == "out":
        gbuf = nans(N * ldg + GUARD)
        gview = gbuf[:N * ldg].view(N, ldg)
        gptr = gbuf.data_ptr()
    else:
        gptr, ldg = None, 0
    L.check(lib.sat_ce_rows_ls(buf.data_ptr() + 4 * offset, ldl, L.ptr(tg), N, V, inv, eps, gptr, ldg, L.ptr(rl),
                               L.ptr(rn) if row_nll else None, L.ptr(lo) if loss else None, L.ptr(nl) if nll else None, st()),
            "sat_ce_rows_ls")
    sync()
    return dict(before=before, buf=buf, view=view, gbuf=gbuf, grad=None if gview is None else gview[:, :V], gview=gview,
                row_loss=rl, row_nll=rn, loss=lo, nll=nl)


def check_outputs(tag, o, ref, e, N):
    close(tag + " row_loss", o["row_loss"][:N], ref["row_loss"], e["row_loss"])
    close(tag + " row_nll", o["row_nll"][:N], ref["row_nll"], e["row_nll"])
    close(tag + " loss", o["loss"][:1], ref["loss"].reshape(1), e["loss"], rtol=1e-5)
    close(tag + " nll", o["nll"][:1], ref["nll"].reshape(1), e["nll"], rtol=1e-5)
    assert all_nan(o["row_loss"][N:]) and all_nan(o["row_nll"][N:]) and all_nan(o["loss"][1:]) and all_nan(o["nll"][1:]), tag


# ---------------------------------------------------------------------------------------------- A. sat_ce_rows_ls

@pytest.mark.parametrize("eps", LR.LS_EPS)
@pytest.mark.parametrize("V", R.CE_V)
def test_ce_rows_ls_paths_tails_placed_targets_and_gradient_forms(lib, V, eps):
    logits, targets, _ = R.ce_inputs(V)
    ref = cached(("ls", V, eps), lambda: LR.ls_rows(logits.double(), targets, eps, R.CE_INV))
    e = LR.f32_err("ls", V, eps)
    N = logits.shape[0]
    variants = [(ldl, 0) for ldl in sorted({L.pad4(V), V, V + 4})] + [(L.pad4(V), 1)]
    for ldl, offset in variants:
        tag = "ls V %d eps %g ldl %d%s" % (V, eps, ldl, " base+1" if offset else "")
        a = ls_call(lib, logits, targets, V, ldl, eps, "inplace", offset=offset)
        check_outputs(tag + " in place", a, ref, e, N)
        close(tag + " in place grad", a["grad"], ref["grad"], e["grad"], atol=GRAD_TOL)
        grad_bits = a["grad"].clone()
        a["view"][:, :V] = a["before"][offset:offset + N * ldl].view(N, ldl)[:, :V]         # then only pads and guards can differ
        assert same_bits(a["buf"], a["before"]), tag + ": pads or guards changed"
        # out of place, the path the logits choose: the same bits, the logits untouched, the gradient's pads and guard left alone
        ldg = L.pad4(V) + 4
        b = ls_call(lib, logits, targets, V, ldl, eps, "out", ldg=ldg, offset=offset)
        assert same_bits(b["grad"], grad_bits), tag + ": out of place differs from in place"
        assert same_bits(b["buf"], b["before"]), tag + ": out of place touched the logits"
        assert all_nan(b["gview"][:, V:]) and all_nan(b["gbuf"][N * ldg:]), tag
        for k in ("row_loss", "row_nll", "loss", "nll"):
            assert same_bits(b[k], a[k]), (tag, k)
        # no gradient: the logits untouched, the same outputs
        c = ls_call(lib, logits, targets, V, ldl, eps, "none", offset=offset)
        assert same_bits(c["buf"], c["before"]), tag + ": grad = NULL touched the logits"
        for k in ("row_loss", "row_nll", "loss", "nll"):
            assert same_bits(c[k], a[k]), (tag, k)
    # a gradient pitch that is no multiple of 4 (strided path whatever the logits allow)
    d = ls_call(lib, logits, targets, V, L.pad4(V), eps, "out", ldg=V + 1)
    check_outputs("ls V %d eps %g ldg V+1" % (V, eps), d, ref, e, N)
    close("ls V %d eps %g ldg V+1 grad" % (V, eps), d["grad"], ref["grad"], e["grad"], atol=GRAD_TOL)
    assert same_bits(d["buf"], d["before"]) and all_nan(d["gview"][:, V:]) and all_nan(d["gbuf"][N * (V + 1):])


@pytest.mark.parametrize("V", [1003, 12292])
def test_null_outputs_leave_the_other_outputs_bitwise_equal(lib, V):
    logits, targets, _ = R.ce_inputs(V)
    N, ldl = logits.shape[0], L.pad4(V)
    full = ls_call(lib, logits, targets, V, ldl, 0.1)
    for kw in (dict(row_nll=False, nll=False), dict(nll=False), dict(loss=False), dict(loss=False, nll=False, row_nll=False)):
        o = ls_call(lib, logits, targets, V, ldl, 0.1, **kw)
        assert same_bits(o["buf"], full["buf"]), kw
        for k, given in (("row_loss", True), ("row_nll", kw.get("row_nll", True)), ("loss", kw.get("loss", True)), ("nll", kw.get("nll", True))):
            assert same_bits(o[k], full[k]) if given else all_nan(o[k]), (kw, k)


@pytest.mark.parametrize("N", R.CE_LOSS_N)
def test_loss_out_and_nll_out_over_row_counts(lib, N):
    logits, targets = R.ce_loss_inputs(N)
    V, eps = R.CE_LOSS_V, LR.LS_LOSS_EPS
    ref = LR.ls_rows(logits.double(), targets, eps, R.CE_INV)
    e = LR.f32_err("ls_loss", N, eps)
    o = ls_call(lib, logits, targets, V, L.pad4(V), eps)
    check_outputs("ls N %d" % N, o, ref, e, N)
    close("ls N %d grad" % N, o["grad"], ref["grad"], e["grad"], atol=GRAD_TOL)
    assert all_nan(o["view"][:, V:])
    # nll_out is sat_ce_rows's loss_out on the same inputs
    buf = torch.zeros(N, L.pad4(V), device="cuda")
    buf[:, :V] = logits.cuda()
    rl, lo, tg = nans(N), nans(1), targets.cuda()
    L.check(lib.sat_ce_rows(L.ptr(buf), L.pad4(V), L.ptr(tg), N, V, R.CE_INV, 0, L.ptr(rl), L.ptr(lo), st()), "sat_ce_rows")
    sync()
    close("ls N %d nll against sat_ce_rows" % N, o["nll"][:1], lo.double().cpu(), R.f32_err("ce_loss", N)["loss"], rtol=1e-5)


@pytest.mark.parametrize("V", [1003, 12292])
def test_smoothing_zero_is_sat_ce_rows_bit_for_bit(lib, V):
    """register path (1003) and strided path (12292): row_loss, loss_out and the gradient"""
    logits, targets, _ = R.ce_inputs(V)
    N, ldl = logits.shape[0], L.pad4(V)
    o = ls_call(lib, logits, targets, V, ldl, 0.0)
    buf = nans(N * ldl + GUARD)
    buf[:N * ldl].view(N, ldl)[:, :V] = logits.cuda()
    rl, lo, tg = nans(N + 1), nans(2), targets.cuda()
    L.check(lib.sat_ce_rows(L.ptr(buf), ldl, L.ptr(tg), N, V, R.CE_INV, 1, L.ptr(rl), L.ptr(lo), st()), "sat_ce_rows")
    sync()
    assert same_bits(o["row_loss"], rl) and same_bits(o["loss"], lo) and same_bits(o["buf"], buf)
    out = ls_call(lib, logits, targets, V, ldl, 0.0, "out", ldg=ldl + 4)
    assert same_bits(out["grad"], buf[:N * ldl].view(N, ldl)[:, :V])


# ---------------------------------------------------------------------------------------------- B. the bf16 form

def vocab_inputs(N, H, V):
    g = torch.Generator().manual_seed(N + V)
    return (torch.tanh(torch.randn(N, H, generator=g)).cuda(), torch.empty(V, H).uniform_(-0.1, 0.1, generator=g).cuda(),
            (torch.randn(V, generator=g) * 0.01).cuda(), torch.randint(0, V, (N,), generator=g).cuda())


def bf16_path(lib, Hs, W, b, tg, eps):
    """(logits, row_loss, row_nll, loss, nll, dW, db, dHs) of sat_vocab_ce_fwd_bf16_ls (eps None: sat_vocab_ce_fwd_bf16) + _bwd_bf16"""
    (N, H), V = Hs.shape, W.shape[0]
    wb = lib.sat_vocab_bf16_ws_bytes(N, H, V)
    assert wb > 0
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    lg, rl, rn, lo, nl = nans(N, V), nans(N), nans(N), nans(1), nans(1)
    if eps is None:
        L.check(lib.sat_vocab_ce_fwd_bf16(L.ptr(Hs), L.ptr(W), L.ptr(b), L.ptr(tg), N, H, V, 1.0 / N, L.ptr(lg), V, L.ptr(rl), L.ptr(lo),
                                          L.ptr(ws), wb, st()), "sat_vocab_ce_fwd_bf16")
    else:
        L.check(lib.sat_vocab_ce_fwd_bf16_ls(L.ptr(Hs), L.ptr(W), L.ptr(b), L.ptr(tg), N, H, V, 1.0 / N, eps, L.ptr(lg), V, L.ptr(rl),
                                             L.ptr(rn), L.ptr(lo), L.ptr(nl), L.ptr(ws), wb, st()), "sat_vocab_ce_fwd_bf16_ls")
    dW, db, dH = nans(V, H), nans(V), nans(N, H)
    L.check(lib.sat_vocab_ce_bwd_bf16(N, H, V, L.ptr(dW), L.ptr(db), L.ptr(dH), L.ptr(ws), wb, st()), "sat_vocab_ce_bwd_bf16")
    sync()
    return lg, rl, rn, lo, nl, dW, db, dH


@pytest.mark.parametrize("N,H,V", [(76, 64, 500), (200, 128, 1000), (8, 64, 12288)])
def test_vocab_ce_bf16_ls_vs_exact_f32_path_and_smoothing_zero(lib, N, H, V):
    """the tolerances of test_vocab_ce_bf16_path_vs_exact_f32_path (tests/test_gpu_kernels.py): mean CE 1e-3, gradients 1 % relative
    L2 against sat_vocab_logits_fwd + sat_ce_rows_ls + sat_vocab_ce_bwd; smoothing = 0 is sat_vocab_ce_fwd_bf16 bit for bit"""
    eps = 0.1
    Hs, W, b, tg = vocab_inputs(N, H, V)
    lg32 = torch.empty(N, V, device="cuda")
    L.check(lib.sat_vocab_logits_fwd(L.ptr(Hs), L.ptr(W), L.ptr(b), N, H, V, L.ptr(lg32), V, st()), "sat_vocab_logits_fwd")
    rl32, rn32, lo32, nl32 = nans(N), nans(N), nans(1), nans(1)
    L.check(lib.sat_ce_rows_ls(L.ptr(lg32), V, L.ptr(tg), N, V, 1.0 / N, eps, L.ptr(lg32), V, L.ptr(rl32), L.ptr(rn32), L.ptr(lo32),
                               L.ptr(nl32), st()), "sat_ce_rows_ls")
    wsb = lib.sat_vocab_ce_bwd_ws_bytes(N, H, V)
    ws = torch.empty(max(wsb // 4, 4), device="cuda")
    dW32, db32, dH32 = torch.empty(V, H, device="cuda"), torch.empty(V, device="cuda"), torch.empty(N, H, device="cuda")
    L.check(lib.sat_vocab_ce_bwd(L.ptr(lg32), V, L.ptr(Hs), L.ptr(W), N, H, V, L.ptr(dW32), L.ptr(db32), L.ptr(dH32), L.ptr(ws), wsb,
                                 st()), "sat_vocab_ce_bwd")
    lg, rl, rn, lo, nl, dW, db, dH = bf16_path(lib, Hs, W, b, tg, eps)
    for t in (lg, rl, rn, lo, nl, dW, db, dH):
        assert torch.isfinite(t).all()

    def rel(a, c):
        return ((a - c).norm() / c.norm()).item()
    print("bf16 ls N=%d H=%d V=%d: |dloss| %.2e |dnll| %.2e, rel-L2 dW %.2e db %.2e dHs %.2e"
          % (N, H, V, abs(lo.item() - lo32.item()), abs(nl.item() - nl32.item()), rel(dW, dW32), rel(db, db32), rel(dH, dH32)))
    assert abs(lo.item() - lo32.item()) < 1e-3 and abs(nl.item() - nl32.item()) < 1e-3
    assert rel(dW, dW32) < 1e-2 and rel(db, db32) < 1e-2 and rel(dH, dH32) < 1e-2
    # the logits are the unsmoothed call's, written once and not modified; the gradient is another one
    old = bf16_path(lib, Hs, W, b, tg, None)
    assert same_bits(lg, old[0]) and not same_bits(dW, old[5])
    zero = bf16_path(lib, Hs, W, b, tg, 0.0)
    for i in (0, 1, 3, 5, 6, 7):
        assert same_bits(zero[i], old[i]), i
    assert same_bits(zero[2], zero[1]) and same_bits(zero[4], zero[3])          # row_nll / nll_out at smoothing 0: the loss itself


# ---------------------------------------------------------------------------------------------- C. the criterion

def make_decoder(E, H, V, Lh, seed=4):
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(seed))
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    return dec.cuda().train(), params


def inputs(B, E, V, width, seed=5):
    g = torch.Generator().manual_seed(seed)
    caps = torch.randint(4, V, (B, width), generator=g)
    caps[:, 0] = 1
    return torch.randn(B, E, generator=g), caps


def compare_criteria(forward, params, targets, extra=None):
    """the same forward under nn.CrossEntropyLoss(label_smoothing=0.1) and under sat.CrossEntropy(0.1): loss within 1e-4, every
    gradient rtol 1e-3 + 1e-7, the outputs bitwise untouched by the criterion, last_nll within 1e-4 of torch's plain CE"""
    def run(crit):
        for p in params.values():
            p.grad = None
        out = forward()
        before = out.detach().clone()
        loss = crit(out, targets)
        if extra is not None:
            loss = loss + extra()
        loss.backward()
        sync()
        assert same_bits(out.detach(), before), "the criterion changed the model's outputs"
        return loss.item(), before, {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
    want_loss, out_t, want = run(torch.nn.CrossEntropyLoss(label_smoothing=0.1))
    crit = sat.CrossEntropy(0.1)
    got_loss, out_s, got = run(crit)
    assert same_bits(out_s, out_t)
    assert abs(got_loss - want_loss) < 1e-4, (got_loss, want_loss)
    assert set(got) == set(want) and len(got) > 0
    for k in want:
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k].cpu().numpy(), rtol=1e-3, atol=1e-7, err_msg=k)
    plain = torch.nn.functional.cross_entropy(out_t, targets)
    assert crit.last_nll.shape == (1,) and abs(crit.last_nll.item() - plain.item()) < 1e-4
    rows = torch.nn.functional.cross_entropy(out_t, targets, reduction="none")
    assert (crit.last_row_nll - rows).abs().max().item() < 1e-4
    crit.check_ids()                                            # every target was in range
    return crit


@pytest.mark.parametrize("Lh", [1, 2])
def test_criterion_on_a_small_decoder_equals_torchs(Lh):
    E, H, V = 32, 64, 1003
    dec, _ = make_decoder(E, H, V, Lh)
    feats, caps = inputs(len(LENGTHS), E, V, 12)
    targets, l1 = sat.pack_targets(caps.cuda(), LENGTHS)
    f = feats.cuda().requires_grad_(True)
    params = dict(dec.named_parameters())
    params["features"] = f
    compare_criteria(lambda: dec(f, caps[:, :-1].cuda(), l1), params, targets)


def test_criterion_on_the_small_attention_model_with_the_penalty():
    g = torch.Generator().manual_seed(12)
    hidden, embed, vocab, B, T = 64 + 32, 32, 120, 6, 9
    vp = OA.init_vgg_params(g, cfg=SMALL_VGG)
    dp = OA.init_attend_params(hidden, 64, vocab, embed, generator=g, feat=64)
    model = sat.ShowAttendTellModel(hidden, 64, vocab, embed, None, feature_size=(16, 64), compute_dtype="f32", vgg_cfg=SMALL_VGG)
    sd = dict(vp)
    sd.update(dp)
    model.load_state_dict(sd)
    model.cuda()
    model.alpha_c = 1.0
    images = torch.randn(B, 3, 32, 32, generator=g)
    lengths = [9, 9, 7, 6, 4, 3]
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, vocab, (l - 2,), generator=g)
        caps[b, l - 1] = 2
    di, dc = images.cuda(), caps.cuda()
    targets, l1 = sat.pack_targets(dc, lengths)
    params = {k: p for k, p in model.named_parameters() if p.requires_grad}
    compare_criteria(lambda: model(di, dc[:, :-1], l1), params, targets, extra=lambda: model.last_attention_penalty)


def test_criterion_function_form_default_and_target_check():
    logits, targets = R.ce_loss_inputs(255)
    x, t = logits.cuda().requires_grad_(True), targets.cuda()
    out = {}
    loss = sat.cross_entropy(x, t, out=out)                     # label_smoothing = 0: the plain mean CE
    want = torch.nn.functional.cross_entropy(logits.double(), targets)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and abs(loss.item() - want.item()) < 1e-5 * want.item()
    assert same_bits(out["last_nll"], loss.detach().view(1)) and out["last_row_nll"].shape == (255,)
    (2 * loss).backward()
    ref = LR.ls_rows(logits.double(), targets, 0.0, 1.0)["grad"] * (2.0 / 255)
    assert (x.grad.double().cpu() - ref).abs().max().item() <= 2 * (2e-8 + 1e-6 / 255)       # (the backward doubles the gradient)
    crit = sat.CrossEntropy(0.1)
    bad = t.clone()
    bad[7] = R.CE_LOSS_V
    crit(x.detach(), bad)
    with pytest.raises(IndexError, match="targets"):
        crit.check_ids()


# ---------------------------------------------------------------------------------------------- D. TrainStep

def ts_model(E, H, V, Lh, dtype, seed=4):
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY, compute_dtype=dtype)
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(seed))
    model.decoder.load_state_dict(params)
    return model.cuda().train(), params


@pytest.mark.parametrize("Lh", [1, 2])
def test_trainstep_f32_mode_against_the_oracle_backward_of_the_smoothed_gradient(Lh):
    """the pattern of test_trainstep_exact_mode_parity_on_used (tests/test_gpu_ss.py): loss 1e-4, gradients rtol 1e-3 + 1e-7"""
    E, H, V = 32, 64, 1003
    model, params = ts_model(E, H, V, Lh, "f32")
    feats, caps = inputs(len(LENGTHS), E, V, 12, seed=6)
    ts = sat.TrainStep(model, label_smoothing=0.1)
    assert ts.decoder_gemm_dtype == "f32" and ts.label_smoothing == 0.1
    n_tok = sum(l - 1 for l in LENGTHS)
    loss = ts.forward_backward((feats.cuda(), caps.cuda(), LENGTHS), 1.0 / n_tok)
    targets, l1 = sat.pack_targets(caps.cuda(), LENGTHS)
    ref_logits, tape = OD.decoder_forward(params, feats, caps[:, :-1], l1, Lh, keep=True)
    ref = LR.ls_rows(ref_logits.double(), targets.cpu(), 0.1, 1.0 / n_tok)
    assert abs(loss.item() - ref["loss"].item()) < 1e-4
    assert ts.last_nll.shape == (1,) and abs(ts.last_nll.item() - ref["nll"].item()) < 1e-4
    assert abs(ref["nll"].item() - OD.cross_entropy(ref_logits, targets.cpu()).item()) < 1e-6
    grads, d_feat = OD.decoder_backward(params, tape, caps[:, :-1], l1, ref["grad"].float(), Lh)
    np.testing.assert_allclose(ts.last_d_features.cpu().numpy(), d_feat.numpy(), rtol=1e-3, atol=1e-7)
    for k, p in model.decoder.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), rtol=1e-3, atol=1e-7, err_msg=k)


def test_trainstep_bf16_mode_loss_replay_sampling_and_dropout():
    """E 64, H 64, V 1000: the loss within 2e-3 of the f32-mode step (the bf16 CE tolerance of
    test_trainstep_bf16_cfg1_shape_reproducible_and_learns); identical calls, and replays under ss_prob / dropout_p, bit for bit"""
    E, H, V = 64, 64, 1000
    feats, caps = inputs(len(LENGTHS), E, V, 12, seed=7)
    batch = (feats.cuda(), caps.cuda(), LENGTHS)
    n_tok = sum(l - 1 for l in LENGTHS)
    m32, _ = ts_model(E, H, V, 1, "f32")
    t32 = sat.TrainStep(m32, label_smoothing=0.1)
    loss32 = t32.forward_backward(batch, 1.0 / n_tok).item()
    nll32 = t32.last_nll.item()
    model, _ = ts_model(E, H, V, 1, "bf16")
    ts = sat.TrainStep(model)
    ts.label_smoothing = 0.1                                    # the settable attribute
    assert ts.decoder_gemm_dtype == "bf16" and t32.decoder_gemm_dtype == "f32"

    def run(seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        loss = ts.forward_backward(batch, 1.0 / n_tok).clone()
        return loss, ts.flat_grad.clone(), ts.last_nll.clone()
    l0, g0, n0 = run()
    l1, g1, n1 = run()
    assert abs(l0.item() - loss32) < 2e-3 and abs(n0.item() - nll32) < 2e-3, (l0.item(), loss32, n0.item(), nll32)
    assert not same_bits(l0, n0)                                # the loss slot holds the smoothed loss, last_nll the plain one
    assert same_bits(l0, l1) and same_bits(g0, g1) and same_bits(n0, n1)
    assert torch.isfinite(g0).all() and float(g0.abs().sum()) > 0
    model.decoder.ss_prob = 0.5
    a, b, c = run(21), run(21), run(22)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and not same_bits(a[1], c[1])
    assert not same_bits(a[1], g0) and torch.isfinite(a[1]).all()
    model.decoder.ss_prob = 0.0
    model.decoder.dropout_p = 0.5
    a, b, c = run(31), run(31), run(32)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and not same_bits(a[1], c[1])
    assert not same_bits(a[1], g0) and torch.isfinite(a[1]).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainstep_label_smoothing_zero_is_the_step_without_the_keyword(dtype):
    E, H, V = 64, 64, 1000
    feats, caps = inputs(len(LENGTHS), E, V, 12, seed=8)
    batch = (feats.cuda(), caps.cuda(), LENGTHS)
    n_tok = sum(l - 1 for l in LENGTHS)
    out = []
    for kw in ({}, dict(label_smoothing=0.0)):
        model, _ = ts_model(E, H, V, 1, dtype)
        ts = sat.TrainStep(model, **kw)
        assert ts.decoder_gemm_dtype == dtype and ts.label_smoothing == 0.0
        loss = ts.forward_backward(batch, 1.0 / n_tok)
        assert ts.last_nll.data_ptr() == loss.data_ptr()        # with 0 the loss is the NLL: the loss slot itself
        out.append((loss.clone(), ts.flat_grad.clone()))
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])
    assert torch.isfinite(out[0][1]).all() and float(out[0][1].abs().sum()) > 0
