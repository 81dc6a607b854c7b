"""GPU (MI355X): token-level unlikelihood training -- `sat_ce_rows_ul`, `sat_vocab_ce_fwd_bf16_ul`, `sat.CrossEntropy(unlikelihood=)`
and `TrainStep.unlikelihood` -- against the float64 autograd reference of tests/unlikelihood_reference.py (validated on the CPU by
tests/test_unlikelihood_host.py, which also asserts on that reference what this file relies on: no candidate near the clamp, bounded
amplification in the sweeps, firmly clamped clamp rows).

Edges: V = 3, 5 (scalar tail / one chunk + 1); 255, 1003 (tails of 3); 1024; 12288 (all 12 register chunks); 12289 (+ 1 tail element);
12292 (strided path).  ldl = pad4(V) and V + 4 with NaN pad columns that must survive; a base misaligned by one float (strided
path).  Packs [12,12,11,9,9,7,4,3], [1], [1,1,1], [2,1], [64,64,3] (63 candidates: every lane of the wave); T = 65 is refused.
Candidates at column 0, V - 1, in the scalar tail, on both sides of a 16-byte chunk boundary, equal to the target (excluded),
one repeated id, all distinct, -1 and V (clamped onto 0 and V - 1), and ids 2048 apart.  Rows random, equal, +60, -80, and clamp
rows with one dominant candidate.

Tolerances (the rule of tests/test_gpu_elementwise_edges.py as tests/test_gpu_label_smoothing.py applies it).  An output passes
within the existing tolerance where there is one -- that is alpha = 0 only: gradient 2e-8 + 1e-6 inv_denom, loss and nll 1e-5
relative -- OR within 8 x the error of the float32 restatement against float64 at that case (unlikelihood_reference.F32_ERR,
frozen from the host test's measurement).  Bitwise where the arithmetic is pinned.  The bf16 form, the criterion and the steps carry
the tolerances of the tests they extend, named at each.  Nothing here is set from a kernel's output."""
import importlib

import numpy as np
import pytest
import torch

import elementwise_reference as R
import label_smoothing_reference as LR
import unlikelihood_reference as UR

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
OUT = ("row_loss", "row_nll", "row_ul", "loss", "nll", "ul")


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
    print("%-64s err %.3g   f32 restatement %.3g   existing tolerance %s" % (tag, worst, e32, "met" if legacy else "not met / none"))
    assert legacy or second, "%s: err %.3g > %g x %.3g" % (tag, worst, R.TOL_FACTOR, e32)


_REF = {}


def cached(key, fn):
    """float64 references are computed once, shared, and never modified"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def prefix_dev(lengths):
    return torch.tensor(UR.prefix(lengths), dtype=torch.int32, device="cuda")


def ul_call(lib, logits, targets, lengths, V, ldl, eps, alpha, grad="inplace", ldg=None, offset=0, give=OUT, inv=R.CE_INV):
    """logits [N, V] into a NaN buffer of pitch ldl starting `offset` floats into an aligned allocation.  grad: "inplace", "out" (a
    NaN buffer of pitch ldg) or "none".  `give`: the optional outputs that are not NULL.  Returns the logits buffer before and after,
    the gradient rows [N, :V], the whole gradient buffer, and the six outputs with NaN guards behind them"""
    N = logits.shape[0]
    buf = nans(offset + N * ldl + GUARD)
    view = buf[offset:offset + N * ldl].view(N, ldl)
    view[:, :V] = logits.cuda()
    before = buf.clone()
    o = dict(row_loss=nans(N + 1), row_nll=nans(N + 1), row_ul=nans(N + 1), loss=nans(2), nll=nans(2), ul=nans(2))
    tg, pre = targets.cuda(), prefix_dev(lengths)
    gbuf = gview = None
    if grad == "inplace":
        gptr, ldg, gview = buf.data_ptr() + 4 * offset, ldl, view
    elif grad == "out":
        gbuf = nans(N * ldg + GUARD)
        gview = gbuf[:N * ldg].view(N, ldg)
        gptr = gbuf.data_ptr()
    else:
        gptr, ldg = None, 0
    p = {k: (L.ptr(o[k]) if k in give or k == "row_loss" else None) for k in OUT}
    L.check(lib.sat_ce_rows_ul(buf.data_ptr() + 4 * offset, ldl, L.ptr(tg), L.ptr(pre), len(UR.batch_sizes(lengths)), N, V, inv, eps,
                               alpha, gptr, ldg, p["row_loss"], p["row_nll"], p["row_ul"], p["loss"], p["nll"], p["ul"], st()),
            "sat_ce_rows_ul")
    sync()
    o.update(before=before, buf=buf, view=view, gbuf=gbuf, grad=None if gview is None else gview[:, :V], gview=gview)
    return o


def check_outputs(tag, o, ref, e, N, legacy=False):
    """`legacy`: alpha = 0, where loss and nll have the existing 1e-5 relative tolerance"""
    rt = 1e-5 if legacy else 0.0
    for k in ("row_loss", "row_nll", "row_ul"):
        close("%s %s" % (tag, k), o[k][:N], ref[k], e[k])
        assert all_nan(o[k][N:]), (tag, k)
    for k in ("loss", "nll", "ul"):
        close("%s %s" % (tag, k), o[k][:1], ref[k].reshape(1), e[k], rtol=0.0 if k == "ul" else rt)
        assert all_nan(o[k][1:]), (tag, k)


# ---------------------------------------------------------------------------------------------- A. sat_ce_rows_ul

@pytest.mark.parametrize("alpha,eps", UR.UL_SETTINGS)
@pytest.mark.parametrize("V", UR.UL_V)
def test_ce_rows_ul_paths_tails_candidate_edges_and_gradient_forms(lib, V, alpha, eps):
    logits, targets, lengths = UR.ul_inputs(V)
    ref = cached(("ul", V, alpha, eps), lambda: UR.ul_autograd(logits.double(), targets, lengths, eps, alpha, R.CE_INV))
    e = UR.f32_err("ul", V, alpha, eps)
    N = logits.shape[0]
    for ldl, offset in [(ldl, 0) for ldl in sorted({L.pad4(V), V + 4})] + [(L.pad4(V), 1)]:
        tag = "ul V %d alpha %g eps %g ldl %d%s" % (V, alpha, eps, ldl, " base+1" if offset else "")
        a = ul_call(lib, logits, targets, lengths, V, ldl, eps, alpha, "inplace", offset=offset)
        check_outputs(tag + " in place", a, ref, e, N)
        close(tag + " in place grad", a["grad"], ref["grad"], e["grad"])
        grad_bits = a["grad"].clone()
        a["view"][:, :V] = a["before"][offset:offset + N * ldl].view(N, ldl)[:, :V]         # then only pads and guards can differ
        assert same_bits(a["buf"], a["before"]), tag + ": pads or guards changed"
        # out of place, the path the logits choose: the same bits, the logits untouched, the gradient's pads and guard left alone
        ldg = L.pad4(V) + 4
        b = ul_call(lib, logits, targets, lengths, V, ldl, eps, alpha, "out", ldg=ldg, offset=offset)
        assert same_bits(b["grad"], grad_bits), tag + ": out of place differs from in place"
        assert same_bits(b["buf"], b["before"]), tag + ": out of place touched the logits"
        assert all_nan(b["gview"][:, V:]) and all_nan(b["gbuf"][N * ldg:]), tag
        # no gradient: the logits untouched; and two replays: the same bits
        c = ul_call(lib, logits, targets, lengths, V, ldl, eps, alpha, "none", offset=offset)
        assert same_bits(c["buf"], c["before"]), tag + ": grad = NULL touched the logits"
        for k in OUT:
            assert same_bits(b[k], a[k]) and same_bits(c[k], a[k]), (tag, k)
    # a gradient pitch that is no multiple of 4 (strided path whatever the logits allow)
    d = ul_call(lib, logits, targets, lengths, V, L.pad4(V), eps, alpha, "out", ldg=V + 1)
    check_outputs("ul V %d alpha %g eps %g ldg V+1" % (V, alpha, eps), d, ref, e, N)
    close("ul V %d alpha %g eps %g ldg V+1 grad" % (V, alpha, eps), d["grad"], ref["grad"], e["grad"])
    assert same_bits(d["buf"], d["before"]) and all_nan(d["gview"][:, V:]) and all_nan(d["gbuf"][N * (V + 1):])


@pytest.mark.parametrize("name,V", [(n, V) for n, Vs in UR.UL_PACK_V.items() for V in Vs])
def test_other_packs_no_candidates_and_every_lane_of_the_wave(lib, name, V):
    logits, targets, lengths = UR.ul_pack_inputs(name, V)
    ref = UR.ul_autograd(logits.double(), targets, lengths, 0.1, 1.0, R.CE_INV)
    e = UR.f32_err("ul_pack", name, V)
    N = logits.shape[0]
    for grad in ("inplace", "out"):
        o = ul_call(lib, logits, targets, lengths, V, L.pad4(V), 0.1, 1.0, grad, ldg=L.pad4(V))
        check_outputs("pack %s V %d %s" % (name, V, grad), o, ref, e, N)
        close("pack %s V %d %s grad" % (name, V, grad), o["grad"], ref["grad"], e["grad"])
    if lengths[0] == 1:
        # no candidates anywhere: plain rows, bit for bit sat_ce_rows_ls's
        buf = torch.zeros(N, L.pad4(V), device="cuda")
        buf[:, :V] = logits.cuda()
        rl, rn, lo, nl, tg = nans(N), nans(N), nans(1), nans(1), targets.cuda()
        L.check(lib.sat_ce_rows_ls(L.ptr(buf), L.pad4(V), L.ptr(tg), N, V, R.CE_INV, 0.1, L.ptr(buf), L.pad4(V), L.ptr(rl), L.ptr(rn),
                                   L.ptr(lo), L.ptr(nl), st()), "sat_ce_rows_ls")
        sync()
        assert same_bits(o["grad"], buf[:, :V]) and same_bits(o["row_loss"][:N], rl) and same_bits(o["loss"][:1], lo)
        assert float(o["row_ul"][:N].abs().max()) == 0 and float(o["ul"][0]) == 0


@pytest.mark.parametrize("V", UR.UL_CLAMP_V)
def test_clamp_rows_pay_exactly_the_clamped_term_and_carry_no_weight(lib, V):
    logits, targets, lengths = UR.ul_clamp_inputs(V)
    ref = UR.ul_autograd(logits.double(), targets, lengths, 0.0, 1.0, R.CE_INV)
    e = UR.f32_err("ul_clamp", V)
    o = ul_call(lib, logits, targets, lengths, V, L.pad4(V), 0.0, 1.0)
    check_outputs("clamp V %d" % V, o, ref, e, 12)
    close("clamp V %d grad" % V, o["grad"], ref["grad"], e["grad"])
    # row 3 = (t 1, b 0): its only candidate is the dominant column 0: the term is logf of the f32 constant 1e-5 and nothing else
    # (two faithful f32 logarithms differ by at most 2 ulp of 11.5)
    assert abs(float(o["row_ul"][3]) + float(np.log(np.float32(1e-5)))) <= 2 * 2.0 ** -20


def test_t_65_is_unsupported_in_c_and_a_value_error_in_python(lib):
    V, lengths = 8, [65]
    logits, targets = torch.zeros(65, V, device="cuda"), torch.zeros(65, dtype=torch.int64, device="cuda")
    pre = prefix_dev(lengths)
    rl = nans(65)
    before = logits.clone()
    rc = lib.sat_ce_rows_ul(L.ptr(logits), V, L.ptr(targets), L.ptr(pre), 65, 65, V, 1.0, 0.0, 1.0, L.ptr(logits), V, L.ptr(rl), None, None,
                            None, None, None, st())
    sync()
    assert rc == 1003 and all_nan(rl) and same_bits(logits, before)
    with pytest.raises(ValueError, match="64"):
        sat.cross_entropy(logits, targets, unlikelihood=1.0, lengths=lengths)
    with pytest.raises(ValueError, match="64"):
        sat.CrossEntropy(unlikelihood=1.0)(logits, targets, lengths)


@pytest.mark.parametrize("V", [1003, 12292])
def test_alpha_zero_is_sat_ce_rows_ls_and_sat_ce_rows_bit_for_bit(lib, V):
    """register path (1003) and strided path (12292): every output and the gradient; the existing tolerances hold too"""
    logits, targets, lengths = UR.ul_inputs(V)
    N, ldl = logits.shape[0], L.pad4(V)
    tg = targets.cuda()
    for eps in (0.1, 0.0):
        o = ul_call(lib, logits, targets, lengths, V, ldl, eps, 0.0)
        buf = nans(N * ldl + GUARD)
        buf[:N * ldl].view(N, ldl)[:, :V] = logits.cuda()
        rl, rn, lo, nl = nans(N + 1), nans(N + 1), nans(2), nans(2)
        L.check(lib.sat_ce_rows_ls(L.ptr(buf), ldl, L.ptr(tg), N, V, R.CE_INV, eps, L.ptr(buf), ldl, L.ptr(rl), L.ptr(rn), L.ptr(lo),
                                   L.ptr(nl), st()), "sat_ce_rows_ls")
        sync()
        assert same_bits(o["buf"], buf), (V, eps)
        for k, want in (("row_loss", rl), ("row_nll", rn), ("loss", lo), ("nll", nl)):
            assert same_bits(o[k], want), (V, eps, k)
        assert float(o["row_ul"][:N].abs().max()) == 0 and float(o["ul"][0]) == 0
        out = ul_call(lib, logits, targets, lengths, V, ldl, eps, 0.0, "out", ldg=ldl + 4)
        assert same_bits(out["grad"], buf[:N * ldl].view(N, ldl)[:, :V])
        ref = LR.ls_rows(logits.double(), targets, eps, R.CE_INV)
        close("alpha 0 V %d eps %g grad" % (V, eps), o["grad"], ref["grad"], 0.0, atol=GRAD_TOL)
        close("alpha 0 V %d eps %g loss" % (V, eps), o["loss"][:1], ref["loss"].reshape(1), 0.0, rtol=1e-5)
        close("alpha 0 V %d eps %g nll" % (V, eps), o["nll"][:1], ref["nll"].reshape(1), 0.0, rtol=1e-5)
    # smoothing 0 as well: sat_ce_rows
    buf = nans(N * ldl + GUARD)
    buf[:N * ldl].view(N, ldl)[:, :V] = logits.cuda()
    rl, lo = nans(N + 1), nans(2)
    L.check(lib.sat_ce_rows(L.ptr(buf), ldl, L.ptr(tg), N, V, R.CE_INV, 1, L.ptr(rl), L.ptr(lo), st()), "sat_ce_rows")
    sync()
    assert same_bits(o["row_loss"], rl) and same_bits(o["loss"], lo) and same_bits(o["buf"], buf)


@pytest.mark.parametrize("V", [1003, 12292])
def test_null_outputs_leave_the_other_outputs_bitwise_equal(lib, V):
    logits, targets, lengths = UR.ul_inputs(V)
    ldl = L.pad4(V)
    full = ul_call(lib, logits, targets, lengths, V, ldl, 0.1, 1.0)
    for give in (("row_nll", "row_ul", "loss"), ("row_ul", "ul"), ("row_nll", "nll"), ("loss",), ()):
        o = ul_call(lib, logits, targets, lengths, V, ldl, 0.1, 1.0, give=give)
        assert same_bits(o["buf"], full["buf"]), give
        for k in OUT:
            assert same_bits(o[k], full[k]) if (k in give or k == "row_loss") else all_nan(o[k]), (give, k)


@pytest.mark.parametrize("V", [1003, 12292])
def test_the_same_row_with_the_same_prefix_in_two_batches_has_the_same_bits(lib, V):
    """sequences 0, 3 and 6 of the sweep's pack, alone as the pack [12, 9, 4]: their rows' outputs do not depend on the batch"""
    logits, targets, lengths = UR.ul_inputs(V)
    ldl = L.pad4(V)
    a = ul_call(lib, logits, targets, lengths, V, ldl, 0.1, 1.0, "out", ldg=ldl)
    keep, sub = [0, 3, 6], [lengths[0], lengths[3], lengths[6]]
    pre = UR.prefix(lengths)
    rows = [pre[t] + keep[b] for t, b in UR.positions(sub)]
    b = ul_call(lib, logits[rows], targets[rows], sub, V, ldl, 0.1, 1.0, "out", ldg=ldl)
    assert float(b["row_ul"][:len(rows)].max()) > 0
    for k in ("row_loss", "row_nll", "row_ul"):
        assert same_bits(b[k][:len(rows)], a[k][rows]), k
    assert same_bits(b["grad"], a["grad"][rows])


# ---------------------------------------------------------------------------------------------- B. the bf16 form

def vocab_inputs(N, H, V):
    g = torch.Generator().manual_seed(N + V)
    return (torch.tanh(torch.randn(N, H, generator=g)).cuda(), torch.empty(V, H).uniform_(-0.1, 0.1, generator=g).cuda(),
            (torch.randn(V, generator=g) * 0.01).cuda(), torch.randint(0, min(V, 40), (N,), generator=g).cuda())


def bf16_path(lib, Hs, W, b, tg, lengths, eps, alpha):
    """(logits, row_loss, row_nll, row_ul, loss, nll, ul, dW, db, dHs) of sat_vocab_ce_fwd_bf16_ul (alpha None: _ls; eps None too: the
    plain call) + sat_vocab_ce_bwd_bf16"""
    (N, H), V = Hs.shape, W.shape[0]
    wb = lib.sat_vocab_bf16_ws_bytes(N, H, V)
    assert wb > 0
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    lg, rl, rn, ru, lo, nl, ul = nans(N, V), nans(N), nans(N), nans(N), nans(1), nans(1), nans(1)
    if eps is None:
        L.check(lib.sat_vocab_ce_fwd_bf16(L.ptr(Hs), L.ptr(W), L.ptr(b), L.ptr(tg), N, H, V, 1.0 / N, L.ptr(lg), V, L.ptr(rl), L.ptr(lo),
                                          L.ptr(ws), wb, st()), "sat_vocab_ce_fwd_bf16")
    elif alpha is None:
        L.check(lib.sat_vocab_ce_fwd_bf16_ls(L.ptr(Hs), L.ptr(W), L.ptr(b), L.ptr(tg), N, H, V, 1.0 / N, eps, L.ptr(lg), V, L.ptr(rl),
                                             L.ptr(rn), L.ptr(lo), L.ptr(nl), L.ptr(ws), wb, st()), "sat_vocab_ce_fwd_bf16_ls")
    else:
        pre = prefix_dev(lengths)
        L.check(lib.sat_vocab_ce_fwd_bf16_ul(L.ptr(Hs), L.ptr(W), L.ptr(b), L.ptr(tg), L.ptr(pre), lengths[0], N, H, V, 1.0 / N, eps,
                                             alpha, L.ptr(lg), V, L.ptr(rl), L.ptr(rn), L.ptr(ru), L.ptr(lo), L.ptr(nl), L.ptr(ul),
                                             L.ptr(ws), wb, st()), "sat_vocab_ce_fwd_bf16_ul")
    dW, db, dH = nans(V, H), nans(V), nans(N, H)
    L.check(lib.sat_vocab_ce_bwd_bf16(N, H, V, L.ptr(dW), L.ptr(db), L.ptr(dH), L.ptr(ws), wb, st()), "sat_vocab_ce_bwd_bf16")
    sync()
    return lg, rl, rn, ru, lo, nl, ul, dW, db, dH


@pytest.mark.parametrize("N,H,V,lengths", [(76, 64, 500, [20, 20, 20, 16]), (200, 128, 1000, [50] * 4), (8, 64, 12288, [4, 4])])
def test_vocab_ce_bf16_ul_vs_exact_f32_path_and_alpha_zero(lib, N, H, V, lengths):
    """the shapes of tests/test_gpu_label_smoothing.py and the tolerances of test_vocab_ce_bf16_path_vs_exact_f32_path
    (tests/test_gpu_kernels.py): sums 1e-3, gradients 1 % relative L2 against sat_vocab_logits_fwd + sat_ce_rows_ul + sat_vocab_ce_bwd;
    alpha = 0 is sat_vocab_ce_fwd_bf16_ls bit for bit, and with smoothing = 0 sat_vocab_ce_fwd_bf16"""
    eps, alpha = 0.1, 1.0
    assert sum(lengths) == N
    Hs, W, b, tg = vocab_inputs(N, H, V)
    pre = prefix_dev(lengths)
    lg32 = torch.empty(N, V, device="cuda")
    L.check(lib.sat_vocab_logits_fwd(L.ptr(Hs), L.ptr(W), L.ptr(b), N, H, V, L.ptr(lg32), V, st()), "sat_vocab_logits_fwd")
    rl32, rn32, ru32, lo32, nl32, ul32 = nans(N), nans(N), nans(N), nans(1), nans(1), nans(1)
    L.check(lib.sat_ce_rows_ul(L.ptr(lg32), V, L.ptr(tg), L.ptr(pre), lengths[0], N, V, 1.0 / N, eps, alpha, L.ptr(lg32), V, L.ptr(rl32),
                               L.ptr(rn32), L.ptr(ru32), L.ptr(lo32), L.ptr(nl32), L.ptr(ul32), st()), "sat_ce_rows_ul")
    wsb = lib.sat_vocab_ce_bwd_ws_bytes(N, H, V)
    ws = torch.empty(max(wsb // 4, 4), device="cuda")
    dW32, db32, dH32 = torch.empty(V, H, device="cuda"), torch.empty(V, device="cuda"), torch.empty(N, H, device="cuda")
    L.check(lib.sat_vocab_ce_bwd(L.ptr(lg32), V, L.ptr(Hs), L.ptr(W), N, H, V, L.ptr(dW32), L.ptr(db32), L.ptr(dH32), L.ptr(ws), wsb,
                                 st()), "sat_vocab_ce_bwd")
    lg, rl, rn, ru, lo, nl, ul, dW, db, dH = bf16_path(lib, Hs, W, b, tg, lengths, eps, alpha)
    for t in (lg, rl, rn, ru, lo, nl, ul, dW, db, dH):
        assert torch.isfinite(t).all()

    def rel(a, c):
        return ((a - c).norm() / c.norm()).item()
    print("bf16 ul N=%d H=%d V=%d: |dloss| %.2e |dnll| %.2e |dul| %.2e (ul %.3g), rel-L2 dW %.2e db %.2e dHs %.2e"
          % (N, H, V, abs(lo.item() - lo32.item()), abs(nl.item() - nl32.item()), abs(ul.item() - ul32.item()), ul32.item(),
             rel(dW, dW32), rel(db, db32), rel(dH, dH32)))
    assert ul32.item() > 0
    assert abs(lo.item() - lo32.item()) < 1e-3 and abs(nl.item() - nl32.item()) < 1e-3 and abs(ul.item() - ul32.item()) < 1e-3
    assert rel(dW, dW32) < 1e-2 and rel(db, db32) < 1e-2 and rel(dH, dH32) < 1e-2
    # alpha = 0: the label-smoothed call bit for bit, the logits written once and not modified; the gradient with alpha is another
    ls = bf16_path(lib, Hs, W, b, tg, lengths, eps, None)
    zero = bf16_path(lib, Hs, W, b, tg, lengths, eps, 0.0)
    assert same_bits(lg, ls[0]) and not same_bits(dW, ls[7])
    for i in (0, 1, 2, 4, 5, 7, 8, 9):
        assert same_bits(zero[i], ls[i]), i
    assert float(zero[3].abs().max()) == 0 and float(zero[6]) == 0
    plain = bf16_path(lib, Hs, W, b, tg, lengths, None, None)
    zz = bf16_path(lib, Hs, W, b, tg, lengths, 0.0, 0.0)
    for i in (0, 1, 4, 7, 8, 9):
        assert same_bits(zz[i], plain[i]), i
    # replay
    again = bf16_path(lib, Hs, W, b, tg, lengths, eps, alpha)
    for i, t in enumerate((lg, rl, rn, ru, lo, nl, ul, dW, db, dH)):
        assert same_bits(again[i], t), i


# ---------------------------------------------------------------------------------------------- C. the criterion

def torch_criterion(eps, alpha, lengths):
    """the reference on the device, through torch autograd: the fairseq formulation, mean over the rows; keeps the mean term"""
    def crit(out, targets):
        V = out.shape[1]
        lp = torch.log_softmax(out, 1)
        ce = torch.nn.functional.cross_entropy(out, targets, reduction="none", label_smoothing=eps)
        mask = UR.negative_mask(targets.cpu(), lengths, V, torch.float32).cuda()
        ul = (-torch.log(torch.clamp(1.0 - lp.exp(), min=UR.QMIN)) * mask).sum(1)
        crit.row_ul = ul.detach()
        return (ce + alpha * ul).mean()
    return crit


def make_decoder(E, H, V, Lh, seed=4):
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(seed))
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    return dec.cuda().train(), params


def inputs(B, E, V, width, seed=5, lo=4, hi=None):
    g = torch.Generator().manual_seed(seed)
    caps = torch.randint(lo, V if hi is None else hi, (B, width), generator=g)
    caps[:, 0] = 1
    return torch.randn(B, E, generator=g), caps


def compare_criteria(forward, params, targets, lengths, extra=None):
    """the same forward under the torch reference and under sat.CrossEntropy(0.1, unlikelihood=1.0): loss within 1e-4, every gradient
    rtol 1e-3 + 1e-7 (the criterion test of tests/test_gpu_label_smoothing.py), the outputs bitwise untouched, last_ul / last_row_ul
    within 1e-4 of the reference's"""
    def run(crit, *more):
        for p in params.values():
            p.grad = None
        out = forward()
        before = out.detach().clone()
        loss = crit(out, targets, *more)
        if extra is not None:
            loss = loss + extra()
        loss.backward()
        sync()
        assert same_bits(out.detach(), before), "the criterion changed the model's outputs"
        return loss.item(), before, {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
    ref = torch_criterion(0.1, 1.0, lengths)
    want_loss, out_t, want = run(ref)
    crit = sat.CrossEntropy(0.1, unlikelihood=1.0)
    got_loss, out_s, got = run(crit, lengths)
    assert same_bits(out_s, out_t)
    print("criterion: loss %.6f (torch %.6f), mean ul %.6f" % (got_loss, want_loss, crit.last_ul.item()))
    assert abs(got_loss - want_loss) < 1e-4, (got_loss, want_loss)
    assert set(got) == set(want) and len(got) > 0
    for k in want:
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k].cpu().numpy(), rtol=1e-3, atol=1e-7, err_msg=k)
    assert crit.last_ul.shape == (1,) and crit.last_row_ul.shape == ref.row_ul.shape and ref.row_ul.max().item() > 0
    assert abs(crit.last_ul.item() - ref.row_ul.mean().item()) < 1e-4
    assert (crit.last_row_ul - ref.row_ul).abs().max().item() < 1e-4
    plain = torch.nn.functional.cross_entropy(out_t, targets)
    assert abs(crit.last_nll.item() - plain.item()) < 1e-4
    crit.check_ids()                                            # every target was in range
    return crit


@pytest.mark.parametrize("Lh", [1, 2])
def test_criterion_on_a_small_decoder_equals_the_torch_reference(Lh):
    E, H, V = 32, 64, 1003
    dec, _ = make_decoder(E, H, V, Lh)
    feats, caps = inputs(len(LENGTHS), E, V, 12, hi=10)         # few ids: captions that repeat themselves
    targets, l1 = sat.pack_targets(caps.cuda(), LENGTHS)
    f = feats.cuda().requires_grad_(True)
    params = dict(dec.named_parameters())
    params["features"] = f
    compare_criteria(lambda: dec(f, caps[:, :-1].cuda(), l1), params, targets, l1)


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
        caps[b, 1:l - 1] = torch.randint(4, 9, (l - 2,), generator=g)
        caps[b, l - 1] = 2
    di, dc = images.cuda(), caps.cuda()
    targets, l1 = sat.pack_targets(dc, lengths)
    params = {k: p for k, p in model.named_parameters() if p.requires_grad}
    compare_criteria(lambda: model(di, dc[:, :-1], l1), params, targets, l1, extra=lambda: model.last_attention_penalty)


def test_criterion_function_form_and_unlikelihood_zero_is_todays_call():
    logits, targets, lengths = UR.ul_inputs(1003)
    N = logits.shape[0]
    x, t = logits.cuda().requires_grad_(True), targets.clamp(0, 1002).cuda()
    out = {}
    loss = sat.cross_entropy(x, t, 0.1, out=out, unlikelihood=0.5, lengths=lengths)
    ref = UR.ul_autograd(logits.double(), targets, lengths, 0.1, 0.5, 1.0 / N)
    assert loss.dim() == 0 and abs(loss.item() - ref["loss"].item()) < 1e-5 * ref["loss"].item()
    assert abs(out["last_ul"].item() - ref["ul"].item()) < 1e-5 and out["last_row_ul"].shape == (N,)
    (2 * loss).backward()
    assert (x.grad.double().cpu() - 2 * ref["grad"]).abs().max().item() <= 2 * R.TOL_FACTOR * UR.f32_err("ul", 1003, 0.5, 0.1)["grad"] * 50 / N
    # unlikelihood = 0: the bits of the call without the keyword, zeros for the term, no lengths needed
    o0, o1 = {}, {}
    a = sat.cross_entropy(x.detach(), t, 0.1, out=o0)
    b = sat.cross_entropy(x.detach(), t, 0.1, out=o1, unlikelihood=0.0, lengths=lengths)
    assert same_bits(a.view(1), b.view(1)) and same_bits(o0["last_nll"], o1["last_nll"])
    assert float(o1["last_ul"]) == 0 and float(o1["last_row_ul"].abs().max()) == 0


# ---------------------------------------------------------------------------------------------- D. TrainStep

def ts_model(E, H, V, Lh, dtype, seed=4):
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY, compute_dtype=dtype)
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(seed))
    model.decoder.load_state_dict(params)
    return model.cuda().train(), params


@pytest.mark.parametrize("ss_prob", [0.0, 0.5])
@pytest.mark.parametrize("Lh", [1, 2])
def test_trainstep_f32_mode_against_the_oracle_backward_of_the_reference_gradient(Lh, ss_prob):
    """the pattern of test_trainstep_exact_mode_parity_on_used (tests/test_gpu_ss.py): loss 1e-4, gradients rtol 1e-3 + 1e-7.  With
    ss_prob > 0 the oracle runs on the tokens the step fed, and the candidates are still the ground-truth targets"""
    E, H, V = 32, 64, 1003
    model, params = ts_model(E, H, V, Lh, "f32")
    model.decoder.ss_prob = ss_prob
    feats, caps = inputs(len(LENGTHS), E, V, 12, seed=6, hi=10)
    ts = sat.TrainStep(model, label_smoothing=0.1)
    ts.unlikelihood = 1.0
    assert ts.decoder_gemm_dtype == "f32" and ts.unlikelihood == 1.0
    n_tok = sum(l - 1 for l in LENGTHS)
    torch.manual_seed(3)
    loss = ts.forward_backward((feats.cuda(), caps.cuda(), LENGTHS), 1.0 / n_tok)
    targets, l1 = sat.pack_targets(caps.cuda(), LENGTHS)
    fed = caps[:, :-1]
    if ss_prob > 0:
        fed = model.decoder.last_ss_inputs.cpu()
        assert not torch.equal(fed, caps[:, :fed.shape[1]])
    ref_logits, tape = OD.decoder_forward(params, feats, fed, l1, Lh, keep=True)
    ref = UR.ul_autograd(ref_logits.double(), targets.cpu(), l1, 0.1, 1.0, 1.0 / n_tok)
    print("step Lh %d ss %g: loss %.6f (ref %.6f) ul %.6f (ref %.6f)" % (Lh, ss_prob, loss.item(), ref["loss"].item(),
                                                                        ts.last_ul.item(), ref["ul"].item()))
    assert ref["ul"].item() > 0
    assert abs(loss.item() - ref["loss"].item()) < 1e-4
    assert ts.last_nll.shape == (1,) and abs(ts.last_nll.item() - ref["nll"].item()) < 1e-4
    assert ts.last_ul.shape == (1,) and abs(ts.last_ul.item() - ref["ul"].item()) < 1e-4
    grads, d_feat = OD.decoder_backward(params, tape, fed, l1, ref["grad"].float(), Lh)
    np.testing.assert_allclose(ts.last_d_features.cpu().numpy(), d_feat.numpy(), rtol=1e-3, atol=1e-7)
    for k, p in model.decoder.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k].numpy(), rtol=1e-3, atol=1e-7, err_msg=k)


def test_trainstep_bf16_mode_loss_replay_sampling_and_dropout():
    """E 64, H 64, V 1000: loss, nll and ul within 2e-3 of the f32-mode step (the bf16 CE tolerance of
    test_trainstep_bf16_cfg1_shape_reproducible_and_learns); identical calls, and replays under ss_prob / dropout_p, bit for bit"""
    E, H, V = 64, 64, 1000
    feats, caps = inputs(len(LENGTHS), E, V, 12, seed=7, hi=10)
    batch = (feats.cuda(), caps.cuda(), LENGTHS)
    n_tok = sum(l - 1 for l in LENGTHS)
    m32, _ = ts_model(E, H, V, 1, "f32")
    t32 = sat.TrainStep(m32)
    t32.unlikelihood = 1.0
    loss32 = t32.forward_backward(batch, 1.0 / n_tok).item()
    nll32, ul32 = t32.last_nll.item(), t32.last_ul.item()
    model, _ = ts_model(E, H, V, 1, "bf16")
    ts = sat.TrainStep(model)
    ts.unlikelihood = 1.0                                       # the settable attribute
    assert ts.decoder_gemm_dtype == "bf16" and t32.decoder_gemm_dtype == "f32"

    def run(seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        loss = ts.forward_backward(batch, 1.0 / n_tok).clone()
        return loss, ts.flat_grad.clone(), ts.last_nll.clone(), ts.last_ul.clone()
    l0, g0, n0, u0 = run()
    l1, g1, n1, u1 = run()
    print("bf16 step: loss %.6f (f32 %.6f) nll %.6f (%.6f) ul %.6f (%.6f)" % (l0.item(), loss32, n0.item(), nll32, u0.item(), ul32))
    assert ul32 > 0
    assert abs(l0.item() - loss32) < 2e-3 and abs(n0.item() - nll32) < 2e-3 and abs(u0.item() - ul32) < 2e-3
    assert not same_bits(l0, n0)                                # the loss slot holds the whole loss, last_nll the plain one
    assert same_bits(l0, l1) and same_bits(g0, g1) and same_bits(n0, n1) and same_bits(u0, u1)
    assert torch.isfinite(g0).all() and float(g0.abs().sum()) > 0
    model.decoder.ss_prob = 0.5
    a, b, c = run(21), run(21), run(22)
    assert all(same_bits(a[i], b[i]) for i in range(4)) and not same_bits(a[1], c[1])
    assert not same_bits(a[1], g0) and torch.isfinite(a[1]).all()
    model.decoder.ss_prob = 0.0
    model.decoder.dropout_p = 0.5
    a, b, c = run(31), run(31), run(32)
    assert all(same_bits(a[i], b[i]) for i in range(4)) and not same_bits(a[1], c[1])
    assert not same_bits(a[1], g0) and torch.isfinite(a[1]).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_trainstep_unlikelihood_zero_is_the_step_without_the_attribute(dtype):
    """the same calls (spied on the library object) and the same bits"""
    E, H, V = 64, 64, 1000
    feats, caps = inputs(len(LENGTHS), E, V, 12, seed=8)
    batch = (feats.cuda(), caps.cuda(), LENGTHS)
    n_tok = sum(l - 1 for l in LENGTHS)
    out = []
    for alpha in (None, 0.0, 1.0):
        model, _ = ts_model(E, H, V, 1, dtype)
        ts = sat.TrainStep(model)
        if alpha is not None:
            ts.unlikelihood = alpha
        calls = []

        class Spy:
            def __getattr__(self, name, lib=ts.lib):
                fn = getattr(lib, name)
                if name.startswith("sat_ce_rows") or name.startswith("sat_vocab_ce_fwd"):
                    calls.append(name)
                return fn
        ts.lib = Spy()
        loss = ts.forward_backward(batch, 1.0 / n_tok)
        out.append((loss.clone(), ts.flat_grad.clone(), calls, ts.last_nll.data_ptr() == loss.data_ptr(), ts.last_ul))
    assert out[0][2] == out[1][2] == (["sat_ce_rows"] if dtype == "f32" else ["sat_vocab_ce_fwd_bf16"])
    assert out[2][2] == (["sat_ce_rows_ul"] if dtype == "f32" else ["sat_vocab_ce_fwd_bf16_ul"])
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])
    assert out[0][3] and out[1][3] and not out[2][3]            # with 0 the loss is the NLL: the loss slot itself
    assert out[0][4] is None and out[1][4] is None and out[2][4].shape == (1,)
    assert not same_bits(out[2][1], out[0][1]) and torch.isfinite(out[2][1]).all()
