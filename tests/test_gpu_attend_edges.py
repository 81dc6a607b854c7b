"""GPU (MI355X): the step kernels of the attention decoder at the shapes where their branches change -- `sat_attention_fwd / _bwd /
_bwd_ex`, `sat_attention_coverage`, `sat_lstmcell_fwd`, `sat_lstm_step`, `sat_lstmcell_bwd_point`, `sat_gemm_f32_splitk` +
`sat_sum_slabs_f32` and the row utilities, each through the C ABI against the float64 reference of tests/attend_step_reference.py
(validated on the CPU by tests/test_attend_step_reference_host.py).

Buffers a kernel promises to overwrite start as NaN, buffers it accumulates into start random, strided destinations and the row
after the last carry NaN guards that must survive.

Attention shapes (rows, P, C) and what each reaches:
  (1, 1, 4)      P = 1: alpha exactly 1, context = feats; minimum C
  (3, 3, 4)      fewer positions than the 4 row-dot waves and the 8 channel waves
  (2, 5, 36)     P not a multiple of 4 (LDS carving by P4); C < 64 and not a multiple of 64
  (7, 9, 68)     P = 8 + 1; the second 64-channel chunk has 4 live lanes
  (1, 197, 260)  rows = 1: the most position chunks; odd P; C > 256 and not a multiple of 256
  (600, 8, 64)   rows > 512: one position chunk per row; P = the wave count
  (2, 1030, 8)   P > 2 * 512: the softmax loops run more than once per thread; P % 4 == 2
  (5, 196, 512)  the shape of test_attention_fwd_bwd_kernels_vs_fp64
LSTM shapes (B, In, H): (1,4,4) one K block, seven idle waves; (5,20,20) K not a multiple of 16; (65,36,48) a second 64-row
chunk with one live row; (64,64,64) a full chunk; (3,1028,8) long K against a tiny H.

Tolerances.  An output passes when it meets the tolerance the existing one-shape tests use for it (alpha, context 2e-7 abs;
d_ctx_enc 3e-7 abs; d_proj, d_w_att rtol 1e-4 + 1e-6; d_feats rtol 1e-4 + 1e-8: test_attention_fwd_bwd_kernels_vs_fp64; the
split-K GEMM 3e-6 x max |A||B|: test_gemm_f32; coverage T^2 2^-24 and 1e-5 relative: test_attention_coverage_vs_fp64, plus
3 T 2^-24 on the gradient, see there) OR lies within 8 x the error of the float32 torch restatement of the same formula against
float64 at that shape and seed (the kernel sums wave-strided, then through LDS in wave order; torch sums otherwise).  The LSTM
kernels have no earlier kernel-level tolerance: 8 x the restatement's error only.  Nothing here is set from a kernel's output.
The restatement's max abs errors, as the host test measured them (`pytest -s tests/test_attend_step_reference_host.py`) and as
attend_step_reference.F32_ERR keeps them (torch's float32 sums depend on the host CPU, so the table is frozen; the host test
re-measures).  d_ce = d_ctx_enc; acc_* are the accumulated buffers as left in memory; "extra" rows are sat_attention_bwd_ex with
scale 0.37 on alpha:

  case     (rows, P, C)    alpha    context  d_ce     d_proj   d_w_att  d_feats  acc_ce   acc_feats
           (1, 1, 4)       0        0        0        0        0        0        0        1e-07
           (3, 3, 4)       1.4e-08  1.3e-08  6.3e-10  7.7e-10  5.1e-09  1.3e-08  1.4e-09  1.7e-08
           (2, 5, 36)      1.8e-08  2.3e-08  3.9e-09  6.6e-09  4.7e-08  1.3e-08  4.1e-09  1.5e-08
           (7, 9, 68)      2.6e-08  1.6e-08  6.2e-09  1.5e-08  1.4e-07  7.3e-09  6.4e-09  1e-08
           (1, 197, 260)   2.8e-09  4.3e-10  6.5e-11  4.4e-10  2.2e-09  4.8e-11  2.1e-09  3.2e-09
           (600, 8, 64)    4.4e-08  3.7e-08  1.9e-08  4.4e-08  1.7e-06  2e-08    1.9e-08  2e-08
           (2, 1030, 8)    1.6e-10  5e-11    1.9e-13  7.8e-12  3.2e-11  4.5e-13  3e-09    3.7e-09
           (5, 196, 512)   2.3e-08  5.9e-10  4.5e-10  6.4e-10  1.2e-08  4e-10    3.6e-09  3.6e-09
  extra    (2, 5, 36)      1.8e-08  2.3e-08  4.3e-09  9.9e-09  3.9e-08  1.3e-08  6.1e-09  1.5e-08
  extra    (7, 9, 68)      2.6e-08  1.6e-08  1.4e-08  3.5e-08  2.2e-07  7.3e-09  1.5e-08  1e-08
  extra    (1, 197, 260)   2.8e-09  4.3e-10  6.7e-10  1.6e-09  1.5e-08  4.8e-11  2.6e-09  3.2e-09
  zero_w   (2, 5, 36)      3e-09    2e-08    0        0        5.4e-08  4.5e-09  0        6.7e-09
  large    (2, 5, 36)      2.8e-11  1.2e-08  3.2e-10  3.2e-10  1.3e-11  2.4e-08  3.2e-10  2.5e-08
  dominant (2, 5, 36)      7.7e-24  1.2e-08  4.2e-23  6.6e-23  1.8e-23  2.4e-08  6.9e-18  2.5e-08
  zero_w   (5, 196, 512)   1e-10    4.9e-10  0        0        1e-08    6.3e-12  0        3.6e-09
  large    (5, 196, 512)   3.4e-07  5.2e-09  2.4e-07  1.4e-07  7.2e-08  5.1e-09  2.4e-07  5.9e-09
  dominant (5, 196, 512)   4.7e-15  6.1e-10  4.3e-19  4.3e-19  1.6e-16  9.1e-10  3.5e-18  2.2e-09

  lstmcell (1, 4, 4)       h 1.8e-08  c 1.7e-07  gates 6.2e-08
  lstmcell (5, 20, 20)     h 6.1e-08  c 1.7e-07  gates 1.6e-07
  lstmcell (65, 36, 48)    h 1e-07    c 3e-07    gates 2.7e-07
  lstmcell (64, 64, 64)    h 1.2e-07  c 2.5e-07  gates 3.7e-07
  lstmcell (3, 1028, 8)    h 2.3e-07  c 6.2e-07  gates 7.3e-07
  DG/dc_state per (n_carry 0, n/2, n) x (c_prev NULL, given):
  bwd_point (1, 4)    4.1e-08/2.8e-08 4.1e-08/2.8e-08 5.4e-08/3.9e-08 5.4e-08/3.9e-08
  bwd_point (5, 20)   4.2e-08/5.4e-08 4.2e-08/5.4e-08 7.5e-08/8e-08 1.4e-07/8e-08 7.5e-08/8e-08 1.4e-07/8e-08
  bwd_point (64, 64)  1.2e-07/1.1e-07 1.2e-07/1.1e-07 1.7e-07/1.9e-07 1.7e-07/1.9e-07 1.9e-07/2.4e-07 1.9e-07/2.4e-07
  bwd_point (300, 12) 1e-07/1.4e-07 1e-07/1.4e-07 2e-07/2.1e-07 2.1e-07/2.1e-07 2.2e-07/2.4e-07 2.2e-07/2.4e-07
"""
import importlib

import numpy as np
import pytest
import torch

import attend_step_reference as R

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

NAN = float("nan")


def st():
    return L.stream()


def sid(shape):
    return "x".join(str(v) for v in shape)


def sync():
    torch.cuda.synchronize()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def same_bits(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def all_nan(t):
    return bool(torch.isnan(t).all())


def strided(src, ld, fill=NAN):
    """device copy of the 2-D `src` with row pitch ld > cols, the pad columns NaN: a kernel that reads or writes them shows"""
    out = torch.full((src.shape[0], ld), fill, device="cuda", dtype=src.dtype)
    out[:, :src.shape[1]] = src.cuda()
    return out


def close(tag, got, ref, e32, rtol=0.0, atol=0.0, delta_of=None):
    """got (f32, device or host) against ref (f64): the existing tolerance |err| <= atol + rtol |ref| (of the increment `ref -
    delta_of` for an accumulated buffer), or 8 x the f32 restatement's error `e32`; prints the figures before it asserts"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert torch.isfinite(got).all(), tag + ": inf or NaN in the output"
    err = (got - ref).abs()
    mag = (ref - delta_of).abs() if delta_of is not None else ref.abs()
    legacy = (atol > 0 or rtol > 0) and bool((err <= atol + rtol * mag).all())
    worst = err.max().item() if err.numel() else 0.0
    print("%-44s err %.3g   f32 restatement %.3g   existing tolerance %s" % (tag, worst, e32, "met" if legacy else "not met"))
    assert legacy or worst <= R.TOL_FACTOR * e32, "%s: err %.3g > %g x %.3g" % (tag, worst, R.TOL_FACTOR, e32)


# ---------------------------------------------------------------------------------------------- A. attention step

_ATT = {}


def att_case(shape, kind="plain", extra=False):
    """inputs (host f32 and device), float64 results and the restatement's frozen errors of one case: computed once, never modified"""
    key = (shape, kind, extra)
    if key not in _ATT:
        d = R.attention_inputs(*shape, kind=kind)
        _ATT[key] = dict(d=d, dev={k: v.cuda() for k, v in d.items()}, r64=R.attention_case(*shape, kind=kind, extra=extra),
                         e32=R.f32_err("att", shape, kind, extra))
    return _ATT[key]


def att_fwd(lib, c, shape, with_alpha=True):
    """sat_attention_fwd with ld_proj = C + 4 and ld_ctx = C + 8; returns alpha [rows,P] (or None), the whole context buffer
    [rows, C+8] (the context in columns 4 .. C+3) and the workspace with its 4-float NaN tail"""
    rows, P, C = shape
    dv = c["dev"]
    proj = strided(c["d"]["proj"], C + 4)
    alpha = nans(rows, P) if with_alpha else None
    ctx = nans(rows, C + 8)
    n = lib.sat_attention_ws_bytes(rows, P) // 4
    assert n == rows * P
    ws = nans(n + 4)
    L.check(lib.sat_attention_fwd(dv["ce"].data_ptr(), dv["fe"].data_ptr(), proj.data_ptr(), C + 4, dv["w"].data_ptr(), rows, P, C,
                                  L.ptr(alpha), ctx.data_ptr() + 16, C + 8, ws.data_ptr(), n * 4, st()), "sat_attention_fwd")
    sync()
    assert all_nan(ctx[:, :4]) and all_nan(ctx[:, 4 + C:]) and all_nan(ws[n:])
    return alpha, ctx, ws


def att_bwd(lib, c, shape, alpha, split, with_dfeats, extra=False):
    """sat_attention_bwd (or _bwd_ex with ld_extra = P + 3 and a device scalar) with ld_dctx = C + 4; `split`: d_ctx arrives as two
    addends.  Returns the accumulated d_ctx_enc, d_proj, d_w_att partials [rows,C], the accumulated d_feats (or None)."""
    rows, P, C = shape
    dv, d = c["dev"], c["d"]
    proj = strided(d["proj"], C + 4)
    if split:
        half = d["dctx"] * 0.25
        dctx, dctx2 = strided(half, C + 4), (d["dctx"] - half).cuda()
    else:
        dctx, dctx2 = strided(d["dctx"], C + 4), None
    dce = dv["pre_dce"].clone()
    dfe = dv["pre_dfe"].clone() if with_dfeats else None
    dpj, dwp = nans(rows + 1, C), nans(rows + 1, C)                   # row `rows` is a guard
    n = rows * P
    ws = nans(n + 4)
    head = (dv["ce"].data_ptr(), dv["fe"].data_ptr(), proj.data_ptr(), C + 4, dv["w"].data_ptr(), alpha.data_ptr(), dctx.data_ptr(), C + 4,
            L.ptr(dctx2), C)
    tail = (rows, P, C, dce.data_ptr(), dpj.data_ptr(), dwp.data_ptr(), L.ptr(dfe), ws.data_ptr(), n * 4, st())
    if extra:
        ex = strided(d["extra"], P + 3)
        sc = torch.tensor([R.EX_SCALE], device="cuda")
        L.check(lib.sat_attention_bwd_ex(*head, ex.data_ptr(), P + 3, sc.data_ptr(), *tail), "sat_attention_bwd_ex")
    else:
        L.check(lib.sat_attention_bwd(*head, *tail), "sat_attention_bwd")
    sync()
    assert all_nan(dpj[rows:]) and all_nan(dwp[rows:]) and all_nan(ws[n:])
    return dce, dpj[:rows], dwp[:rows], dfe


def check_bwd(tag, c, out, with_dfeats):
    """the tolerances of test_attention_fwd_bwd_kernels_vs_fp64 for the same outputs, or 8 x the restatement's error"""
    dce, dpj, dwp, dfe = out
    r64, e32, d = c["r64"], c["e32"], c["d"]
    close(tag + " d_ctx_enc (accumulated)", dce, r64["acc_ctx_enc"], e32["acc_ctx_enc"], atol=3e-7, delta_of=d["pre_dce"].double())
    close(tag + " d_proj", dpj, r64["d_proj"], e32["d_proj"], rtol=1e-4, atol=1e-6)
    close(tag + " d_w_att (sum of the row partials)", dwp.double().sum(0), r64["d_w_att"], e32["d_w_att"], rtol=1e-4, atol=1e-6)
    if with_dfeats:
        close(tag + " d_feats (accumulated)", dfe, r64["acc_feats"], e32["acc_feats"], rtol=1e-4, atol=1e-8, delta_of=d["pre_dfe"].double())


@pytest.mark.parametrize("shape", R.ATT_SHAPES, ids=sid)
def test_attention_fwd_at_shape_edges(shape):
    lib = L.load()
    rows, P, C = shape
    c = att_case(shape)
    alpha, ctx, _ = att_fwd(lib, c, shape, True)
    none, ctx2, _ = att_fwd(lib, c, shape, False)
    assert none is None and same_bits(ctx, ctx2)                      # alpha = NULL changes nothing else
    close("%s alpha" % (shape,), alpha, c["r64"]["alpha"], c["e32"]["alpha"], atol=2e-7)
    close("%s context" % (shape,), ctx[:, 4:4 + C], c["r64"]["context"], c["e32"]["context"], atol=2e-7)
    assert (alpha.double().sum(1) - 1).abs().max().item() < 1e-6
    if P == 1:
        assert torch.equal(alpha.cpu(), torch.ones(rows, 1)) and torch.equal(ctx[:, 4:4 + C].cpu(), c["d"]["fe"][:, 0])


@pytest.mark.parametrize("shape", R.ATT_SHAPES, ids=sid)
def test_attention_bwd_at_shape_edges(shape):
    lib = L.load()
    c = att_case(shape)
    alpha = att_fwd(lib, c, shape, True)[0]
    for split in (False, True):
        full = att_bwd(lib, c, shape, alpha, split, True)
        check_bwd("%s d_ctx2 %s" % (shape, "given" if split else "NULL"), c, full, True)
        bare = att_bwd(lib, c, shape, alpha, split, False)
        assert bare[3] is None and all(same_bits(a, b) for a, b in zip(full[:3], bare[:3]))      # d_feats = NULL: the rest, bit for bit


@pytest.mark.parametrize("shape", R.ATT_EX_SHAPES, ids=sid)
def test_attention_bwd_ex_at_shape_edges(shape):
    lib = L.load()
    c = att_case(shape, extra=True)
    alpha = att_fwd(lib, c, shape, True)[0]
    out = att_bwd(lib, c, shape, alpha, False, True, extra=True)
    check_bwd("%s extra" % (shape,), c, out, True)
    plain = att_bwd(lib, c, shape, alpha, False, True)
    assert not same_bits(out[1], plain[1])                            # the extra gradient arrived


@pytest.mark.parametrize("shape", R.ATT_VALUE_SHAPES, ids=sid)
@pytest.mark.parametrize("kind", R.ATT_VALUE_KINDS)
def test_attention_value_cases(shape, kind):
    lib = L.load()
    rows, P, C = shape
    c = att_case(shape, kind)
    tag = "%s %s" % (kind, shape)
    alpha, ctx, _ = att_fwd(lib, c, shape, True)
    close(tag + " alpha", alpha, c["r64"]["alpha"], c["e32"]["alpha"], atol=2e-7)
    close(tag + " context", ctx[:, 4:4 + C], c["r64"]["context"], c["e32"]["context"], atol=2e-7)
    out = att_bwd(lib, c, shape, alpha, False, True)
    check_bwd(tag, c, out, True)                                      # every output finite (close() asserts it)
    if kind == "zero_w":
        assert torch.equal(alpha, alpha[:, :1].expand(rows, P)), "alpha must be uniform"
        assert same_bits(out[0], c["dev"]["pre_dce"]), "w_att = 0 adds exact zeros to d_ctx_enc"
    if kind == "dominant":
        assert (alpha.max(1)[0] > 1 - 1e-6).all()


def test_attention_limits_return_before_any_launch():
    lib = L.load()

    def fwd(rows, P, C, ws_short=0):
        ce, fe, pj, w = (torch.zeros(*s, device="cuda") for s in ((rows, P, C), (rows, P, C), (rows, C), (C,)))
        al, co, ws = nans(rows, P), nans(rows, C), nans(rows * P)
        rc = lib.sat_attention_fwd(ce.data_ptr(), fe.data_ptr(), pj.data_ptr(), C, w.data_ptr(), rows, P, C, al.data_ptr(), co.data_ptr(),
                                   C, ws.data_ptr(), rows * P * 4 - ws_short, st())
        sync()
        assert all_nan(al) and all_nan(co) and all_nan(ws)            # nothing ran
        return rc
    assert fwd(1, 15300, 4) == L.SAT_ERR_UNSUPPORTED                  # the softmax row no longer fits the LDS
    assert fwd(1, 1, 7684) == L.SAT_ERR_UNSUPPORTED                   # neither do proj and w_att
    assert fwd(2, 5, 6) == L.SAT_ERR_ARG                              # C % 4
    assert fwd(2, 5, 8, ws_short=4) == L.SAT_ERR_WORKSPACE
    rows, P, C = 2, 5, 8
    z = lambda *s: torch.zeros(*s, device="cuda")
    ce, fe, pj, w, al, dc = z(rows, P, C), z(rows, P, C), z(rows, C), z(C), z(rows, P), z(rows, C)
    dce, dpj, dwp, ws = nans(rows, P, C), nans(rows, C), nans(rows, C), nans(rows * P)
    args = lambda C_, wsb: (ce.data_ptr(), fe.data_ptr(), pj.data_ptr(), C, w.data_ptr(), al.data_ptr(), dc.data_ptr(), C, None, 0, rows, P, C_,
                            dce.data_ptr(), dpj.data_ptr(), dwp.data_ptr(), None, ws.data_ptr(), wsb, st())
    assert lib.sat_attention_bwd(*args(C, rows * P * 4 - 4)) == L.SAT_ERR_WORKSPACE        # 4 bytes short
    assert lib.sat_attention_bwd(*args(6, rows * P * 4)) == L.SAT_ERR_ARG
    sync()
    assert all_nan(dce) and all_nan(dpj) and all_nan(dwp) and all_nan(ws)


# ---------------------------------------------------------------------------------------------- B. coverage

# test_gpu_alpha.py::test_attention_coverage_vs_fp64 covers P = 196 and 13 with lengths [6, 6, 4, 2, 1]; none of the cases below
# repeats one of those, so none is skipped.
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_attention_coverage_at_chunk_edges(P):
    lib = L.load()
    for lengths in ([1], [4], [6, 6, 4, 2, 1], [1, 1, 1, 1, 1], [3, 3, 3, 1, 1]):     # B = 1 and 5; T = 1; ragged; ties
        B, T = len(lengths), lengths[0]
        pi = sat.PackInfo(lengths, "cuda")
        g = torch.Generator().manual_seed(100 * P + 7 * B + T)
        alpha = torch.softmax(torch.randn(pi.N, P, generator=g) * 2, dim=1)
        coef = 0.37 / (B * P)
        cov64, grad64, pen64 = R.coverage(alpha.double(), pi.batch_sizes, coef)
        ad = alpha.cuda()
        wsb = lib.sat_attention_coverage_ws_bytes(B, P)
        assert wsb == B * ((P + 63) // 64) * 4
        res = []
        for with_cov in (True, False):
            cov, grad, pen, ws = (nans(B + 1, P) if with_cov else None), nans(B + 1, P), nans(2), nans(wsb // 4 + 1)
            L.check(lib.sat_attention_coverage(ad.data_ptr(), pi.prefix_dev.data_ptr(), T, B, P, coef, L.ptr(cov), grad.data_ptr(),
                                               pen.data_ptr(), ws.data_ptr(), wsb, st()), "sat_attention_coverage")
            sync()
            assert all_nan(grad[B:]) and all_nan(pen[1:]) and all_nan(ws[wsb // 4:]) and (cov is None or all_nan(cov[B:]))
            res.append((cov, grad[:B], pen[:1]))
        (cov, grad, pen), (_, grad2, pen2) = res
        assert same_bits(grad, grad2) and same_bits(pen, pen2)        # cov = NULL changes nothing else
        # cov: T f32 additions of values <= T (test_attention_coverage_vs_fp64).  grad = (2 coef) (cov - 1) adds three roundings of a
        # value |cov - 1| <= T: coef to f32, the subtraction, the product -- 2^-24 T each.  The earlier test (T = 6) folds them into
        # T^2 2^-24; at T = 1 they are the whole error, so they are counted here.
        tol = T * T * 2.0 ** -24
        tol_grad = tol + 3 * T * 2.0 ** -24
        ecov = (cov[:B].cpu().double() - cov64).abs().max().item()
        egrad = (grad.cpu().double() / (2 * coef) - (cov64 - 1)).abs().max().item()
        print("P %d lengths %s: cov err %.3g (tol %.3g), grad/(2 coef) err %.3g (tol %.3g), penalty %.8g vs %.8g"
              % (P, lengths, ecov, tol, egrad, tol_grad, pen.item(), pen64.item()))
        assert ecov <= tol and egrad <= tol_grad
        assert abs(pen.item() - pen64.item()) <= 1e-5 * abs(pen64.item())


# ---------------------------------------------------------------------------------------------- C. LSTM cell forward

@pytest.mark.parametrize("shape", R.LSTM_SHAPES, ids=sid)
def test_lstmcell_fwd_and_lstm_step_at_shape_edges(shape):
    lib = L.load()
    B, In, H = shape
    d = R.lstm_inputs(B, In, H)
    h64, c64, g64 = R.lstmcell_step(*[d[k].double() for k in ("x", "h", "c", "w_ih", "w_hh", "b_ih", "b_hh")])
    g64, e32 = torch.cat(g64, 1), R.f32_err("lstm", shape)
    dv = {k: v.cuda() for k, v in d.items()}

    def run(entry, tapes):
        c = nans(B + 1, H)                                            # row B is a guard in every output
        c[:B] = dv["c"]
        h_out = nans(B + 1, H)
        gates, c_tape = (nans(B + 1, 4 * H), nans(B + 1, H)) if tapes else (None, None)
        head = (dv["x"].data_ptr(), dv["h"].data_ptr(), c.data_ptr(), dv["w_ih"].data_ptr(), dv["w_hh"].data_ptr(), dv["b_ih"].data_ptr(),
                dv["b_hh"].data_ptr(), B, In, H, h_out.data_ptr())
        if entry == "cell":
            L.check(lib.sat_lstmcell_fwd(*head, L.ptr(gates), L.ptr(c_tape), st()), "sat_lstmcell_fwd")
        else:
            L.check(lib.sat_lstm_step(*head, st()), "sat_lstm_step")
        sync()
        assert all_nan(h_out[B:]) and all_nan(c[B:]) and (not tapes or (all_nan(gates[B:]) and all_nan(c_tape[B:])))
        return h_out[:B], c[:B], gates, c_tape
    h, c, gates, c_tape = run("cell", True)
    close("%s h" % (shape,), h, h64, e32["h"])
    close("%s c" % (shape,), c, c64, e32["c"])
    close("%s gates" % (shape,), gates[:B], g64, e32["gates"])
    assert same_bits(c_tape[:B], c)
    h2, c2, _, _ = run("cell", False)
    assert same_bits(h, h2) and same_bits(c, c2)                      # the tapes are optional and change nothing
    h3, c3, _, _ = run("step", False)
    assert same_bits(h, h3) and same_bits(c, c3)                      # sat_lstm_step is the same launch


# ---------------------------------------------------------------------------------------------- D. LSTM pointwise backward

@pytest.mark.parametrize("shape", R.BWD_POINT_SHAPES, ids=sid)
def test_lstmcell_bwd_point_at_carry_edges(shape):
    lib = L.load()
    n, H = shape
    d = R.bwd_point_inputs(n, H)
    dv = {k: v.cuda() for k, v in d.items()}
    for n_carry in sorted({0, n // 2, n}):
        for with_c_prev in (False, True):
            d64 = {k: v.double() for k, v in d.items()}
            dg64, dc64 = R.lstmcell_bwd_point(d64["dh_out"], d64["dh_carry"], n_carry, d64["gates"], d64["c"],
                                              d64["c_prev"] if with_c_prev else None, d64["dc_state"])
            e32 = R.f32_err("bwd_point", shape, n_carry, with_c_prev)
            dcs = nans(n + 1, H)
            dcs[:n] = dv["dc_state"]                                  # random: a row >= n_carry that reads it shows
            DG = nans(n + 1, 4 * H)
            L.check(lib.sat_lstmcell_bwd_point(dv["dh_out"].data_ptr(), dv["dh_carry"].data_ptr() if n_carry else None, n_carry,
                                               dv["gates"].data_ptr(), dv["c"].data_ptr(), dv["c_prev"].data_ptr() if with_c_prev else None,
                                               dcs.data_ptr(), DG.data_ptr(), n, H, st()), "sat_lstmcell_bwd_point")
            sync()
            assert all_nan(DG[n:]) and all_nan(dcs[n:])
            tag = "%s n_carry %d c_prev %s" % (shape, n_carry, "given" if with_c_prev else "NULL")
            close(tag + " DG", DG[:n], dg64, e32["DG"])
            close(tag + " dc_state = dc f", dcs[:n], dc64, e32["dc_state"])


# ---------------------------------------------------------------------------------------------- E. split-K GEMM

def splitk(lib, amode, bmode, A, B, M, N, K, ks, bias=None, bias2=None, gap=8):
    """A [M,K], B [N,K] host f32 -> (the slab buffer [ks, M*N + gap] as left by sat_gemm_f32_splitk, its [ks,M,N] view, the sum by
    sat_sum_slabs_f32).  amode 2
    stores A K-major with lda = M rounded up to 4 and a zero pad (the launcher's rule for M % 4 != 0)."""
    if amode == 0:
        Ad, lda = A.cuda(), K
    else:
        lda = (M + 3) // 4 * 4
        Ad = torch.zeros(K, lda, device="cuda")
        Ad[:, :M] = A.t().cuda()
    Bd, ldb = (B.cuda(), K) if bmode == 0 else (B.t().contiguous().cuda(), N)
    stride = M * N + gap
    slabs = nans(ks, stride)
    b1, b2 = (None if b is None else b.cuda() for b in (bias, bias2))
    L.check(lib.sat_gemm_f32_splitk(amode, bmode, Ad.data_ptr(), lda, Bd.data_ptr(), ldb, slabs.data_ptr(), N, L.ptr(b1), L.ptr(b2), M, N, K,
                                    ks, stride, st()), "sat_gemm_f32_splitk")
    out = nans(M * N + 4)
    L.check(lib.sat_sum_slabs_f32(slabs.data_ptr(), ks, stride, M * N, out.data_ptr(), st()), "sat_sum_slabs_f32")
    sync()
    assert all_nan(slabs[:, M * N:]) and all_nan(out[M * N:])         # the gap between slabs and the tail stay untouched
    return slabs, slabs[:, :M * N].reshape(ks, M, N), out[:M * N].view(M, N)


# every (amode, bmode) pair runs at every shape: K % 4 == 0 and N % 4 == 0 throughout, and M = 33 in amode 2 is legal with lda = 36
# and a zero pad; no case is skipped
@pytest.mark.parametrize("amode,bmode", [(0, 0), (0, 1), (2, 1), (2, 0)])
@pytest.mark.parametrize("M,N,K,ks", R.SPLITK_SHAPES)
def test_gemm_f32_splitk_and_sum_slabs(amode, bmode, M, N, K, ks):
    lib = L.load()
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, bias2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    prod = A.double() @ B.double().t()
    tol = 3e-6 * (A.abs().double() @ B.abs().double().t()).max().item()          # test_gemm_f32: exact-f32 MFMA, ~1e-7 sum |a b|
    raw, slabs, out = splitk(lib, amode, bmode, A, B, M, N, K, ks)
    err = (out.cpu().double() - prod).abs().max().item()
    print("(%d,%d) M %d N %d K %d ks %d: err %.3g (tol %.3g)" % (amode, bmode, M, N, K, ks, err, tol))
    assert torch.isfinite(slabs).all() and err < tol
    nk = (K + 31) // 32                                               # 32-wide K steps, dealt ceil(nk / ks) per slice
    per = (nk + ks - 1) // ks
    for z in range(ks):
        if z * per >= nk:
            assert float(slabs[z].abs().max()) == 0.0                 # a slice without K steps writes exact zeros
    # bias: documented as "bias in slice 0" -- the sum carries bias + bias2 exactly once, later slices none
    _, slabs_b, out_b = splitk(lib, amode, bmode, A, B, M, N, K, ks, bias, bias2)
    assert (out_b.cpu().double() - (prod + bias.double() + bias2.double())).abs().max().item() < tol
    assert all(same_bits(slabs_b[z], slabs[z]) for z in range(1, ks))
    assert ((slabs_b[0] - slabs[0]).cpu().double() - (bias.double() + bias2.double())).abs().max().item() < tol
    one = nans(M * N + 4)                                             # nslab = 1: a copy
    L.check(lib.sat_sum_slabs_f32(raw.data_ptr(), 1, raw.shape[1], M * N, one.data_ptr(), st()), "sat_sum_slabs_f32")
    sync()
    assert same_bits(one[:M * N], slabs[0].reshape(-1)) and all_nan(one[M * N:])


def test_gemm_f32_splitk_vgg_weight_gradient_form():
    """dW tap = dZp^T . shift(Xp): amode 2, bmode 1, M = N = 8 channels, K = 72 flat padded pixels (2 images of 6 x 6), B a
    pointer shift*Cin floats into the padded NHWC buffer (show-and-tell_amd/vgg.py); slab_stride > M*ldc with a NaN gap"""
    lib = L.load()
    cout = cin = 8
    wp, npix, ks = 6, 72, 3
    margin = wp + 1
    g = torch.Generator().manual_seed(61)
    dZp, Xp = torch.randn(npix, cout, generator=g), torch.randn(npix + 2 * margin, cin, generator=g)
    dZd, Xd = dZp.cuda(), Xp.cuda()
    stride = cout * cin + 8
    for shift in (0, 1, wp + 1):
        slabs = nans(ks, stride)
        L.check(lib.sat_gemm_f32_splitk(2, 1, dZd.data_ptr(), cout, Xd.data_ptr() + (margin + shift) * cin * 4, cin, slabs.data_ptr(), cin,
                                        None, None, cout, cin, npix, ks, stride, st()), "sat_gemm_f32_splitk")
        out = nans(cout * cin)
        L.check(lib.sat_sum_slabs_f32(slabs.data_ptr(), ks, stride, cout * cin, out.data_ptr(), st()), "sat_sum_slabs_f32")
        sync()
        assert all_nan(slabs[:, cout * cin:])
        Xs = Xp[margin + shift:margin + shift + npix]
        want = dZp.double().t() @ Xs.double()
        tol = 3e-6 * (dZp.abs().double().t() @ Xs.abs().double()).max().item()
        err = (out.view(cout, cin).cpu().double() - want).abs().max().item()
        print("shift %d: err %.3g (tol %.3g)" % (shift, err, tol))
        assert err < tol


# ---------------------------------------------------------------------------------------------- F. row utilities (bit-exact)

def scatter(lib, rows, ids, V):
    N, E = rows.shape
    rd, idd, tab = rows.cuda(), ids.cuda(), nans(V + 1, E)
    L.check(lib.sat_scatter_rows_add(rd.data_ptr(), idd.data_ptr(), N, E, V, tab.data_ptr(), st()), "sat_scatter_rows_add")
    sync()
    assert all_nan(tab[V:])
    want = R.scatter_rows_add_rowordered_f32(rows, ids, V)
    assert same_bits(tab[:V], want), "N %d: max diff %.3g" % (N, (tab[:V].cpu() - want).abs().max().item())
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[ids] = False
    assert float(tab[:V].cpu()[untouched].abs().sum()) == 0.0


@pytest.mark.parametrize("N", [1, 32, 33, 64, 65])
def test_scatter_rows_add_all_ids_equal(N):
    g = torch.Generator().manual_seed(70 + N)
    scatter(L.load(), torch.randn(N, 5, generator=g), torch.full((N,), 1, dtype=torch.int64), 3)


def test_scatter_rows_add_distinct_ids_and_lds_opt_in():
    lib = L.load()
    g = torch.Generator().manual_seed(71)
    scatter(lib, torch.randn(65, 5, generator=g), torch.randperm(70, generator=g)[:65], 70)
    N, E, V = 12000, 8, 50                                            # (12000 + 375) * 4 bytes of LDS > 48 KiB: the opt-in branch
    assert (N + (N + 31) // 32) * 4 > 48 * 1024
    scatter(lib, torch.randn(N, E, generator=g), torch.randint(0, V - 1, (N,), generator=g), V)      # id V-1 stays untouched


@pytest.mark.parametrize("col0", [0, 1])
def test_pack_tokens_edges(col0):
    lib = L.load()
    g = torch.Generator().manual_seed(72 + col0)
    for lengths in ([12] * 10 + [10] * 10 + [6] * 10 + [2] * 10, [1, 1, 1], [1]):     # N = 300 (two workgroups), ragged; T = 1
        B, T = len(lengths), lengths[0]
        caps = torch.randint(1, 1000, (B, T + col0 + 3), generator=g)               # cap_stride > T + col0
        pi = sat.PackInfo(lengths, "cuda")
        out = torch.full((pi.N + 1,), -1, dtype=torch.int64, device="cuda")
        cd = caps.cuda()
        L.check(lib.sat_pack_tokens(cd.data_ptr(), caps.shape[1], pi.prefix_dev.data_ptr(), T, pi.N, col0, out.data_ptr(), st()))
        sync()
        assert pi.N == sum(lengths) and torch.equal(out[:pi.N].cpu(), R.pack_tokens(caps, lengths, col0)) and int(out[pi.N]) == -1
    assert sum([12] * 10 + [10] * 10 + [6] * 10 + [2] * 10) == 300


@pytest.mark.parametrize("lens", [[7, 300, 1, 7, 300, 2], [5]], ids=["B6_Tmax300", "B1"])
def test_collate_captions_edges(lens):
    lib = L.load()
    g = torch.Generator().manual_seed(73)
    B, Tmax = len(lens), max(lens)
    flat = torch.randint(1, 1000, (sum(lens),), generator=g)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)
    order = sorted(range(B), key=lambda i: -lens[i])                  # longest first, ties in dataset order
    out = torch.full((B + 1, Tmax), -1, dtype=torch.int64, device="cuda")
    fd, od, rd = flat.cuda(), offsets.cuda(), torch.tensor(order, dtype=torch.int32).cuda()
    L.check(lib.sat_collate_captions(fd.data_ptr(), od.data_ptr(), rd.data_ptr(), B, Tmax, out.data_ptr(), st()))
    sync()
    assert torch.equal(out[:B].cpu(), R.collate(flat, offsets, order, Tmax)) and bool((out[B] == -1).all())


@pytest.mark.parametrize("cols", [75, 76, 1028 * 64])
def test_gather_rows_scalar_vector_and_multi_chunk(cols):
    lib = L.load()
    g = torch.Generator().manual_seed(74)
    src = torch.randn(5, cols, generator=g)
    order = [3, 0, 3, 1, 4]                                           # not the identity; source row 3 twice
    out = nans(len(order) + 1, cols)
    sd, rd = src.cuda(), torch.tensor(order, dtype=torch.int32).cuda()
    L.check(lib.sat_gather_rows_f32(sd.data_ptr(), rd.data_ptr(), len(order), cols, out.data_ptr(), st()))
    sync()
    assert same_bits(out[:len(order)], src[order]) and all_nan(out[len(order):])


def test_rows_copy_identity_strided_and_zero_rows():
    lib = L.load()
    g = torch.Generator().manual_seed(75)
    src = torch.randn(6, 310, generator=g)
    out = nans(7, 304)
    sd = src.cuda()
    L.check(lib.sat_rows_copy(sd.data_ptr(), 310, None, 0, 6, 6, 300, out.data_ptr(), 304, st()))
    sync()
    assert same_bits(out[:6, :300], src[:, :300]) and all_nan(out[:6, 300:]) and all_nan(out[6:])
    out2 = nans(7, 304)
    L.check(lib.sat_rows_copy(sd.data_ptr(), 310, None, 0, 6, 0, 300, out2.data_ptr(), 304, st()))      # rows = 0
    sync()
    assert all_nan(out2)


@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("C", [4, 12])
def test_pad_nhwc_with_signed_zero_mask(pad, C):
    lib = L.load()
    g = torch.Generator().manual_seed(76 + C)
    N, H, W = 2, 3, 5
    x, y = torch.randn(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g)
    y.view(-1)[::7], y.view(-1)[3::7] = 0.0, -0.0                      # exact zeros of both signs: masked like negatives
    assert (y == 0).sum() > 10 and torch.signbit(y[y == 0]).any() and not torch.signbit(y[y == 0]).all()
    xd, yd = x.cuda(), y.cuda()
    for mask in (yd, None):
        out = nans(N * (H + 2 * pad) * (W + 2 * pad) * C + 4)
        L.check(lib.sat_pad_nhwc_f32(xd.data_ptr(), L.ptr(mask), N, H, W, C, pad, out.data_ptr(), st()))
        sync()
        want = R.pad_nhwc(x, None if mask is None else y, pad)
        assert same_bits(out[:-4].view(want.shape), want) and all_nan(out[-4:])


@pytest.mark.parametrize("C", [1, 5])
def test_maxpool2_bwd_sends_the_gradient_to_the_first_maximum(C):
    lib = L.load()
    g = torch.Generator().manual_seed(77 + C)
    for x in (torch.randint(0, 3, (2, 6, 8, C), generator=g).float(), torch.full((1, 4, 4, C), 1.5)):      # most windows tie; all equal
        N, Hin, Win, _ = x.shape
        dy = torch.randn(N, Hin // 2, Win // 2, C, generator=g)
        dx = nans(x.numel() + 4)
        xd, dyd = x.cuda(), dy.cuda()
        L.check(lib.sat_maxpool2_bwd_f32(xd.data_ptr(), dyd.data_ptr(), N, Hin, Win, C, dx.data_ptr(), st()))
        sync()
        assert same_bits(dx[:-4].view(x.shape), R.maxpool2_bwd_first_max(x.numpy(), dy.numpy())) and all_nan(dx[-4:])


def test_bcast_add_accumulates_into_a_random_buffer():
    """values on a 2^-8 grid and scale 3/8: every product and sum is exact in f32, so the result is the same bits whether or not
    the compiler contracts the multiply-add"""
    lib = L.load()
    g = torch.Generator().manual_seed(78)
    B, P, C = 3, 7, 5
    out = torch.randint(-2048, 2048, (B, P, C), generator=g).float() / 256
    v = torch.randint(-2048, 2048, (B, C), generator=g).float() / 256
    od = nans(B * P * C + 4)
    od[:B * P * C] = out.cuda().view(-1)
    vd = v.cuda()
    L.check(lib.sat_bcast_add_f32(vd.data_ptr(), B, P, C, 0.375, od.data_ptr(), st()))
    sync()
    want = R.bcast_add(out, v, 0.375)
    assert torch.equal(want.double(), out.double() + 0.375 * v.double()[:, None, :])     # exact in f32
    assert same_bits(od[:-4].view(B, P, C), want) and all_nan(od[-4:])
