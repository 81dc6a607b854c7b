"""CPU: the host side of label smoothing -- tests/label_smoothing_reference.py against torch's own
F.cross_entropy(..., label_smoothing=) with autograd in float64, the float32 restatement's error at every case of the GPU sweep
(tests/test_gpu_label_smoothing.py reads its second tolerance from the frozen table; run with -s to print it), the two new symbols in
the header, the built library and the ctypes table, the argument errors the library returns before it touches a device, the Python
refusals, and the defaults."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_reference as R
import label_smoothing_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

ARG = 1001
NEW = ("sat_ce_rows_ls", "sat_vocab_ce_fwd_bf16_ls")


def near(a, b, atol=1e-12):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=0, atol=atol)


@pytest.mark.parametrize("eps", LR.LS_EPS + (0.0,))
@pytest.mark.parametrize("V", [1, 5, 255, 1003, 12289])
def test_reference_equals_torch_cross_entropy_and_autograd_in_float64(V, eps):
    logits, targets, kinds = R.ce_inputs(V)
    assert set(kinds) == set(R.CE_KINDS)
    r = LR.ls_rows(logits.double(), targets, eps, R.CE_INV)
    e, s = R.f32v(eps), R.f32v(R.CE_INV)
    t = targets.clamp(0, V - 1)                               # -1 and V: the kernel clamps for memory safety
    lg = logits.double().requires_grad_(True)
    rows = F.cross_entropy(lg, t, reduction="none", label_smoothing=e)
    (rows.sum() * s).backward()
    near(r["row_loss"], rows)
    near(r["grad"], lg.grad)
    near(r["loss"], rows.sum() * s)
    near(r["loss"] / (s * logits.shape[0]), F.cross_entropy(logits.double(), t, reduction="mean", label_smoothing=e))
    plain = F.cross_entropy(logits.double(), t, reduction="none")
    near(r["row_nll"], plain)
    near(r["nll"], plain.sum() * s)
    assert all(torch.isfinite(v).all() for v in r.values())
    if eps == 0:
        near(r["row_loss"], r["row_nll"], atol=0)


def test_gradient_of_the_mean_equals_autograd():
    logits, targets = R.ce_loss_inputs(255)
    lg = logits.double().requires_grad_(True)
    F.cross_entropy(lg, targets, label_smoothing=R.f32v(0.1)).backward()
    near(LR.ls_rows(logits.double(), targets, 0.1, 1.0)["grad"] / 255, lg.grad)


def test_f32_restatement_error_at_every_case_of_the_sweep():
    """The figures of label_smoothing_reference.F32_ERR, re-measured and compared with the frozen table as
    test_elementwise_reference_host.py does: the same figure on the host that measured it, within 16 x elsewhere."""
    got = LR.measure_all()
    assert set(got) == set(LR.F32_ERR), set(got) ^ set(LR.F32_ERR)
    assert {k[1] for k in got if k[0] == "ls"} == set(R.CE_V) and {k[2] for k in got if k[0] == "ls"} == set(LR.LS_EPS)
    for key, errs in got.items():
        frozen = LR.F32_ERR[key]
        print("%-28s " % (key,) + "  ".join("%s %.3g" % (k, v) for k, v in zip(LR.LS_OUTPUTS, errs)))
        assert len(errs) == len(frozen) == len(LR.LS_OUTPUTS)
        for k, v, f in zip(LR.LS_OUTPUTS, errs, frozen):
            assert np.isfinite(v), (key, k, v)
            assert (v == 0) == (f == 0) and f / 16 <= v <= f * 16, (key, k, v, f)


def test_new_symbols_are_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]
    assert lib.sat_version() == L.ABI_VERSION == 18
    assert len(L.SIGNATURES["sat_ce_rows_ls"][1]) == 14
    assert len(L.SIGNATURES["sat_vocab_ce_fwd_bf16_ls"][1]) == len(L.SIGNATURES["sat_vocab_ce_fwd_bf16"][1]) + 3


def test_argument_errors_come_back_before_any_launch():
    """no GPU here: every call below must return SAT_ERR_ARG without launching (fake non-null addresses are never dereferenced)"""
    lib = L.load()
    P = 4096                                                    # a non-null address

    def ce(logits=P, ldl=8, targets=P, N=2, V=8, smoothing=0.1, grad=P, ldg=8, row_loss=P, row_nll=P, loss=P, nll=P):
        return lib.sat_ce_rows_ls(logits, ldl, targets, N, V, 0.5, smoothing, grad, ldg, row_loss, row_nll, loss, nll, None)

    for kw in (dict(logits=None), dict(targets=None), dict(row_loss=None), dict(smoothing=-0.1), dict(smoothing=1.0),
               dict(smoothing=1.5), dict(smoothing=float("nan")), dict(ldg=7), dict(N=0), dict(V=0), dict(ldl=7),
               dict(row_nll=None)):
        assert ce(**kw) == ARG, kw

    def vocab(smoothing=0.1, row_nll=P, nll=P, hs=P):
        return lib.sat_vocab_ce_fwd_bf16_ls(hs, P, P, P, 8, 64, 64, 0.5, smoothing, P, 64, P, row_nll, P, nll, P, 1 << 30, None)

    for kw in (dict(smoothing=-0.1), dict(smoothing=1.0), dict(smoothing=float("nan")), dict(row_nll=None), dict(hs=None)):
        assert vocab(**kw) == ARG, kw


def test_python_refusals():
    x, t = torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64)
    for bad in (-0.1, 1.0, 2, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            sat.CrossEntropy(bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            sat.cross_entropy(x, t, bad)
    for logits in (x.double(), x.bfloat16(), x.t(), x[0], torch.zeros(4, 20)[:, ::2]):
        with pytest.raises(TypeError, match="outputs"):
            sat.cross_entropy(logits, t, 0.1)
    for targets in (t.int(), t[:3], t.view(2, 2)):
        with pytest.raises(TypeError, match="targets"):
            sat.cross_entropy(x, targets, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sat.cross_entropy(x, t, 0.1)


def test_defaults_are_zero_and_the_attribute_is_checked():
    assert sat.CrossEntropy().label_smoothing == 0.0
    assert inspect.signature(sat.cross_entropy).parameters["label_smoothing"].default == 0.0
    p = list(inspect.signature(sat.TrainStep.__init__).parameters.values())
    assert p[-1].name == "label_smoothing" and p[-1].default == 0.0
    assert isinstance(sat.TrainStep.label_smoothing, property)
    ts = object.__new__(sat.TrainStep)                          # the setter alone: no model, no device
    ts.label_smoothing = 0.25
    assert ts.label_smoothing == 0.25
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            ts.label_smoothing = bad
    assert ts.label_smoothing == 0.25
    D = importlib.import_module("show-and-tell_amd.decoder")
    ce = D.VocabCE(1, 2, 3, 4, 5)
    assert ce.smoothing == 0.0 and ce.row_nll is None and ce.nll_out is None
