"""CPU: the host side of unlikelihood training -- tests/unlikelihood_reference.py validated (closed form against torch autograd of
the fairseq formulation in float64, alpha = 0 against label_smoothing_reference, set semantics, the excluded target, plain step-0
rows), the float32 restatement's error at every case of the GPU sweep (tests/test_gpu_unlikelihood.py reads its tolerance from the
frozen table; run with -s to print it), the conditions the GPU test relies on asserted on the float64 reference of its own inputs,
the two new symbols, the argument errors the library returns before it touches a device, and the Python refusals."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import elementwise_reference as R
import label_smoothing_reference as LR
import unlikelihood_reference as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

ARG, UNSUPPORTED = 1001, 1003
NEW = ("sat_ce_rows_ul", "sat_vocab_ce_fwd_bf16_ul")


def near(a, b, atol=1e-12):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=0, atol=atol)


# ---------------------------------------------------------------------------------------------- 1. the reference

@pytest.mark.parametrize("key", [("ul", 5, 1.0, 0.0), ("ul", 255, 0.5, 0.1), ("ul", 1003, 1.0, 0.0), ("ul_pack", "full", 255),
                                 ("ul_pack", "two", 5), ("ul_clamp", 1003)])
def test_closed_form_equals_autograd_of_the_fairseq_formulation_in_float64(key):
    lg, tg, ln, eps, alpha = UR.all_cases()[key]
    auto = UR.ul_autograd(lg.double(), tg, ln, eps, alpha, R.CE_INV)
    closed = UR.ul_rows(lg.double(), tg, ln, eps, alpha, R.CE_INV)
    for k in UR.UL_OUTPUTS:
        near(closed[k], auto[k], atol=1e-12 * max(1.0, float(auto[k].abs().max())))
    assert all(torch.isfinite(auto[k]).all() for k in UR.UL_OUTPUTS)
    assert float(auto["row_ul"].max()) > 0


def test_the_issues_pack_gives_the_gradient_of_the_mean():
    """lengths [12,12,11,9,9,7,4,3], mean over the rows: the closed-form gradient against autograd, to 1e-14"""
    lg, tg, ln = UR.ul_inputs(1003)
    N = lg.shape[0]
    auto = UR.ul_autograd(lg.double(), tg, ln, 0.1, 1.0, 1.0 / N)
    closed = UR.ul_rows(lg.double(), tg, ln, 0.1, 1.0, 1.0 / N)
    assert float((auto["grad"] - closed["grad"]).abs().max()) < 1e-14


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_alpha_zero_is_the_label_smoothing_reference(eps):
    lg, tg, ln = UR.ul_inputs(255)
    want = LR.ls_rows(lg.double(), tg, eps, R.CE_INV)
    for got in (UR.ul_rows(lg.double(), tg, ln, eps, 0.0, R.CE_INV), UR.ul_autograd(lg.double(), tg, ln, eps, 0.0, R.CE_INV)):
        for k in LR.LS_OUTPUTS:
            near(got[k], want[k])


def test_set_semantics_excluded_target_and_plain_step_zero_rows():
    V, lengths = 11, [5, 2]
    # sequence 0: 3 3 3 4 3 -- sequence 1: 6 6
    targets = torch.tensor([3, 6, 3, 6, 3, 4, 3], dtype=torch.int64)
    assert UR.positions(lengths) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (3, 0), (4, 0)]
    sets = UR.candidate_sets(targets, lengths, V)
    assert sets == [[], [], [], [], [], [3], [4]]        # 3 three times in the prefix counts once; the own target is no candidate
    lg = torch.randn(7, V, generator=R.gen(3)).double()
    r = UR.ul_rows(lg, targets, lengths, 0.0, 1.0, 1.0)
    p = torch.softmax(lg, 1)
    near(r["row_ul"][5], -torch.log(1 - p[5, 3]))
    near(r["row_ul"][6], -torch.log(1 - p[6, 4]))
    assert float(r["row_ul"][:5].abs().max()) == 0
    assert r["mask"].sum(1).tolist() == [0, 0, 0, 0, 0, 1, 1]
    plain = LR.ls_rows(lg, targets, 0.0, 1.0)
    near(r["grad"][:5], plain["grad"][:5], atol=0)       # step-0 rows and rows without candidates are plain rows
    near(r["row_loss"][:5], plain["row_loss"][:5], atol=0)
    # clamped ids collide with real ones: -1 is column 0, V is column V - 1
    t2 = torch.tensor([-1, 0, V, V - 1, 5], dtype=torch.int64)
    assert UR.candidate_sets(t2, [5], V) == [[], [], [0], [0], [0, V - 1]]


def test_every_sweep_case_has_its_candidates_where_the_gpu_test_says():
    for V in UR.UL_V:
        lg, tg, ln = UR.ul_inputs(V)
        sets = UR.candidate_sets(tg, ln, V)
        cols = {c for s in sets for c in s}
        assert {0, V - 1} <= cols, V
        if V % 4 and V > 4:
            assert 4 * (V // 4) in cols, V                      # the scalar tail
        if V > 4:
            assert {3, 4} <= cols, V                            # both sides of a 16-byte chunk boundary
        if V > 4100:
            assert {4, 2052, 4100} <= cols, V                   # three ids 2048 apart
        assert (-1 in tg.tolist()) and (V in tg.tolist())
        assert max(len(s) for s in sets) >= min(3, V - 1)
    lg, tg, ln = UR.ul_pack_inputs("full", 255)
    sets = UR.candidate_sets(tg, ln, 255)
    pre = UR.prefix(ln)
    assert len(sets[pre[63]]) == 63 and sets[pre[63] + 1] == [7] and sets[pre[62] + 1] == [] and sets[pre[2] + 2] == [5]


# ---------------------------------------------------------------------------------------------- 2. the frozen f32 error

def test_f32_restatement_error_at_every_case_of_the_sweep():
    """re-measured and compared with the frozen table as test_label_smoothing_host.py does: within 16 x of the frozen figure"""
    got = UR.measure_all()
    assert set(got) == set(UR.F32_ERR), set(got) ^ set(UR.F32_ERR)
    for key, errs in got.items():
        frozen = UR.F32_ERR[key]
        print("    %r: (%s)," % (key, ", ".join("%.3g" % v for v in errs)))
        assert len(errs) == len(frozen) == len(UR.UL_OUTPUTS)
        for k, v, f in zip(UR.UL_OUTPUTS, errs, frozen):
            assert np.isfinite(v), (key, k, v)
            assert (v == 0) == (f == 0) and f / 16 <= v <= f * 16, (key, k, v, f)


# ---------------------------------------------------------------------------------------------- 3. conditions on the GPU test's inputs

def test_conditions_the_gpu_test_relies_on_hold_on_the_float64_reference():
    for key, (lg, tg, ln, eps, alpha) in UR.all_cases().items():
        r = UR.ul_rows(lg.double(), tg, ln, eps, alpha, R.CE_INV)
        q = r["q"][r["mask"] > 0]
        # (a) no candidate in the clamp band: f32 and f64 land on the same side of the clamp
        assert not bool(((q > 5e-6) & (q < 2e-5)).any()), key
        if key[0] != "ul_clamp":
            # (b) amplification: the sweeps stay sensitive
            wmax = float(r["w"].max())
            print("%-32s max w_c %.3g   max W %.3g" % (key, wmax, float(r["w"].sum(1).max())))
            assert wmax <= 10, (key, wmax)
            assert bool((q > 2e-5).all()), key
    for V in UR.UL_CLAMP_V:
        lg, tg, ln = UR.ul_clamp_inputs(V)
        r = UR.ul_rows(lg.double(), tg, ln, 0.0, 1.0, R.CE_INV)
        t = tg.clamp(0, V - 1)
        clamped = 0
        for n, (step, b) in enumerate(UR.positions(ln)):
            c = int(t[b])
            if step and c != int(t[n]):
                # (c) firmly clamped: the term is exactly -log(1e-5) in f32, the weight 0
                assert r["mask"][n, c] == 1 and float(r["q"][n, c]) < 1e-6, (V, n)
                assert float(r["w"][n, c]) == 0
                q32 = 1 - torch.exp(lg[n, c] - torch.logsumexp(lg[n], 0))
                assert float(q32) < 1e-6
                clamped += 1
        assert clamped == 8
        assert float(r["row_ul"].max()) >= -np.log(1e-5)


# ---------------------------------------------------------------------------------------------- 4. symbols, argument errors, refusals

def test_new_symbols_are_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]
    assert lib.sat_version() == L.ABI_VERSION == 18
    assert len(L.SIGNATURES["sat_ce_rows_ul"][1]) == len(L.SIGNATURES["sat_ce_rows_ls"][1]) + 5
    assert len(L.SIGNATURES["sat_vocab_ce_fwd_bf16_ul"][1]) == len(L.SIGNATURES["sat_vocab_ce_fwd_bf16_ls"][1]) + 5


def test_argument_errors_come_back_before_any_launch():
    """no GPU here: every call below must return its error without launching (fake non-null addresses are never dereferenced)"""
    lib = L.load()
    P = 4096                                                    # a non-null address

    def ce(logits=P, ldl=8, targets=P, prefix=P, T=2, N=2, V=8, smoothing=0.1, alpha=1.0, grad=P, ldg=8, row_loss=P, row_nll=P,
           row_ul=P, loss=P, nll=P, ul=P):
        return lib.sat_ce_rows_ul(logits, ldl, targets, prefix, T, N, V, 0.5, smoothing, alpha, grad, ldg, row_loss, row_nll, row_ul,
                                  loss, nll, ul, None)

    for kw in (dict(logits=None), dict(targets=None), dict(row_loss=None), dict(smoothing=-0.1), dict(smoothing=1.0),
               dict(smoothing=float("nan")), dict(ldg=7), dict(N=0), dict(V=0), dict(ldl=7), dict(row_nll=None),
               dict(prefix=None), dict(T=0), dict(T=-1), dict(alpha=-0.5), dict(alpha=float("nan")), dict(row_ul=None)):
        assert ce(**kw) == ARG, kw
    assert ce(T=65) == UNSUPPORTED
    assert ce(T=65, alpha=-1.0) == ARG

    def vocab(smoothing=0.1, alpha=1.0, prefix=P, T=2, row_nll=P, row_ul=P, nll=P, ul=P, hs=P):
        return lib.sat_vocab_ce_fwd_bf16_ul(hs, P, P, P, prefix, T, 8, 64, 64, 0.5, smoothing, alpha, P, 64, P, row_nll, row_ul, P, nll,
                                            ul, P, 1 << 30, None)

    for kw in (dict(smoothing=1.0), dict(smoothing=float("nan")), dict(row_nll=None), dict(hs=None), dict(prefix=None), dict(T=0),
               dict(alpha=-0.5), dict(alpha=float("nan")), dict(row_ul=None)):
        assert vocab(**kw) == ARG, kw
    assert vocab(T=65) == UNSUPPORTED


def test_python_refusals():
    x, t = torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="unlikelihood"):
            sat.CrossEntropy(unlikelihood=bad)
        with pytest.raises(ValueError, match="unlikelihood"):
            sat.cross_entropy(x, t, unlikelihood=bad, lengths=[2, 2])
    with pytest.raises(ValueError, match="lengths"):
        sat.cross_entropy(x, t, unlikelihood=1.0)                      # no lengths
    with pytest.raises(ValueError, match="lengths"):
        sat.CrossEntropy(unlikelihood=1.0)(x, t)
    with pytest.raises(ValueError, match="sum"):
        sat.cross_entropy(x, t, unlikelihood=1.0, lengths=[2, 1])      # 3 rows, not 4
    x65, t65 = torch.zeros(65, 10), torch.zeros(65, dtype=torch.int64)
    with pytest.raises(ValueError, match="64"):
        sat.cross_entropy(x65, t65, unlikelihood=1.0, lengths=[65])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sat.cross_entropy(x, t, unlikelihood=1.0, lengths=[2, 2])      # everything host-side passed
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sat.cross_entropy(x, t)                                        # without the term no lengths are needed


def test_defaults_are_zero_and_the_attribute_is_checked():
    crit = sat.CrossEntropy()
    assert crit.unlikelihood == 0.0 and crit.last_ul is None and crit.last_row_ul is None
    assert sat.CrossEntropy(0.1, 0.5).unlikelihood == 0.5
    sig = inspect.signature(sat.cross_entropy).parameters
    assert sig["unlikelihood"].default == 0.0 and sig["lengths"].default is None
    assert inspect.signature(sat.CrossEntropy.forward).parameters["lengths"].default is None
    assert "unlikelihood" not in inspect.signature(sat.TrainStep.__init__).parameters      # an attribute, as max_grad_norm is
    assert isinstance(sat.TrainStep.unlikelihood, property)
    ts = object.__new__(sat.TrainStep)                          # the setter alone: no model, no device
    assert ts.unlikelihood == 0.0
    ts.unlikelihood = 0.25
    assert ts.unlikelihood == 0.25
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="unlikelihood"):
            ts.unlikelihood = bad
    assert ts.unlikelihood == 0.25
    D = importlib.import_module("show-and-tell_amd.decoder")
    ce = D.VocabCE(1, 2, 3, 4, 5)
    assert ce.alpha == 0.0 and ce.row_ul is None and ce.ul_out is None and ce.smoothing == 0.0
