"""Host side of the global-norm clipping and AdamW weight decay (csrc/sat_optim.hip, optim.py, trainer.py); no GPU.

The yardstick first: optim_reference.adamw_step against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (two param groups) on
the CPU, and its float32-against-float64 error at every case of the GPU sweep against the frozen table.  Then the C ABI (symbols,
argument errors before any launch) and the Python refusals and defaults."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import elementwise_reference as R
import optim_reference as O
from flat_adam_host import bare, host_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

ARG = 1001
NEW = ("sat_grad_sumsq_partials", "sat_grad_sumsq_ws_bytes", "sat_grad_sumsq", "sat_adamw_step")
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------- 1. the yardstick

def torch_three_steps(n, clip, max_norm, wd, ranges, dtype):
    """clip_grad_norm_ + AdamW over the elements of adam_inputs(n), the exempt ranges as a second param group of weight decay 0"""
    d = R.adam_inputs(n)
    hp = {k: R.f32v(v) for k, v in R.ADAM_HP.items()}
    mask = O.exempt_mask(ranges, n)
    idx = [torch.nonzero(~mask)[:, 0], torch.nonzero(mask)[:, 0]]
    ps = [d["p"].to(dtype)[i].clone().requires_grad_(True) for i in idx]
    groups = [dict(params=[ps[0]], weight_decay=R.f32v(wd)), dict(params=[ps[1]], weight_decay=0.0)]
    opt = torch.optim.AdamW(groups, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    for p, i in zip(ps, idx):
        opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=d["m"].to(dtype)[i].clone(), exp_avg_sq=d["v"].to(dtype)[i].clone())
    out = []
    for gr in d["grads"]:
        g = O.clamp(gr.to(dtype), clip)
        for p, i in zip(ps, idx):
            p.grad = g[i].clone()
        nrm = torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm is not None else None
        opt.step()
        full = lambda parts: torch.zeros(n, dtype=dtype).index_put_((torch.cat(idx),), torch.cat(parts))
        out.append(dict(p=full([p.detach() for p in ps]), g=full([p.grad for p in ps]), m=full([opt.state[p]["exp_avg"] for p in ps]),
                        v=full([opt.state[p]["exp_avg_sq"] for p in ps]), norm=nrm))
    return out


@pytest.mark.parametrize("dtype", [R.F32, R.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode,wd,ex", [("half", 0.01, "interior"), ("twice", 0.01, "many"), ("inf", 0.0, "none"), ("off", 0.01, "last"),
                                        ("half", 0.0, "first"), ("half", 0.01, "none")])
@pytest.mark.parametrize("clip", O.ADAMW_CLIP)
def test_reference_equals_torch_clip_grad_norm_and_adamw(clip, mode, wd, ex, dtype):
    """Three steps at n = 1023.  In float64 the two differ by what the launcher's float32 hyper-parameters cost (step size and
    sqrt(bc2): 2^-24 relative each, of the update; the decay factor 1 - lr wd: 2^-24 relative of itself, i.e. of p, per step; torch
    keeps all three in double).  In float32 every operation of a step rounds once more or less in another place: at most 8 roundings of the update
    (clip coefficient, step size, sqrt(bc2), m, v, sqrt, quotient, product) and 3 of p (decay, sum, the other side's sum).  With a
    norm, torch's other summation order moves the clip coefficient, and with it gradient, moments and update, by up to n roundings."""
    n = 1023
    mx, ranges = O.max_norm_of(mode, n, clip), O.exempt_ranges(ex, n)
    ref = O.adamw_case(n, clip, mode, wd, ex, dtype)
    tor = torch_three_steps(n, clip, mx, wd, ranges, dtype)
    eps = 2.0 ** -53 if dtype == R.F64 else 2.0 ** -24
    d = R.adam_inputs(n)
    moved, before = torch.zeros(n, dtype=torch.float64), d["p"].double()
    assert mode != "half" or not ref[0]["coef_is_one"], "half the first norm must scale the first step"
    assert mode != "twice" or ref[0]["coef_is_one"]
    for step, (r, t) in enumerate(zip(ref, tor), 1):
        tag = "step %d" % step
        if mx is not None:
            np.testing.assert_allclose(float(r["norm"]), float(t["norm"]), rtol=(n + 2) * eps, err_msg=tag)
        # the scaled gradient: torch sums the squares in another order (n eps relative of the norm at worst), then the quotient, the
        # clamp's operand and the product round
        ge = ((n + 6) if mx is not None else 0) * eps
        assert ((r["g"].double() - t["g"].double()).abs() <= ge * t["g"].double().abs()).all(), tag
        # the moments: per step a few roundings of their own (torch's lerp form rounds otherwise) and what the gradient's error brings
        ga, ma, va = t["g"].double().abs(), t["m"].double().abs(), t["v"].double().abs()
        assert ((r["m"].double() - t["m"].double()).abs() <= step * (8 * eps * (ma + ga) + ge * ga) + 1e-17).all(), tag
        assert ((r["v"].double() - t["v"].double()).abs() <= step * (8 * eps * (va + ga * ga) + 2 * ge * ga * ga) + 1e-17).all(), tag
        moved = moved + (t["p"].double() - before).abs()
        before = t["p"].double()
        hyper = 2.0 ** -22 * moved + (step * 2.0 ** -24 * before.abs() if wd > 0 else 0.0)       # f32 step size, sqrt(bc2); f32 decay factor
        rounding = ge * moved + (0.0 if dtype == R.F64 else 8 * eps * moved + 3 * step * eps * before.abs())
        err = (r["p"].double() - t["p"].double()).abs()
        print("%s  p err %.3g" % (tag, err.max().item()))
        assert (err <= hyper + rounding + 1e-15).all(), (tag, err.max().item())
    # the decay reached the elements outside the ranges only
    if wd > 0 and ranges and mode == "off":
        plain = O.adamw_case(n, clip, mode, 0.0, ex, dtype)
        mask = O.exempt_mask(ranges, n)
        assert torch.equal(plain[0]["p"][mask], ref[0]["p"][mask]) and not torch.equal(plain[0]["p"][~mask], ref[0]["p"][~mask])


def test_sumsq_inputs_hold_the_edges_the_gpu_test_names():
    assert [O.sumsq_grid(n) for n in O.SUMSQ_N] == [1, 1, 1, 1, 1, 1, 2, 768, 768]
    w = O.sumsq_inputs("wide", 1023)
    assert torch.isinf(w * w).any() and ((w * w) == 0).any(), "float32 squares overflow and underflow"
    tot, bad = O.sumsq(w.double())
    assert torch.isfinite(tot) and bad == 0
    assert O.sumsq(O.sumsq_inputs("zeros", 5).double())[0] == 0
    assert float(O.coef(O.norm(torch.zeros((), dtype=R.F64)), 0.5)) == 1.0
    g = O.sumsq_inputs("nan_last", 1023)
    assert torch.isnan(g[-1]) and O.sumsq(g.double())[1] == 1
    g = O.sumsq_inputs("inf_first", 1023)
    tot, bad = O.sumsq(g.double(), 0.1)
    assert bad == 1 and torch.isfinite(tot), "the clamp hides the Inf from the sum, not from the count"


def test_exempt_ranges_of_every_case_are_a_valid_table():
    for n in O.ADAMW_N:
        for ex in O.ADAMW_EXEMPT:
            r = O.exempt_ranges(ex, n)
            assert len(r) <= O.MAX_EXEMPT and all(lo % 4 == 0 and lo < hi and (hi % 4 == 0 or hi >= n) for lo, hi in r), (n, ex, r)
            assert all(a[1] <= b[0] for a, b in zip(r, r[1:])), (n, ex)
    assert len(O.exempt_ranges("many", 1023)) == 32 and O.exempt_ranges("last", 1023) == [(1016, 1023)]
    assert O.exempt_ranges("interior", 1023)[0][1] % 4 == 0 and O.exempt_ranges("interior", 1023)[0][1] < 1020


def test_f32_restatement_error_at_every_case_of_the_sweep():
    """The figures of optim_reference.F32_ERR, re-measured and compared with the frozen table as
    test_label_smoothing_host.py does: the same figure on the host that measured it, within 16 x elsewhere."""
    got = O.measure_all()
    assert set(got) == set(O.F32_ERR) and len(got) == 480
    for key, errs in got.items():
        frozen = O.F32_ERR[key]
        assert len(errs) == len(frozen) == len(O.ADAMW_OUTPUTS)
        for k, v, f in zip(O.ADAMW_OUTPUTS, errs, frozen):
            assert np.isfinite(v), (key, k, v)
            assert (v == 0) == (f == 0) and f / 16 <= v <= f * 16, (key, k, v, f)
    # without the feature the case is elementwise_reference's
    for n in O.ADAMW_N:
        for clip in O.ADAMW_CLIP:
            assert O.F32_ERR[(n, clip, "off", 0.0, "none")] == R.F32_ERR[("adam", n, clip)]


# ---------------------------------------------------------------------------------------------- 2. symbols

def test_new_symbols_are_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]
    assert lib.sat_version() == L.ABI_VERSION == 18
    assert len(L.SIGNATURES["sat_adamw_step"][1]) == 20 and len(L.SIGNATURES["sat_grad_sumsq"][1]) == 7
    for n in O.SUMSQ_N:
        assert lib.sat_grad_sumsq_partials(n) == O.sumsq_grid(n) and lib.sat_grad_sumsq_ws_bytes(n) == 16 * O.sumsq_grid(n)
    assert lib.sat_grad_sumsq_partials(0) == 0 and lib.sat_grad_sumsq_ws_bytes(0) == 0
    # the build script compiles the new file and links it into both libraries
    sh = open(os.path.join(ROOT, "show-and-tell_amd", "csrc", "build.sh")).read()
    assert len(re.findall(r"build/sat_optim\.o", sh)) == 2 and re.search(r"for f in [^;]*\bsat_optim\b", sh)


# ---------------------------------------------------------------------------------------------- 3. argument errors

def ranges_arg(pairs):
    return (ctypes.c_int64 * (2 * len(pairs)))(*[x for r in pairs for x in r])


def test_argument_errors_come_back_before_any_launch():
    """no GPU here: every call below must return SAT_ERR_ARG without launching (fake non-null addresses are never dereferenced)"""
    lib = L.load()
    P = 4096                                                    # a non-null, 16-byte aligned address

    def sumsq(g=P, n=100, clip=0.1, partials=P, off=0, cap=1):
        return lib.sat_grad_sumsq(g, n, clip, partials, off, cap, None)

    for kw in (dict(g=None), dict(partials=None), dict(g=P + 4), dict(partials=P + 8), dict(n=0), dict(n=-3), dict(clip=NAN),
               dict(off=-1), dict(off=1), dict(cap=0), dict(n=1028, cap=1), dict(n=1 << 40, off=1, cap=768)):
        assert sumsq(**kw) == ARG, kw

    def adamw(p=P, g=P, m=P, v=P, n=100, step=1, wd=0.01, exempt=None, n_exempt=0, max_norm=1.0, partials=P, n_partials=1,
              norm_out=P, skip=P):
        return lib.sat_adamw_step(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.1, step, wd, exempt, n_exempt, max_norm, partials,
                                  n_partials, norm_out, skip, None)

    bad = [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(p=P + 4), dict(g=P + 8), dict(m=P + 4), dict(v=P + 12),
           dict(n=0), dict(n=-1), dict(step=0), dict(wd=-0.01), dict(wd=NAN), dict(max_norm=0.0), dict(max_norm=-1.0),
           dict(max_norm=NAN), dict(n_partials=0), dict(n_partials=-2), dict(partials=P + 8), dict(norm_out=P + 4),
           dict(n_exempt=1), dict(n_exempt=-1),
           dict(exempt=ranges_arg([(4 * k, 4 * k + 4) for k in range(0, 66, 2)]), n_exempt=33),
           dict(exempt=ranges_arg([(8, 12), (0, 4)]), n_exempt=2), dict(exempt=ranges_arg([(0, 8), (4, 12)]), n_exempt=2),
           dict(exempt=ranges_arg([(2, 8)]), n_exempt=1), dict(exempt=ranges_arg([(-4, 8)]), n_exempt=1),
           dict(exempt=ranges_arg([(8, 8)]), n_exempt=1), dict(exempt=ranges_arg([(8, 4)]), n_exempt=1)]
    for kw in bad:
        assert adamw(**kw) == ARG, kw
    # without partials max_norm and n_partials are not looked at -- but everything else still is
    assert adamw(partials=None, max_norm=0.0, n_partials=0, wd=-1.0) == ARG
    assert adamw(partials=None, max_norm=NAN, n_partials=0, step=0) == ARG


# ---------------------------------------------------------------------------------------------- 4. Python refusals

def host_params():
    lin = torch.nn.Linear(5, 3)
    return lin, list(lin.parameters())


def test_fused_clamp_adam_refuses_before_any_device_call():
    lin, ps = host_params()
    for bad in (-0.01, NAN, "0.01", None, INF, True):
        with pytest.raises(ValueError, match="weight_decay"):
            sat.FusedClampAdam(ps, weight_decay=bad)
    for bad in (0, 0.0, -1.0, NAN, "1", True):
        with pytest.raises(ValueError, match="max_norm"):
            sat.FusedClampAdam(ps, max_norm=bad)
    with pytest.raises(ValueError, match="no_decay"):
        sat.FusedClampAdam(ps, weight_decay=0.01, no_decay=[torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(ValueError, match="no_decay"):
        sat.FusedClampAdam(ps, weight_decay=0.01, no_decay=[lin.bias.detach().clone()])          # equal values, another tensor
    # 33 separate 1-D parameters, each between two matrices: 33 ranges after merging
    many = []
    for _ in range(33):
        many += [torch.nn.Parameter(torch.zeros(2, 2)), torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="33 separate ranges"):
        sat.FusedClampAdam(many, weight_decay=0.01, no_decay=[p for p in many if p.dim() == 1])
    # valid keywords on host tensors get as far as the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sat.FusedClampAdam(ps, max_norm=INF, weight_decay=0.01, no_decay=sat.no_decay_params(lin))
    with pytest.raises(TypeError):
        sat.FusedClampAdam(ps, 1e-3, (0.9, 0.999), 1e-8, None, 0.5)                               # keyword-only


def test_no_decay_params_are_the_one_dimensional_ones():
    m = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3), torch.nn.Embedding(7, 3))
    got = sat.no_decay_params(m)
    assert [id(p) for p in got] == [id(m[0].bias), id(m[1].weight), id(m[1].bias)]
    assert sat.no_decay_names(m) == ["0.bias", "1.weight", "1.bias"]
    m[0].bias.requires_grad_(False)
    assert [id(p) for p in sat.no_decay_params(m)] == [id(m[1].weight), id(m[1].bias)]


def test_adjacent_no_decay_slices_merge_into_one_range():
    from importlib import import_module
    optim = import_module("show-and-tell_amd.optim")
    assert optim.merge_ranges([(8, 11), (0, 2), (12, 16), (24, 25)]) == [(0, 2), (8, 16), (24, 25)]
    arr, k = optim.exempt_array([(0, 2), (8, 16), (24, 25)], 12, 24)
    assert k == 1 and list(arr) == [0, 4]
    assert optim.exempt_array([(0, 6)], 8, 24) == (None, 0)


def test_train_step_properties_refuse_and_default():
    ts = bare(sat.TrainStep, {"decoder.linear.bias": (0, 3, (3,))})
    assert ts.max_grad_norm == 0.0 and ts.weight_decay == 0.0 and ts.no_decay is None and ts.last_grad_norm is None
    assert sat.TrainStep.max_grad_norm.fset is not None and sat.TrainStep.weight_decay.fset is not None
    for bad in (-1.0, NAN, "1", None, True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            ts.max_grad_norm = bad
    for bad in (-0.01, NAN, "0.01", None, INF):
        with pytest.raises(ValueError, match="weight_decay"):
            ts.weight_decay = bad
    for bad in ("decoder.linear.bias", 3, [3], [b"x"]):
        with pytest.raises(ValueError, match="no_decay"):
            ts.no_decay = bad
    assert ts.max_grad_norm == 0.0 and ts.weight_decay == 0.0 and ts.no_decay is None, "a refused value changes nothing"
    ts.max_grad_norm, ts.weight_decay, ts.no_decay = INF, 0.01, ["decoder.linear.bias"]
    assert ts.max_grad_norm == INF and ts.weight_decay == 0.01 and ts.no_decay == ("decoder.linear.bias",)
    ts.max_grad_norm, ts.no_decay = 0, None
    assert ts.max_grad_norm == 0.0 and ts.no_decay is None

    ts.flat = host_flat({"a.weight": (0, 6, (2, 3)), "a.bias": (8, 3, (3,)), "b.bias": (12, 2, (2,))})
    with pytest.raises(ValueError, match="nope"):
        ts.no_decay = ["a.bias", "nope"]
    ts.no_decay = ["b.bias", "a.bias"]
    assert ts._exempt == [(8, 14)]


def test_train_step_signature_is_unchanged():
    sig = inspect.signature(sat.TrainStep.__init__)
    assert list(sig.parameters) == ["self", "model", "lr", "grad_clip", "betas", "eps", "label_smoothing"]
    assert [p.default for p in sig.parameters.values()][2:] == [1e-3, 0.1, (0.9, 0.999), 1e-8, 0.0]
    sig = inspect.signature(sat.FusedClampAdam.__init__)
    assert list(sig.parameters) == ["self", "params", "lr", "betas", "eps", "clip", "max_norm", "weight_decay", "no_decay"]
    kinds = [p.kind for p in sig.parameters.values()]
    assert all(k == inspect.Parameter.KEYWORD_ONLY for k in kinds[6:]) and all(k != inspect.Parameter.KEYWORD_ONLY for k in kinds[:6])


def test_optimizer_state_dict_carries_the_new_keys_and_loads_into_torch_adamw():
    """the flat engine's state dict without a device: an object made without __init__ around a real FlatAdam on the host"""
    w, b = torch.nn.Parameter(torch.randn(2, 3)), torch.nn.Parameter(torch.randn(3))
    ts, Flat = object.__new__(sat.TrainStep), host_flat({"w": (0, 6, (2, 3)), "b": (8, 3, (3,))})
    Flat.m.copy_(torch.rand(12))
    Flat.v.copy_(torch.rand(12))
    ts.flat = Flat
    ts.lr, ts.grad_clip, ts.betas, ts.eps, ts.step_count = 1e-3, 0.1, (0.9, 0.999), 1e-8, 3
    sd = ts.optimizer_state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0 and sd["param_groups"][0]["decoupled_weight_decay"] is False
    assert sd["max_grad_norm"] == 0.0
    torch.optim.Adam([w, b]).load_state_dict(sd)
    ts.weight_decay, ts.max_grad_norm = 0.01, 5.0
    sd = ts.optimizer_state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.01 and sd["param_groups"][0]["decoupled_weight_decay"] is True
    assert sd["max_grad_norm"] == 5.0 and sd["grad_clip"] == 0.1
    opt = torch.optim.AdamW([w, b])
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["weight_decay"] == 0.01 and torch.equal(opt.state[b]["exp_avg"], Flat.m[8:11])
    other = bare(sat.TrainStep)
    other.load_optimizer_state_dict(sd)
    assert other.weight_decay == 0.01 and other.max_grad_norm == 5.0 and other.step_count == 3
    old = {k: v for k, v in sd.items() if k != "max_grad_norm"}          # a checkpoint from before the key existed
    other.max_grad_norm = 2.0
    other.load_optimizer_state_dict(old)
    assert other.max_grad_norm == 2.0
    coupled = dict(sd, param_groups=[dict(sd["param_groups"][0], decoupled_weight_decay=False)])
    with pytest.raises(ValueError, match="coupled"):
        other.load_optimizer_state_dict(coupled)
