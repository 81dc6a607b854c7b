"""Host side of the averaged weights (csrc/sat_optim.hip: sat_ema_update, sat_swap_f32; optim.py, trainer.py); no GPU.

The yardstick first (ema_reference against torch.optim.swa_utils in float64, and its float32 form against its float64 form), then
the C ABI (symbols, argument errors before any launch), the attribute checks, the decay schedule and the state dicts with the
feature off."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ema_reference as E
from flat_adam_host import bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

ARG = 1001
NEW = ("sat_ema_update", "sat_swap_f32")
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------- 1. the yardstick

@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999, 0.9999])
def test_reference_rule_equals_torch_swa_utils_in_float64(decay):
    g = torch.Generator().manual_seed(3)
    e = [torch.randn(7, 5, generator=g, dtype=torch.float64), torch.randn(11, generator=g, dtype=torch.float64)]
    ours = [t.numpy().copy() for t in e]
    fn = torch.optim.swa_utils.get_ema_multi_avg_fn(decay)
    for step in range(5):
        p = [t + 0.1 * torch.randn(t.shape, generator=g, dtype=torch.float64) for t in e]
        fn(e, p, step)
        ours = [E.ema_step_f64(o, q.numpy(), decay) for o, q in zip(ours, p)]
        for o, t in zip(ours, e):
            np.testing.assert_allclose(o, t.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("decay", E.SWEEP_DECAY)
def test_float32_form_is_the_float64_rule_rounded(decay):
    """three roundings apart at most: the weight (2^-24 of the step), the difference (2^-24 of it), the result (2^-24 of it)"""
    e, p = E.sweep_inputs(1023, decay)
    r, o = E.ema_step(e, p, decay)
    ref = E.ema_step_f64(e.astype(np.float64), p.astype(np.float64), float(np.float32(decay)))
    step = np.abs(p.astype(np.float64) - e.astype(np.float64))
    assert (np.abs(r - ref) <= 2.0 ** -24 * np.abs(ref) + 2.0 ** -22 * step).all()
    assert E.matches(r, r, o).all() and (E.matches(o, r, o)).all()
    # where the two differ they are neighbours
    assert (np.abs(o.astype(np.float64) - r) <= 2.0 ** -22 * np.abs(r)).all()


def test_midpoint_slack_opens_only_at_a_midpoint():
    """e = 1, w = 0.5: d = 2^-23 gives the float64 value 1 + 2^-24, the midpoint of 1 and 1 + 2^-23.  A float64 sum that lands there
    may have been rounded onto it from either side, so both neighbours pass; the expected one is the tie to even"""
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    r, o = E.ema_step([one], [up], 0.5)
    assert r[0] == one and o[0] == up
    assert E.matches([one], r, o).all() and E.matches([up], r, o).all() and not E.matches([np.nextafter(up, np.float32(2))], r, o).any()
    r, o = E.ema_step([one], [np.float32(1.5)], 0.5)
    assert r[0] == np.float32(1.25) and o[0] == r[0]
    assert E.weight(0.9) == np.float32(1.0 - float(np.float32(0.9))) and E.weight(0.5) == np.float32(0.5)


# ---------------------------------------------------------------------------------------------- 2. symbols

def test_new_symbols_are_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]
    assert lib.sat_version() == L.ABI_VERSION == 18
    assert re.search(r"#define SAT_ABI_VERSION 18\b", header)
    assert len(L.SIGNATURES["sat_ema_update"][1]) == 7 and len(L.SIGNATURES["sat_swap_f32"][1]) == 4


# ---------------------------------------------------------------------------------------------- 3. argument errors

def test_argument_errors_come_back_before_any_launch():
    """no GPU here: every call below must return SAT_ERR_ARG without launching (fake non-null addresses are never dereferenced)"""
    lib = L.load()
    P, Q = 4096, 1 << 20                                        # non-null, 16-byte aligned, far apart

    def ema(e=P, p=Q, n=100, decay=0.999, skip=P, norm=Q):
        return lib.sat_ema_update(e, p, n, decay, skip, norm, None)

    for kw in (dict(e=None), dict(p=None), dict(n=0), dict(n=-5), dict(e=P + 4), dict(e=P + 8), dict(p=Q + 4), dict(p=Q + 12),
               dict(norm=Q + 4), dict(norm=Q + 12), dict(decay=NAN), dict(decay=0.0), dict(decay=1.0), dict(decay=-0.5),
               dict(decay=1.5), dict(decay=INF), dict(decay=-INF)):
        assert ema(**kw) == ARG, kw
    assert ema(skip=None, norm=None, decay=NAN) == ARG and ema(skip=None, norm=None, n=0) == ARG

    def swap(a=P, b=Q, n=100):
        return lib.sat_swap_f32(a, b, n, None)

    for kw in (dict(a=None), dict(b=None), dict(n=0), dict(n=-1), dict(a=P + 4), dict(b=Q + 8), dict(b=P), dict(b=P + 16 * 24),
               dict(a=P + 16 * 24, b=P), dict(b=P + 400 - 16, n=100), dict(a=Q, b=Q - 4 * 1028 + 16, n=1028)):
        assert swap(**kw) == ARG, kw


# ---------------------------------------------------------------------------------------------- 4. the schedule

def test_ema_decay_at():
    for t in (1, 9, 10, 10 ** 6):
        assert sat.ema_decay_at(0.999, t, False) == 0.999 and E.ema_decay_at(0.999, t, False) == 0.999
        assert sat.ema_decay_at(0.999, t, True) == E.ema_decay_at(0.999, t, True) == min(0.999, (1 + t) / (10 + t))
    assert sat.ema_decay_at(0.999, 1, True) == 2 / 11 and sat.ema_decay_at(0.999, 9, True) == 10 / 19
    assert sat.ema_decay_at(0.999, 10, True) == 11 / 20 and sat.ema_decay_at(0.999, 10 ** 6, True) == 0.999
    assert sat.ema_decay_at(0.5, 9, True) == 0.5 and sat.ema_decay_at(0.5, 1, True) == 2 / 11
    assert isinstance(sat.ema_decay_at(0.9, 3, True), float)
    assert list(inspect.signature(sat.ema_decay_at).parameters) == ["decay", "t", "warmup"]


# ---------------------------------------------------------------------------------------------- 5. attributes

@pytest.mark.parametrize("cls", [sat.TrainStep, sat.FusedClampAdam], ids=["TrainStep", "FusedClampAdam"])
def test_attributes_refuse_and_default(cls):
    obj = bare(cls)
    assert obj.ema_decay == 0.0 and obj.ema_warmup is False
    for bad in (True, False, NAN, 1.0, 1, -0.1, 1.5, INF, -INF, "0.9", None, [0.9]):
        with pytest.raises(ValueError, match="ema_decay"):
            obj.ema_decay = bad
    for bad in (0, 1, "yes", None, 0.0):
        with pytest.raises(ValueError, match="ema_warmup"):
            obj.ema_warmup = bad
    assert obj.ema_decay == 0.0 and obj.ema_warmup is False, "a refused value changes nothing"
    obj.ema_decay, obj.ema_warmup = 0.999, True             # (copies the host buffer)
    assert obj.ema_decay == 0.999 and obj.ema_warmup is True
    obj.ema_decay = 0
    assert obj.ema_decay == 0.0 and isinstance(obj.ema_decay, float)


def test_without_an_average_the_entry_points_raise():
    ts = host_engine()
    ts._params_list = []
    for call in (ts.reset_ema, ts.averaged_state_dict, lambda: ts.averaged_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay has never been set"):
            call()
    opt = bare(sat.FusedClampAdam)
    for call in (opt.reset_ema, opt.ema_params):
        with pytest.raises(RuntimeError, match="ema_decay has never been set"):
            call()


def test_constructor_signatures_are_unchanged():
    """the two settings are attributes on both classes: the constructors keep the parameter lists other tests pin"""
    assert "ema_decay" not in inspect.signature(sat.TrainStep.__init__).parameters
    assert "ema_decay" not in inspect.signature(sat.FusedClampAdam.__init__).parameters
    assert isinstance(sat.TrainStep.ema_decay, property) and isinstance(sat.FusedClampAdam.ema_decay, property)


# ---------------------------------------------------------------------------------------------- 6. state dicts, feature off

def host_engine():
    """the flat engine without a device, as test_optim_host.py builds it: parameters w [2, 3] at 0 and b [3] at 8 of 12 floats"""
    ts = bare(sat.TrainStep)
    for t in (ts.flat.m, ts.flat.v, ts.flat.params):
        t.copy_(torch.rand(12))
    ts.lr, ts.grad_clip, ts.betas, ts.eps, ts.step_count = 1e-3, 0.1, (0.9, 0.999), 1e-8, 3
    return ts


def test_state_dicts_have_no_ema_entry_with_the_feature_off():
    ts = host_engine()
    sd = ts.optimizer_state_dict()
    assert set(sd) == {"state", "param_groups", "param_names", "grad_clip", "max_grad_norm"}
    other = host_engine()
    other.ema_warmup = True
    other.load_optimizer_state_dict(sd)                        # no entry: the averaging state stays what it is
    assert other.ema_decay == 0.0 and other.ema_warmup is True and getattr(other.flat, "ema", None) is None
    assert "ema" not in other.optimizer_state_dict()


def test_state_dict_carries_the_average_once_it_exists():
    """host tensors stand in for the flat buffers: nothing is launched by the state dict calls"""
    ts = host_engine()
    ts.ema_decay = 0.99                                        # copies flat.params
    assert torch.equal(ts.flat.ema, ts.flat.params) and ts.flat.ema is not ts.flat.params
    ts.flat.ema.mul_(0.5)
    ts.ema_warmup = True
    ts.ema_decay = 0.0                                         # off again: the buffer stays, and so does the entry
    sd = ts.optimizer_state_dict()
    assert sd["param_names"] == ["w", "b"] and sd["ema"]["decay"] == 0.0 and sd["ema"]["warmup"] is True
    assert [tuple(t.shape) for t in sd["ema"]["params"]] == [(2, 3), (3,)]
    assert torch.equal(sd["ema"]["params"][1], ts.flat.ema[8:11])
    ts.ema_decay = 0.99
    sd = ts.optimizer_state_dict()
    other = host_engine()
    other.load_optimizer_state_dict(sd)
    assert other.ema_decay == 0.99 and other.ema_warmup is True
    assert torch.equal(other.flat.ema[:6], ts.flat.ema[:6]) and torch.equal(other.flat.ema[8:11], ts.flat.ema[8:11])
    bad = dict(sd, ema=dict(sd["ema"], params=[sd["ema"]["params"][0], torch.zeros(4)]))
    with pytest.raises(ValueError, match="shape"):
        host_engine().load_optimizer_state_dict(bad)
    with pytest.raises(ValueError, match="ema_decay"):
        host_engine().load_optimizer_state_dict(dict(sd, ema=dict(sd["ema"], decay=1.0)))
