"""CPU: self-critical training with S sampled captions per image -- the two new entry points (`sat_scst_weights_group`,
`sat_group_sum_rows`) are declared, exported and bound; their restatement (tests/scst_multi_reference.py) has the properties the
header promises; the argument errors come back before any launch; and every ValueError of the Python layer is raised on the host."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import scst_multi_reference as G
import scst_reference as S1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

END = 2
ARG, UNSUPPORTED = 1001, 1003
NEW = ("sat_scst_weights_group", "sat_group_sum_rows")


def bits64(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


# ---- symbols -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]
    assert lib.sat_version() == L.ABI_VERSION == 18
    assert len(L.SIGNATURES["sat_scst_weights_group"][1]) == 16 and len(L.SIGNATURES["sat_group_sum_rows"][1]) == 8
    block = header[header.index("Self-critical training with S sampled"):header.index("int sat_scst_weights_group")]
    assert "added within ABI 18" in " ".join(block.replace("*", " ").split())


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_two_samples_have_opposite_advantages():
    rng = np.random.Generator(np.random.PCG64(1))
    B, T = 9, 4
    ids = G.group_ids(B, 2, T, END, 3)
    rw = rng.random(2 * B) * 3 - 1
    _, _, _, adv, base = G.weights_group(ids, rw, None, 1, END)
    adv = adv.reshape(B, 2)
    assert np.array_equal(bits64(adv[:, 0]), bits64(-adv[:, 1])) and np.abs(adv).max() > 0
    assert np.array_equal(base.reshape(B, 2), rw.reshape(B, 2)[:, ::-1])          # the other sample's reward is the baseline


@pytest.mark.parametrize("S", [2, 3, 4, 7])
def test_equal_rewards_give_exact_zeros(S):
    vals = [0.1, -0.3, 1.0 / 3.0, 2.7]
    B, T = len(vals), 3
    rw = np.repeat(np.asarray(vals), S)
    ids = G.group_ids(B, S, T, END, S)
    w, _, _, adv, base = G.weights_group(ids, rw, None, 1, END)
    assert np.array_equal(bits64(adv), bits64(np.zeros(B * S)))                   # +0.0, never -0.0
    assert np.array_equal(w.view(np.int32), np.zeros(T * B * S, dtype=np.int32))
    # ... which reward - mean(others) does not give: three copies of 0.1 sum to 0.30000000000000004
    assert 0.1 + 0.1 + 0.1 != 0.3 and (0.1 + 0.1 + 0.1) / 3.0 != 0.1
    np.testing.assert_allclose(base, rw, rtol=4e-16)


def test_one_sample_mode_0_is_the_single_sample_reference_bit_for_bit():
    rng = np.random.Generator(np.random.PCG64(5))
    B, T = 11, 5
    ids = G.group_ids(B, 1, T, END, 7)
    rw, bl = rng.random(B) * 3, rng.random(B) * 3
    for baseline, denom in ((bl, None), (None, None), (bl, 77.0)):
        w, ln, M, adv, base = G.weights_group(ids, rw, baseline, 0, END, denom)
        w1, ln1, M1 = S1.weights(ids.reshape(B, T), rw, baseline, END, denom)
        assert np.array_equal(w.view(np.int32), w1.view(np.int32)) and np.array_equal(ln, ln1) and M == M1
        assert np.array_equal(adv, rw - (0.0 if baseline is None else baseline))


def test_mode_0_repeats_the_image_baseline_and_leave_one_out_is_the_mean_of_the_others():
    B, S, T = 4, 4, 6                                                             # S = 4: the division by 3 is inexact
    ids, rw = G.group_ids(B, S, T, END, 2), G.group_rewards(B, S, 2)
    bl = np.array([0.5, -0.25, 0.0, 1.5])
    w, ln, M, adv, base = G.weights_group(ids, rw, bl, 0, END)
    w1, ln1, M1 = S1.weights(ids.reshape(B * S, T), rw, np.repeat(bl, S), END)
    assert np.array_equal(w.view(np.int32), w1.view(np.int32)) and np.array_equal(ln, ln1) and M == M1
    assert np.array_equal(base, np.repeat(bl, S)) and set(ln.tolist()) >= {1, T}
    _, _, _, adv, base = G.weights_group(ids, rw, None, 1, END)
    r2 = rw.reshape(B, S)
    others = (r2.sum(1, keepdims=True) - r2) / (S - 1)
    np.testing.assert_allclose(base.reshape(B, S), others, rtol=0, atol=1e-15)
    np.testing.assert_allclose(adv.reshape(B, S), r2 - others, rtol=0, atol=1e-15)
    assert not adv.reshape(B, S)[B // 2].any()                                    # the image whose samples all scored 0.1
    assert (rw < 0).any() and (rw == 0).any()


def test_group_sum_is_sequential_float32():
    x = np.array([[1.0], [2.0 ** -24], [2.0 ** -24], [1.0], [1.0], [1.0]], dtype=np.float32)
    out = G.group_sum_rows(x, 3)
    assert out.dtype == np.float32 and out.shape == (2, 1)
    assert out[0, 0] == np.float32(1.0) and out[1, 0] == np.float32(3.0)          # (1 + 2^-24) + 2^-24 rounds back to 1 twice
    assert np.array_equal(G.group_sum_rows(x, 1), x)


# ---- argument errors, before any launch ------------------------------------------------------------------------------------------
def weights_group_call(lib, **kw):
    P = C.c_void_p(4096)                        # never dereferenced: every check below fails first
    a = dict(G.WEIGHTS_GROUP_VALID, ids=P, reward=P, w=P, len=P, m=P, adv=P, base=P)
    a.update(kw)
    if a["baseline"] == "PTR":
        a["baseline"] = P
    return lib.sat_scst_weights_group(a["ids"], a["stride"], a["B"], a["S"], a["T"], END, a["reward"], a["baseline"], a["mode"],
                                      a["denom"], a["w"], a["len"], a["m"], a["adv"], a["base"], None)


def test_weights_group_argument_errors_come_back_before_any_launch():
    lib = L.load()
    for kw in G.WEIGHTS_GROUP_ARG_ERRORS:
        assert weights_group_call(lib, **kw) == ARG, kw
    for kw in G.WEIGHTS_GROUP_UNSUPPORTED:
        assert weights_group_call(lib, **kw) == UNSUPPORTED, kw


def group_sum_call(lib, **kw):
    base_in, base_out = 1 << 20, 1 << 16
    a = dict(G.GROUP_SUM_VALID, inp=base_in, out=base_out)
    a.update(kw)
    if isinstance(a["out"], str):               # "in+N" / "in-N": an output N bytes from the input
        a["out"] = base_in + int(a["out"][2:])
    return lib.sat_group_sum_rows(a["inp"], a["ld_in"], a["B"], a["S"], a["W"], a["out"], a["ld_out"], None)


def test_group_sum_argument_errors_come_back_before_any_launch():
    lib = L.load()
    for kw in G.GROUP_SUM_ARG_ERRORS:
        assert group_sum_call(lib, **kw) == ARG, kw


# ---- the Python layer's refusals, on the host -----------------------------------------------------------------------------------
BAD_GROUPS = [dict(num_samples=1, baseline="sample_mean"), dict(baseline="sample_mean"), dict(num_samples=3, baseline="mean"),
              dict(num_samples=3, baseline=None), dict(num_samples=2.0), dict(num_samples="3"), dict(num_samples=True),
              dict(num_samples=0), dict(num_samples=-2, baseline="sample_mean")]


@pytest.mark.parametrize("kw", BAD_GROUPS)
def test_bad_num_samples_and_baselines_raise_value_error_without_a_gpu(kw):
    with pytest.raises(ValueError):
        sat.SelfCritical(None, END, **kw)
    model = sat.ShowAndTell(8, 16, 50, 1, arch=dict(layers=(1, 1, 1, 1), width=8))
    with pytest.raises(ValueError):                                     # before the encoder runs (which would refuse CPU images)
        model.scst_forward(torch.zeros(2, 3, 32, 32), [0, 1], None, **kw)
    att = sat.ShowAttendTellModel(16 + 8, 8, 50, 16, None, feature_size=(4, 8), compute_dtype="f32", vgg_cfg=[8, "M", 8])
    with pytest.raises(ValueError):
        att.scst_forward(torch.zeros(2, 3, 32, 32), [0, 1], None, **kw)
    engine = object.__new__(sat.TrainStep)                              # no GPU to build one on: the check comes first of all
    with pytest.raises(ValueError):
        engine.scst_step(torch.zeros(2, 8), [0, 1], None, **kw)
    with pytest.raises(ValueError):
        engine.scst_forward_backward(torch.zeros(2, 8), [0, 1], None, **kw)


def test_rollouts_and_loss_refuse_on_the_host():
    dec = sat.DecoderRNN(8, 16, 50, 1)
    for bad in (0, 2.0, True, "2"):
        with pytest.raises(ValueError, match="num_samples"):
            dec.rollout(torch.zeros(2, 8), 3, num_samples=bad)
    att = sat.ShowAttendTellModel(16 + 8, 8, 50, 16, None, feature_size=(4, 8), compute_dtype="f32", vgg_cfg=[8, "M", 8])
    with pytest.raises(ValueError, match="arg-max"):
        att.rollout(torch.zeros(2, 4, 8), torch.zeros(2, 8), 3, greedy=True, num_samples=2)
    with pytest.raises(ValueError, match="num_samples"):
        att.rollout(torch.zeros(2, 4, 8), torch.zeros(2, 8), 3, num_samples=0)
    logits, ids = torch.zeros(12, 50), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="sample_mean"):
        sat.scst_loss(logits, ids, torch.zeros(4), "sample_mean")                       # one sample per image
    with pytest.raises(ValueError, match="sample_mean"):
        sat.scst_loss(logits, ids.view(4, 1, 3), torch.zeros(4), "sample_mean")
    with pytest.raises(ValueError):
        sat.scst_loss(logits, ids, torch.zeros(4), "greedy", num_samples=2)             # a name that is no tensor and no rule
    with pytest.raises(ValueError, match="num_samples"):
        sat.scst_loss(logits, ids, torch.zeros(4), None, num_samples=1.5)
    with pytest.raises(ValueError, match="num_samples says 4"):
        sat.scst_loss(logits, ids.view(2, 2, 3), torch.zeros(4), "sample_mean", num_samples=4)   # ids name S = 2 themselves
    with pytest.raises(ValueError):
        sat.group_sum_rows(torch.zeros(4, 3), 0)
    assert "out" not in inspect.signature(sat.scst_loss).parameters
    with pytest.raises(ValueError):
        sat.scst_weights_group(ids.view(2, 2, 3), torch.zeros(4), "loo")
    # what passes the host checks goes on to the device path, which has no CPU form
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sat.scst_loss(logits, ids, torch.zeros(4), "sample_mean", num_samples=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sat.scst_weights_group(ids.view(2, 2, 3), torch.zeros(4), "sample_mean")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sat.group_sum_rows(torch.zeros(4, 3), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.rollout(torch.zeros(2, 8), 3, num_samples=2)


def test_defaults_of_the_new_keywords():
    for fn in (sat.DecoderRNN.rollout, sat.ShowAttendTellModel.rollout, sat.scst_loss, sat.ShowAndTell.scst_forward,
               sat.ShowAttendTellModel.scst_forward, sat.TrainStep.scst_step, sat.TrainStep.scst_forward_backward):
        assert inspect.signature(fn).parameters["num_samples"].default == 1, fn
    for fn in (sat.SelfCritical.__init__, sat.ShowAndTell.scst_forward, sat.ShowAttendTellModel.scst_forward, sat.TrainStep.scst_step):
        p = inspect.signature(fn).parameters
        assert p["baseline"].default == "greedy" and p["num_samples"].default == 1, fn
    for name in ("num_samples", "baseline"):
        assert inspect.signature(sat.SelfCritical.__init__).parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
