"""CPU: the attention maps and the doubly stochastic penalty of Show-Attend-Tell -- the f64 restatement (tests/alpha_reference.py)
against the maps the reference class's own `attention_layer` returns (tests/golden/alpha/G10, made by
tests/golden/make_goldens_alpha.py), the fixture's recipe, the penalty's closed form, and the condition under which the GPU
model test can see a dropped penalty gradient."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import alpha_reference as AR
from oracle import attend as OA
from oracle import decoder as OD

HERE = os.path.dirname(os.path.abspath(__file__))
G10 = os.path.join("alpha", "G10_attend_alphas.npz")


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def g6_case(golden_dir):
    """G6's parameters and inputs in float64, the model's lengths (train.py:134) and the packed targets"""
    g = load(golden_dir, "G6_attend_small.npz")
    hidden, context, vocab, embed, B, T, P, feat = [int(x) for x in g["dims"]]
    params = OA.init_attend_params(hidden, context, vocab, embed, generator=torch.Generator().manual_seed(int(g["seed"])), feat=feat)
    p64 = {k: v.double() for k, v in params.items()}
    feats, caps = torch.from_numpy(g["features"]).double(), torch.from_numpy(g["captions"])
    l1 = [int(x) - 1 for x in g["lengths"]]
    return g, p64, feats, caps, l1, OD.pack_time_major(caps[:, 1:], l1)


def test_restatement_reproduces_the_reference_maps_and_penalty(golden_dir):
    g, p, feats, caps, l1, _ = g6_case(golden_dir)
    z = load(golden_dir, G10)
    assert [int(x) for x in z["dims"]] == [int(x) for x in g["dims"]] and int(z["seed"]) == int(g["seed"])
    logits, alphas = AR.forward(p, feats, caps[:, :-1], l1)
    np.testing.assert_allclose(logits.numpy(), g["logits"], rtol=0, atol=2e-6)          # same inputs as G6
    packed = torch.cat(alphas, 0)
    assert z["alphas_train"].shape == tuple(packed.shape) == (sum(l1), feats.shape[1])
    # f64 against the reference's f32 maps: values in [0, 1], a few f32 roundings of the scores in front of the softmax
    np.testing.assert_allclose(packed.numpy(), z["alphas_train"], rtol=0, atol=2e-7)
    assert abs(AR.penalty(alphas, feats.shape[0]).item() - float(z["penalty_alpha_c_1"])) < 1e-6 * float(z["penalty_alpha_c_1"])
    for key, states in (("zero_state", None), ("init_state", OA.init_lstm(p, feats))):
        ids, maps = AR.greedy(p, feats, states)
        assert np.array_equal(ids.numpy(), g["sample_ids_" + key])
        assert z["alphas_greedy_" + key].shape == (4, 20, 16)
        np.testing.assert_allclose(maps.numpy(), z["alphas_greedy_" + key], rtol=0, atol=2e-6)
    # the beam loop at width 1 is the greedy loop, maps included
    ids1, _, maps1 = AR.beam(p, feats, 1)
    gi, gm = AR.greedy(p, feats)
    assert torch.equal(ids1[:, 0], gi) and torch.equal(maps1[:, 0], gm)


@pytest.mark.skipif(not os.path.exists(os.path.join(HERE, "..", "oracle", "_ref", "model2.pyc")),
                    reason="needs oracle/_ref, which build() compiles only where the reference checkout is present")
def test_g10_regenerates_bit_equal_from_the_reference(golden_dir, tmp_path):
    subprocess.check_call([sys.executable, os.path.join(golden_dir, "make_goldens_alpha.py"), str(tmp_path)], stdout=subprocess.DEVNULL)
    a, b = np.load(os.path.join(tmp_path, os.path.basename(G10))), np.load(os.path.join(golden_dir, G10))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert sorted(os.listdir(os.path.join(golden_dir, "alpha"))) == [os.path.basename(G10)]      # no fixture without its recipe


@pytest.mark.parametrize("T,P,alpha_c", [(5, 16, 1.0), (20, 13, 0.5), (7, 7, 2.0)])
def test_uniform_maps_give_the_closed_form(T, P, alpha_c):
    """alpha = 1/P everywhere over T steps of equal lengths: every coverage is T/P, the penalty alpha_c (1 - T/P)^2"""
    B = 3
    alphas = [torch.full((B, P), 1.0 / P, dtype=torch.float64) for _ in range(T)]
    assert abs(AR.penalty(alphas, B, alpha_c).item() - alpha_c * (1 - T / P) ** 2) < 1e-14
    ragged = alphas[:2] + [a[:1] for a in alphas[2:]]                # image 0 lives T steps, the others 2
    want = alpha_c * ((1 - T / P) ** 2 + 2 * (1 - 2 / P) ** 2) / 3
    assert abs(AR.penalty(ragged, B, alpha_c).item() - want) < 1e-14


def test_penalty_moves_the_attention_gradients_far_beyond_the_gpu_tolerance(golden_dir):
    """Sensitivity condition of tests/test_gpu_alpha.py's model test: at AR.MODEL_TEST_ALPHA_C the gradients of weight_att,
    weight_hh.weight and image_att_w with and without the penalty differ in norm by more than 100 x the tolerance that test
    allows (rtol 2e-3 of the norm + atol 2e-7 per element), so a backward that drops the injected term cannot pass it.
    Measured: alpha_c = 1 gives 4667 x / 9.2 x / 841 x (weight_hh.weight too close), alpha_c = 16 gives 77812 x / 170 x / 14309 x."""
    _, p, feats, caps, l1, targets = g6_case(golden_dir)
    without = AR.loss_and_grads(p, feats, caps[:, :-1], l1, targets, 0.0)["grads"]
    with_pen = AR.loss_and_grads(p, feats, caps[:, :-1], l1, targets, AR.MODEL_TEST_ALPHA_C)["grads"]
    for k in ("weight_att", "weight_hh.weight", "image_att_w"):
        a, b = with_pen[k], without[k]
        tol = AR.GRAD_RTOL * b.norm().item() + AR.GRAD_ATOL * b.numel() ** 0.5
        print("%-18s |norm difference| / tol = %.1f, norm of the difference / tol = %.1f"
              % (k, abs(a.norm().item() - b.norm().item()) / tol, (a - b).norm().item() / tol))
        assert abs(a.norm().item() - b.norm().item()) > 100 * tol, k
        assert (a - b).norm().item() > 100 * tol, k
