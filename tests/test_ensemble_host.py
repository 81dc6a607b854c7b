"""CPU: the ensemble references of tests/ensemble_reference.py checked against their own identities, the consensus construction,
the argument checks of `sat.Ensemble` (none needs a GPU), and the whole-decode cases the GPU tests use: their seeds are searched
against the CPU restatement only, and the share of images a GPU comparison may leave out (key gap <= 2e-4) is asserted HERE to be
at most a quarter, so the GPU tests cannot hide a failure behind the exclusion."""
import functools
import importlib

import numpy as np
import pytest
import torch

import beam_constraints_reference as BC
import beam_reference as R
import ensemble_reference as ER

sat = importlib.import_module("show-and-tell_amd")
Ensemble = sat.Ensemble                              # (a tree without the feature fails here: the whole module, references included)


# ---- the reference's own identities ----
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_identical_members_in_prob_mode_are_log_softmax(M):
    x = ER.planted_rows(203, 7, 3)
    for weights in (None, list(range(1, M + 1))):
        out = ER.combine_ref([x] * M, weights, 0)
        assert np.abs(out - R.log_softmax64(x)).max() < 1e-6        # (the f32 rounding of the weights: they sum to 1 within 1e-7)
    out1 = ER.combine_ref([x] * M, None, 1)
    assert np.abs(out1 - R.log_softmax64(x)).max() < 1e-6           # equal members: the log-probability mean too


def test_weights_normalise_and_prob_mode_is_a_distribution():
    xs = [ER.planted_rows(257, 5, s) for s in range(3)]
    a, b = ER.combine_ref(xs, [1.0, 2.0, 5.0], 0), ER.combine_ref(xs, [10.0, 20.0, 50.0], 0)
    assert np.array_equal(a, b)
    assert np.abs(np.exp(a).sum(1) - 1.0).max() < 1e-6
    assert np.array_equal(ER.combine_ref(xs, None, 0), ER.combine_ref(xs, [3.0, 3.0, 3.0], 0))
    w = ER.weights32([1.0, 3.0], 2)
    assert w.tolist() == [0.25, 0.75]
    # mode 0 against the definition, directly
    p = sum(wm * np.exp(R.log_softmax64(x)) for wm, x in zip(ER.weights32([1.0, 2.0, 5.0], 3), xs))
    assert np.abs(a - np.log(p)).max() < 1e-12
    # mode 1 is the weighted mean of log-probabilities and is NOT normalised
    l = ER.combine_ref(xs, [1.0, 2.0, 5.0], 1)
    assert np.abs(l - sum(wm * R.log_softmax64(x) for wm, x in zip(ER.weights32([1.0, 2.0, 5.0], 3), xs))).max() < 1e-12
    assert (np.exp(l).sum(1) < 1.0 - 1e-3).all()


def test_minus_inf_columns_follow_the_rule_of_each_mode():
    xs = [ER.planted_rows(11, 3, s) for s in range(3)]
    xs[0][:, 4] = -np.inf                                           # one member only
    for x in xs:
        x[:, 7] = -np.inf                                           # every member
    p, l = ER.combine_ref(xs, None, 0), ER.combine_ref(xs, None, 1)
    assert np.isfinite(p[:, 4]).all() and np.isneginf(p[:, 7]).all()
    assert np.isneginf(l[:, 4]).all() and np.isneginf(l[:, 7]).all()
    rest = [v for v in range(11) if v not in (4, 7)]
    assert np.isfinite(p[:, rest]).all() and np.isfinite(l[:, rest]).all() and not np.isnan(p).any() and not np.isnan(l).any()


@pytest.mark.parametrize("M", [2, 3, 8])
@pytest.mark.parametrize("mode", [0, 1])
def test_consensus_flips_the_winner(M, mode):
    """every member alone picks its own column, the ensemble picks the shared runner-up -- by the f64 reference alone"""
    xs, own, shared = ER.consensus_rows(M, 10, 203, np.random.default_rng(M))
    out = ER.combine_ref(xs, None, mode)
    assert out.argmax(1).tolist() == shared.tolist()
    for m in range(M):
        assert xs[m].argmax(1).tolist() == own[m].tolist() and (own[m] != shared).all()
    assert len({tuple(o) for o in own}) == M


# ---- sat.Ensemble's argument checks: all on the host ----
def _dec(V=50, E=8, H=16):
    return sat.DecoderRNN(E, H, V, 1)


def test_ensemble_argument_checks_need_no_gpu():
    a, b = _dec(), _dec()
    ens = sat.Ensemble([a, b])
    assert ens.mode == "prob" and ens.weights is None and ens.vocab_size == 50
    assert sat.Ensemble([a, b], [1, 3], "logprob").weights == [1.0, 3.0]
    with pytest.raises(ValueError):
        sat.Ensemble([])                                            # M = 0
    with pytest.raises(ValueError):
        sat.Ensemble([a] * 9)                                       # M = 9
    sat.Ensemble([a] * 8)
    with pytest.raises(ValueError):
        sat.Ensemble([a, _dec(V=51)])                               # V mismatch
    for bad in ([1.0, 0.0], [1.0, -2.0], [1.0, float("nan")], [1.0, float("inf")], [1.0], [1.0, "x"], [1.0, 1e-60]):
        with pytest.raises(ValueError):
            sat.Ensemble([a, b], bad)
    with pytest.raises(ValueError):
        sat.Ensemble([a, b], mode="mean")
    model = sat.ShowAndTell(8, 16, 50, 1, arch=dict(layers=(1, 1, 1, 1), width=8), compute_dtype="f32")
    with pytest.raises(NotImplementedError):
        sat.Ensemble([a, model])                                    # a mixed family
    with pytest.raises(NotImplementedError):
        sat.Ensemble([a, torch.nn.Linear(2, 2)])
    assert sat.Ensemble([model, model]).family is sat.ShowAndTell
    with pytest.raises(NotImplementedError):
        ens.sample_beam(torch.zeros(1, 3, 8, 8))                    # DecoderRNN members have no encoder
    # keyword checks run before the device is touched (CPU tensors would raise RuntimeError behind them)
    feats = [torch.zeros(2, 8), torch.zeros(2, 8)]
    with pytest.raises(ValueError):
        ens.sample_beam_features(feats, beam_size=9)
    with pytest.raises(ValueError):
        ens.sample_beam_features(feats, beam_size=4, num_beam_groups=3)
    with pytest.raises(ValueError):
        ens.sample_beam_features(feats, beam_size=4, min_length=2)  # needs an end_id
    with pytest.raises(ValueError):
        ens.sample_beam_features(feats[:1], beam_size=4)
    with pytest.raises(ValueError):
        ens.sample_beam_features([torch.zeros(2, 8), torch.zeros(3, 8)], beam_size=4)


# ---- the whole-decode cases of tests/test_gpu_ensemble.py ----
@functools.lru_cache(maxsize=None)
def _case(kind):
    return ER.decoder_case(kind)


@pytest.mark.parametrize("kind", ["plain", "logprob", "constrained", "grouped", "greedy", "copies", "wide", "wide_x3"])
def test_decoder_cases_leave_out_at_most_a_quarter(kind):
    w = _case(kind)
    out = int((w["ref"]["gap"] <= ER.GAP).sum())
    print("%s: seed %d, %d of %d images left out, smallest gap %.3g" % (kind, w["seed"], out, w["B"], float(w["ref"]["gap"].min())))
    assert out * 4 <= w["B"]
    assert tuple(w["ref"]["ids"].shape) == (w["B"], w["K"], 20)
    if kind in ("plain", "logprob"):
        assert (w["ref"]["ids"] == ER.END).any()                    # finished hypotheses occur
    if kind == "constrained":
        assert w["ref"]["nbans"] > 0
    if kind == "grouped":
        assert w["ref"]["npen"] > 0


def test_the_ensemble_decodes_what_no_member_decodes_alone():
    w = _case("plain")
    keep = (w["ref"]["gap"] > ER.GAP).numpy()
    for (p, Lh), f in zip(w["members"], w["feats"]):
        own = BC.decoder_beam(p, f, w["K"], Lh, ER.END, BC.Constraints())
        assert (own["ids"].numpy()[keep] != w["ref"]["ids"].numpy()[keep]).any()


def test_three_copies_in_prob_mode_decode_as_the_model_itself():
    w = _case("copies")
    p, Lh = w["members"][0]
    own = BC.decoder_beam(p, w["feats"][0], w["K"], Lh, ER.END, BC.Constraints())
    keep = ((w["ref"]["gap"] > ER.GAP) & (own["gap"] > ER.GAP)).numpy()
    assert keep.sum() * 4 >= 3 * ER.B_DEC
    assert np.array_equal(own["ids"].numpy()[keep], w["ref"]["ids"].numpy()[keep])
    assert np.abs(own["scores"].numpy()[keep] - w["ref"]["scores"].numpy()[keep]).max() < 1e-4


@pytest.mark.parametrize("constrained", [False, True])
def test_attend_cases_leave_out_at_most_a_quarter(constrained):
    w = ER.attend_case(constrained)
    B = w["dims"][4]
    out = int((w["ref"]["gap"] <= ER.GAP).sum())
    print("attend constrained=%s: seed %d, %d of %d images left out" % (constrained, w["seed"], out, B))
    assert out * 4 <= B
    if constrained:
        assert w["ref"]["nbans"] > 0
