"""CPU: scheduled sampling's host side -- the numpy Philox4x32-10 against the Random123 known-answer vectors, the Gumbel-max
sampler's frequencies against softmax, the epoch schedule of train.py:109-113, and the new C-ABI entry points (exported,
bound, argument errors reported without a launch)."""
import importlib
import math

import numpy as np
import pytest
import torch

import ss_reference as R

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib


def hexwords(w):
    return " ".join("%08x" % int(x) for x in w)


@pytest.mark.parametrize("ctr,key,expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, expect):
    assert hexwords(R.philox4x32_10(*ctr, *key)) == expect


def test_uniform_range_is_open():
    u = R.uniform(np.array([0, 255, 0xffffffff], dtype=np.uint32))
    assert u[0] == u[1] == 0.5 * 2.0 ** -24 and u[2] == 1.0 - 0.5 * 2.0 ** -24
    assert np.all(np.isfinite(R.gumbel(np.array([0, 0xffffffff], dtype=np.uint32))))


# chi-square critical value at p = 1e-3 for 9 degrees of freedom
CHI2_9_P001 = 27.877


def test_gumbel_max_frequencies_match_softmax():
    V, n = 10, 200000
    logits = np.array([2.0, 1.0, 0.5, 0.0, -0.5, -1.0, 1.5, 0.25, -2.0, 0.75])
    k0, k1 = R.seed_key(0x0123456789ABCDEF)
    v = np.arange(V)
    b = np.arange(n)[:, None]
    words = R.philox4x32_10(v[None, :] >> 2, b, 7, 0, k0, k1)          # counter (v >> 2, b, t, 2*rank): one draw per row b
    x = np.choose(np.broadcast_to(v & 3, (n, V)), words)
    draws = np.argmax(logits[None, :] + R.gumbel(x), axis=1)
    p = np.exp(logits - logits.max())
    p /= p.sum()
    obs = np.bincount(draws, minlength=V)
    chi2 = float(((obs - n * p) ** 2 / (n * p)).sum())
    assert chi2 < CHI2_9_P001, (chi2, obs, n * p)


def test_mask_frequency_matches_ss_prob():
    n, prob = 20000, 0.25
    k0, k1 = R.seed_key(99)
    u = R.uniform(R.philox4x32_10(0, np.arange(n), 3, 1, k0, k1)[0])
    frac = float((u < prob).mean())
    assert abs(frac - prob) < 4 * math.sqrt(prob * (1 - prob) / n)


def reference_schedule(epoch, start, every, inc, mx, prev=0.0):
    """train.py:109-113 as written (the attribute keeps its previous value outside the branch: 0 from DecoderRNN.__init__)"""
    if epoch > start and start >= 0:
        fraction = (epoch - start) // every
        return min(inc * fraction, mx)
    return prev


@pytest.mark.parametrize("cfg", [dict(), dict(start=0), dict(start=3, increase_every=2, increase_prob=0.1, max_prob=0.4),
                                 dict(start=-1, increase_every=1, increase_prob=0.5)])
def test_ss_prob_schedule_matches_reference_formula(cfg):
    full = dict(start=-1, increase_every=5, increase_prob=0.05, max_prob=0.25)
    full.update(cfg)
    for epoch in range(41):
        want = reference_schedule(epoch, full["start"], full["increase_every"], full["increase_prob"], full["max_prob"])
        assert sat.ss_prob_for_epoch(epoch, **cfg) == pytest.approx(want, abs=0), (epoch, cfg)
    if full["start"] < 0:
        assert all(sat.ss_prob_for_epoch(e, **cfg) == 0 for e in range(41))


def test_ss_symbols_exported_and_bound():
    lib = L.load()
    for name in ("sat_ss_decoder_fwd", "sat_ss_decoder_fwd_ws_bytes", "sat_vocab_sample"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.sat_ss_decoder_fwd_ws_bytes(64, 10000) == 64 * 625 * 8
    assert callable(sat.ss_prob_for_epoch)


def test_ss_argument_errors_are_reported_not_computed():
    lib = L.load()
    assert lib.sat_vocab_sample(None, None, None, 4, 64, 100, None, 0, 0.5, 1, 2, 0, None, 0, None, 0, None, 0, None, None, 0,
                                None) == 1001
    bs = (L.C.c_int32 * 3)(4, 4, 4)
    assert lib.sat_ss_decoder_fwd(None, None, None, 0, bs, None, 3, 32, 100, None, 1, 64, None, None, None, None, None, 0, 0.5, 1,
                                  0, None, 0, None, 0, None) == 1001


def test_decoder_ss_attributes_and_seed_stream():
    dec = sat.DecoderRNN(8, 8, 20, 1)
    assert dec.ss_prob == 0 and dec.ss_rank == 0 and dec.last_ss_inputs is None and dec.last_ss_seed is None
    torch.manual_seed(5)
    a = sat.models.draw_ss_seed()
    torch.manual_seed(5)
    assert sat.models.draw_ss_seed() == a and 0 <= a < 2 ** 63
