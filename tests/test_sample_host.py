"""CPU: the reference of the filtered draw (tests/sample_reference.py) on hand-made rows and against the filtered softmax's
frequencies; the new entry points' size functions; every argument error of the two `sample_stochastic` methods, raised before the
library or a GPU is touched."""
import importlib
import math

import numpy as np
import pytest
import torch

import sample_reference as R
import ss_reference as SS

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
NINF = -np.inf


def test_hand_made_rows():
    # all equal: the order is the column order, k cuts by count, p cuts by count (every w = 1: 4 of 10 reach 0.35 * 10)
    x = np.full(10, 1.5, dtype=np.float32)
    order, n, clr = R.kept_prefix(x, 1.0, 0, 1.0)
    assert order.tolist() == list(range(10)) and n == 10 and clr == np.inf
    assert R.kept_prefix(x, 1.0, 3, 1.0)[1] == 3 and R.kept_prefix(x, 0.5, 10, 1.0)[1] == 10 and R.kept_prefix(x, 2.0, 11, 1.0)[1] == 10
    order, n, clr = R.kept_prefix(x, 1.0, 0, 0.35)
    assert n == 4 and abs(clr - 0.05) < 1e-7                 # (p is rounded to f32)
    assert R.kept_prefix(x, 1.0, 3, 0.35)[1] == 2            # after top-k: Z = 3, 0.35 * 3 = 1.05 needs two
    # +0.0 and -0.0 tie: ascending column decides
    x = np.array([-0.0, 0.0, -1.0, 0.0, -0.0], dtype=np.float32)
    assert R.kept_prefix(x, 1.0, 0, 1.0)[0].tolist() == [0, 1, 3, 4, 2]
    assert R.kept_prefix(x, 1.0, 3, 1.0)[1] == 3
    # -inf columns are no candidates; fewer finite ones than k: all of them stay
    x = np.array([NINF, 2.0, NINF, 3.0, NINF], dtype=np.float32)
    order, n, _ = R.kept_prefix(x, 1.0, 4, 1.0)
    assert order.tolist() == [3, 1] and n == 2
    assert R.kept_prefix(x, 1.0, 1, 1.0)[1] == 1
    # k = 1: the first maximal column, logp 0, whatever the noise
    x = np.array([0.5, 7.0, 7.0, -3.0], dtype=np.float32)
    order, n, _ = R.kept_prefix(x, 0.7, 1, 1.0)
    assert order[:n].tolist() == [1]
    for seed in range(5):
        tok, margin = R.draw(x, 0.7, order[:n], seed, 0, 0, 0)
        assert tok == 1 and margin == np.inf and R.logp(x, 0.7, order[:n], tok) == 0.0
    # p so small that one token stays; temperature sharpens the masses
    x = np.array([0.0, 1.0, 2.0, 3.0], dtype=np.float32)
    order, n, clr = R.kept_prefix(x, 1.0, 0, 1e-3)
    assert order.tolist() == [3, 2, 1, 0] and n == 1 and clr > 1e-4
    w = np.exp(np.array([0.0, -1.0, -2.0, -3.0]) / 0.5)
    assert R.kept_prefix(x, 0.5, 0, 0.9)[1] == int(np.searchsorted(np.cumsum(w), float(np.float32(0.9)) * w.sum())) + 1 == 2
    assert R.kept_prefix(x, 1.0, 0, 0.9)[1] == 3
    # logp is the log of the filtered softmax
    order, n, _ = R.kept_prefix(x, 1.7, 3, 0.95)
    pr = R.probabilities(x, 1.7, 3, 0.95)
    assert abs(pr.sum() - 1) < 1e-15 and np.count_nonzero(pr) == n
    for v in order[:n]:
        assert abs(R.logp(x, 1.7, order[:n], v) - math.log(pr[v])) < 1e-14
    # the unfiltered draw is ss_reference's
    g = SS.noise(11, 2, 3, 4, 4)
    assert R.draw(x, 1.0, np.arange(4), 11, 2, 3, 4)[0] == int(np.argmax(x.astype(np.float64) + g))


def _noise_many(seeds, V):
    """G(0, 0, v) of many seeds at once, [len(seeds), V] (ss_reference.noise, vectorised over the key)"""
    seeds = np.asarray(seeds, dtype=np.uint64)
    k0 = (seeds & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    k1 = (seeds >> np.uint64(32)).astype(np.uint32)[:, None]
    v = np.arange(V)[None, :]
    words = SS.philox4x32_10(v >> 2, 0, 0, 0, k0, k1)
    words = [np.broadcast_to(w, (len(seeds), V)) for w in words]
    return SS.gumbel(np.choose(np.broadcast_to(v & 3, (len(seeds), V)), words))


@pytest.mark.parametrize("tau,k,p", [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 5, 1.0), (1.3, 0, 0.8), (0.5, 6, 0.9)])
def test_reference_frequencies_match_the_filtered_softmax(tau, k, p):
    """20 000 seeds on one V = 8 row: Pearson's chi-square of the token counts against the filtered softmax.

    Bound: with d = kept - 1 degrees of freedom, P(chi2_d >= d + 2 sqrt(d t) + 2 t) <= exp(-t) (Laurent and Massart 2000); t = 14
    puts a correct sampler over it less than once in 10^6 seed sets.  The reference meets it on its own because the Gumbel-max of
    x / tau + G over the kept columns IS a draw from their softmax, and Philox streams of different keys are independent: the
    counts are multinomial.  The seeds are fixed, so the outcome is too."""
    N, V = 20000, 8
    x = np.random.default_rng(5).normal(0, 1.5, V).astype(np.float32)
    order, n, _ = R.kept_prefix(x, tau, k, p)
    kept = np.sort(order[:n])
    seeds = np.arange(1000, 1000 + N)
    G = _noise_many(seeds, V)
    for i in (0, 1, N - 1):                                   # the vectorised noise is ss_reference.noise
        assert np.array_equal(G[i], SS.noise(int(seeds[i]), 0, 0, 0, V))
        assert R.draw(x, tau, kept, int(seeds[i]), 0, 0, 0)[0] == int(kept[np.argmax(x[kept].astype(np.float64) / float(np.float32(tau)) + G[i, kept])])
    tok = kept[np.argmax(x[kept].astype(np.float64)[None, :] / float(np.float32(tau)) + G[:, kept], axis=1)]
    counts = np.bincount(tok, minlength=V)
    pr = R.probabilities(x, tau, k, p)
    assert counts[pr == 0].sum() == 0                         # nothing outside the kept set
    exp = N * pr[kept]
    chi2 = float(((counts[kept] - exp) ** 2 / exp).sum())
    d, t = n - 1, 14.0
    bound = d + 2 * math.sqrt(d * t) + 2 * t
    print("kept %d  chi2 %.2f  bound %.2f" % (n, chi2, bound))
    assert n >= 2 and exp.min() > 5 and chi2 < bound


def test_ws_bytes_are_zero_for_non_positive_sizes():
    lib = L.load()
    assert lib.sat_sample_filtered_ws_bytes(3, 100) > 0 and lib.sat_sample_decode_ws_bytes(3, 8, 16, 100, 1) > 0
    for a in ((0, 100), (-1, 100), (3, 0), (3, -5)):
        assert lib.sat_sample_filtered_ws_bytes(*a) == 0, a
    for a in ((0, 8, 16, 100, 1), (3, 0, 16, 100, 1), (3, 8, 0, 100, 1), (3, 8, 16, 0, 1), (3, 8, 16, 100, 0), (-3, 8, 16, 100, 1)):
        assert lib.sat_sample_decode_ws_bytes(*a) == 0, a
    assert lib.sat_sample_decode_ws_bytes(3, 8, 16, 101, 1) >= 3 * 104 * 4 + lib.sat_sample_filtered_ws_bytes(3, 101)


BAD = [("temperature", 0), ("temperature", -1.0), ("temperature", float("inf")), ("temperature", float("nan")), ("temperature", "hot"),
       ("temperature", 1e-60), ("top_k", -1), ("top_k", 2.5), ("top_k", True), ("top_p", 0), ("top_p", 1.5), ("top_p", -0.1),
       ("top_p", float("nan")), ("top_p", 1e-60), ("num_samples", 0), ("num_samples", 1.5), ("seed", -1), ("seed", 2 ** 64), ("seed", 0.5)]


@pytest.mark.parametrize("name,value", BAD)
def test_argument_errors_raise_value_error_without_a_gpu(name, value, monkeypatch):
    """bad arguments are named in a ValueError before the library is loaded (load() is made to fail) -- and before the CPU tensors
    would be refused"""
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load", no_load)
    dec = sat.DecoderRNN(8, 16, 50, 1)
    with pytest.raises(ValueError, match=name):
        dec.sample_stochastic(torch.zeros(2, 8), **{name: value})
    model = sat.ShowAndTell(8, 16, 50, 1, arch=dict(layers=(1, 1, 1, 1), width=8))
    with pytest.raises(ValueError, match=name):
        model.sample_stochastic(torch.zeros(2, 3, 32, 32), **{name: value})
    att = sat.ShowAttendTellModel(28, 16, 101, 12, None, feature_size=(9, 16), compute_dtype="f32", vgg_cfg=[8, "M", 16])
    with pytest.raises(ValueError, match=name):
        att.sample_stochastic_features(torch.zeros(2, 9, 16), **{name: value})
    with pytest.raises(ValueError, match=name):
        att.sample_stochastic(torch.zeros(2, 3, 8, 8), **{name: value})


def test_good_arguments_reach_the_device_check():
    """valid arguments pass the checks; CPU tensors are then refused as everywhere else"""
    dec = sat.DecoderRNN(8, 16, 50, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.sample_stochastic(torch.zeros(2, 8), temperature=0.7, top_k=5, top_p=0.9, num_samples=2, seed=3)
    att = sat.ShowAttendTellModel(28, 16, 101, 12, None, feature_size=(9, 16), compute_dtype="f32", vgg_cfg=[8, "M", 16])
    with pytest.raises(ValueError, match="steps"):
        att.sample_stochastic_features(torch.zeros(2, 9, 16), steps=0)
    with pytest.raises(ValueError, match="states"):
        att.sample_stochastic_features(torch.zeros(2, 9, 16), states=(torch.zeros(3, 28), torch.zeros(3, 28)))


def test_c_entry_points_check_arguments_before_any_launch():
    import ctypes as C
    lib = L.load()
    fake = C.c_void_p(4096)                     # never dereferenced: every check below fails first
    need = lib.sat_sample_filtered_ws_bytes(3, 100)

    def call(**kw):
        a = dict(logits=fake, ldl=100, R=3, V=100, tau=1.0, k=0, p=1.0, seed=7, t=0, rank=0, ids=fake, stride=1, logp=None, kept=None,
                 ws=fake, wsb=need)
        a.update(kw)
        return lib.sat_sample_filtered(a["logits"], a["ldl"], a["R"], a["V"], a["tau"], a["k"], a["p"], a["seed"], a["t"], a["rank"],
                                       a["ids"], a["stride"], a["logp"], a["kept"], a["ws"], a["wsb"], None)

    for bad in (dict(logits=None), dict(ids=None), dict(ws=None), dict(R=0), dict(V=0), dict(ldl=99), dict(tau=0.0), dict(tau=-1.0),
                dict(tau=float("inf")), dict(tau=float("nan")), dict(k=-1), dict(p=0.0), dict(p=1.5), dict(p=float("nan")), dict(t=-1),
                dict(rank=-1)):
        assert call(**bad) == 1001, bad
    assert call(wsb=need - 1) == 1002
    assert call(V=32769, ldl=32769) == 1003


def test_decode_entry_points_share_their_argument_check():
    """`sat_greedy_decode` and `sat_sample_decode` refuse, before any HIP call: a null entry of lstm_w, num_layers outside 1..8,
    steps < 1 and an ids row shorter than the steps"""
    import ctypes as C
    lib = L.load()
    fake = C.c_void_p(4096)                     # never dereferenced: every check below fails first
    B, E, H, V = 3, 8, 16, 100
    full = [4096] * 36                          # room for the nine layers a bad num_layers asks for

    def calls(lstm_w=full, num_layers=2, steps=4, ids_stride=4):
        w = (C.c_void_p * len(lstm_w))(*lstm_w)
        common = (fake, fake, w, num_layers, fake, fake, B, E, H, V, steps)
        state = (fake, fake, fake, fake, fake, ids_stride)
        return (lib.sat_greedy_decode(*common, *state, fake, 1 << 30, None),
                lib.sat_sample_decode(*common, 1.0, 0, 1.0, 7, 0, *state, None, None, None, 0, fake, 1 << 30, None))

    for hole in (0, 3, 5, 7):
        assert calls(lstm_w=full[:hole] + [None] + full[hole + 1:]) == (1001, 1001), hole
    for bad in (dict(num_layers=0), dict(num_layers=9), dict(steps=0), dict(steps=-1), dict(ids_stride=3)):
        assert calls(**bad) == (1001, 1001), bad
