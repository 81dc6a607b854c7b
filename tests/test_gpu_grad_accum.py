"""Gradient accumulation on the MI355X: sat_grad_accumulate through the C ABI against tests/grad_accum_reference.py, and the feature
through TrainStep (`accumulate`, `optimizer_step` on the accumulated buffer, `step_accumulated`, `mixed_step`).

Kernel sizes (grad_accum_reference.SIZES; the launcher runs 256 threads of 16-byte accesses, at most 768 workgroups, over the n + 1
gradient-rule elements): n = 1, 3, 4, 5; 1022 / 1023 / 1024 / 1025 / 1027 around one workgroup's span of 1024 elements (n + 1 one short
of it, exactly it, one and two past it, and the first chunk of a second workgroup); 787461 = one sweep of the whole grid (786432)
plus a workgroup's span plus a tail, where the grid-stride loop wraps.

No fault is provoked: where a drop is tested the fault word and the Inf are written into a tensor by hand.  The last test runs
`DataParallelStep.step_accumulated` over the real engine with two processes on the one device (gloo, as tests/test_gpu_dp.py)."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ema_reference as E
import grad_accum_reference as A
import optim_reference as O
from oracle import decoder as OD

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

pytestmark = pytest.mark.gpu

GUARD = 64
INF, NAN = float("inf"), float("nan")
_CASES = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    return L.load()


def bits(t):
    return t.detach().contiguous().view(-1).cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def case(n, k=5):
    """k gradient buffers of n + 2 floats, computed once and never modified"""
    if (n, k) not in _CASES:
        _CASES[(n, k)] = A.inputs(n, k)
    return _CASES[(n, k)]


def pattern(count, seed):
    return (np.arange(count, dtype=np.float32) * np.float32(0.37) + np.float32(seed)).astype(np.float32)


def framed(values, seed):
    """device buffer [GUARD | values | GUARD] (the values start 16-byte aligned), its host copy, the start index"""
    host = pattern(GUARD + len(values) + GUARD, seed)
    host[GUARD:GUARD + len(values)] = values
    return torch.from_numpy(host.copy()).cuda(), host, GUARD


def fold(lib, acc_dev, g_dev, n, weight, first):
    L.check(lib.sat_grad_accumulate(acc_dev.data_ptr() + 4 * GUARD, g_dev.data_ptr() + 4 * GUARD, n, weight, first, L.stream()),
            "sat_grad_accumulate")
    torch.cuda.synchronize()


def check_frames(acc_dev, acc_host, g_dev, g_host, n):
    got = acc_dev.cpu().numpy()
    assert np.array_equal(u32(got[:GUARD]), u32(acc_host[:GUARD])), "sentinels in front of acc"
    assert np.array_equal(u32(got[GUARD + n + 2:]), u32(acc_host[GUARD + n + 2:])), "sentinels behind n + 2"
    assert np.array_equal(bits(g_dev), u32(g_host)), "g and its sentinels are only read"
    return got[GUARD:GUARD + n + 2]


# ---------------------------------------------------------------------------------------------- A. the kernel

@pytest.mark.parametrize("n", A.SIZES)
def test_first_fold_with_weight_one_is_a_copy_over_stale_nan(lib, n):
    g = case(n)[0]
    acc_dev, acc_host, _ = framed(np.full(n + 2, NAN, np.float32), 11.0)
    g_dev, g_host, _ = framed(g, 23.0)
    fold(lib, acc_dev, g_dev, n, 1.0, 1)
    got = check_frames(acc_dev, acc_host, g_dev, g_host, n)
    assert np.array_equal(u32(got[:n + 1]), u32(g[:n + 1])), "gradients and loss slot: a copy, bit for bit"
    assert got[n + 1] == 0.0, "the stale fault word (NaN) is not read by a first fold"


@pytest.mark.parametrize("n", A.SIZES)
def test_two_folds_with_weight_one_are_the_float32_sum(lib, n):
    a, g = case(n)[:2]
    acc_dev, acc_host, _ = framed(np.full(n + 2, NAN, np.float32), 11.0)
    a_dev, a_host, _ = framed(a, 17.0)
    g_dev, g_host, _ = framed(g, 23.0)
    fold(lib, acc_dev, a_dev, n, 1.0, 1)
    fold(lib, acc_dev, g_dev, n, 1.0, 0)
    got = check_frames(acc_dev, acc_host, g_dev, g_host, n)
    assert np.array_equal(u32(got[:n + 1]), u32(a[:n + 1] + g[:n + 1])), "numpy's float32 a + g, loss slot included"
    assert got[n + 1] == 0.0 and np.array_equal(bits(a_dev), u32(a_host))


@pytest.mark.parametrize("n", A.SIZES)
def test_two_halves_of_the_same_gradient_return_it(lib, n):
    g = case(n)[0]
    acc_dev, acc_host, _ = framed(np.full(n + 2, NAN, np.float32), 11.0)
    g_dev, g_host, _ = framed(g, 23.0)
    fold(lib, acc_dev, g_dev, n, 0.5, 1)
    fold(lib, acc_dev, g_dev, n, 0.5, 0)
    got = check_frames(acc_dev, acc_host, g_dev, g_host, n)
    assert np.array_equal(u32(got[:n + 1]), u32(g[:n + 1]))


WEIGHTS = [0.3, -1.7, 1.0, 0.125, 2.5]


@pytest.mark.parametrize("n", A.SIZES)
def test_five_folds_with_general_weights(lib, n):
    """against the float64 sum within the derived bound K * 2^-24 * sum_k |w_k g_k| + one ulp of the result, and every fold against
    the reference's one-rounding fma bit for bit (either neighbour where the float64 value sits on a float32 midpoint)"""
    gs = case(n)
    acc_dev, acc_host, _ = framed(np.full(n + 2, NAN, np.float32), 11.0)
    acc = None
    for k, (g, w) in enumerate(zip(gs, WEIGHTS)):
        g_dev, g_host, _ = framed(g, 23.0)
        fold(lib, acc_dev, g_dev, n, w, 1 if k == 0 else 0)
        got = check_frames(acc_dev, acc_host, g_dev, g_host, n)
        expected, other = A.fold(acc, g, w, k == 0)
        ok = A.matches(got, expected, other)
        assert ok.all(), "fold %d: %d of %d elements differ, first at %d" % (k, (~ok).sum(), n + 2, int(np.argmin(ok)))
        acc = got.copy()                                   # (a midpoint at which the device took the other neighbour does not carry)
    total, abs_sum = A.sum_f64(gs, WEIGHTS)
    err = np.abs(acc[:n + 1].astype(np.float64) - total)
    limit = A.bound(len(gs), abs_sum, acc[:n + 1])
    print("n %d: worst error / bound %.3g, loss slot error %.3g (bound %.3g)" % (n, (err / limit).max(), err[n], limit[n]))
    assert (err <= limit).all()
    assert err[n] <= limit[n], "the loss slot follows the gradient rule"


def test_an_element_has_the_same_bits_under_every_launch_shape(lib):
    """the first 1020 gradients of the largest case (768 workgroups, two trips) folded again as cases of 1023 (one workgroup, no
    tail beyond the loss slot), 1021 and 1020 gradients: the 16-byte loop, the tail and the grid do not show in the bits"""
    n = A.SIZES[-1]
    gs = case(n)

    def run(m):
        acc_dev, _, _ = framed(np.full(m + 2, NAN, np.float32), 11.0)
        for k, (g, w) in enumerate(zip(gs, WEIGHTS)):
            g_dev, _, _ = framed(np.concatenate([g[:m], g[n:]]), 23.0)
            fold(lib, acc_dev, g_dev, m, w, 1 if k == 0 else 0)
        return acc_dev.cpu().numpy()[GUARD:GUARD + m + 2]
    whole = run(n)
    for m in (1023, 1021, 1020, 5, 3):
        part = run(m)
        assert np.array_equal(u32(part[:m]), u32(whole[:m])), m
        assert np.array_equal(u32(part[m:]), u32(whole[n:])), "loss slot and fault word, wherever they lie"


@pytest.mark.parametrize("n", [5, A.SIZES[-1]])
@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("acc_word", [0.0, 1.0])
@pytest.mark.parametrize("g_word", [0.0, 1.0])
def test_fault_word_is_the_or_of_what_was_folded(lib, n, first, acc_word, g_word):
    a, g = (x.copy() for x in case(n)[:2])
    a[n + 1], g[n + 1] = acc_word, g_word
    acc_dev, acc_host, _ = framed(a, 11.0)
    g_dev, g_host, _ = framed(g, 23.0)
    fold(lib, acc_dev, g_dev, n, 1.0, first)
    got = check_frames(acc_dev, acc_host, g_dev, g_host, n)
    want = 1.0 if (g_word != 0 or (acc_word != 0 and not first)) else 0.0
    assert got[n + 1] == want and A.fault(bool(first), acc_word, g_word) == want


def test_fault_word_other_non_zero_values_and_negative_zero(lib):
    """an all-reduced word may hold 2.0; -0.0 is zero; the result is always exactly 0.0 or 1.0"""
    n = 5
    for acc_word, g_word, want in ((2.0, 0.0, 1.0), (0.0, 3.0, 1.0), (-0.0, -0.0, 0.0), (0.0, 1e-30, 1.0)):
        a, g = (x.copy() for x in case(n)[:2])
        a[n + 1], g[n + 1] = acc_word, g_word
        acc_dev, acc_host, _ = framed(a, 11.0)
        g_dev, g_host, _ = framed(g, 23.0)
        fold(lib, acc_dev, g_dev, n, 1.0, 0)
        got = check_frames(acc_dev, acc_host, g_dev, g_host, n)
        assert u32(got[n + 1:])[0] == u32([want])[0], (acc_word, g_word)


def test_non_finite_values_go_through_the_fma(lib):
    n = 9
    a, g = (x.copy() for x in case(n)[:2])
    a[2], g[3], g[4], a[4] = INF, NAN, INF, -INF
    acc_dev, _, _ = framed(a, 11.0)
    g_dev, _, _ = framed(g, 23.0)
    fold(lib, acc_dev, g_dev, n, 1.0, 0)
    got = acc_dev.cpu().numpy()[GUARD:GUARD + n + 2]
    assert got[2] == INF and np.isnan(got[3]) and np.isnan(got[4]) and np.isfinite(got[[0, 1, 5, 6, 7, 8, 9]]).all()


# ---------------------------------------------------------------------------------------------- B. TrainStep

TINY = dict(layers=(1, 1, 1, 1), width=8)
DIM = dict(E=32, H=32, V=53, L=1)
LENGTHS = [9, 8, 7, 5, 4, 3]                 # whole captions, <start> included: 30 target tokens
IDX = [0, 1, 2, 3, 1, 0]
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def dec_params():
    return OD.init_decoder_params(DIM["E"], DIM["H"], DIM["V"], DIM["L"], generator=torch.Generator().manual_seed(4))


def engine():
    """a TrainStep over a tiny ShowAndTell in the f32 decoder mode; the batches below are cached [B, E] features, so no BatchNorm
    lies in the path"""
    torch.manual_seed(1)                                     # (the encoder head's parameters live in the flat buffer too)
    model = sat.ShowAndTell(DIM["E"], DIM["H"], DIM["V"], DIM["L"], arch=TINY, compute_dtype="f32")
    model.decoder.load_state_dict(dec_params())
    ts = sat.TrainStep(model.cuda().train(), lr=HP["lr"], grad_clip=0.1)
    assert ts.decoder_gemm_dtype == "f32" and model.decoder.ss_prob == 0 and ts.flat.acc is None and ts.accumulated == 0
    return ts


def batch():
    if "batch" not in _CASES:
        g = torch.Generator().manual_seed(6)
        B, T = len(LENGTHS), LENGTHS[0]
        caps = torch.zeros(B, T, dtype=torch.long)
        for b, l in enumerate(LENGTHS):
            caps[b, 0] = 1
            caps[b, 1:l - 1] = torch.randint(4, DIM["V"], (l - 2,), generator=g)
            caps[b, l - 1] = 2
        _CASES["batch"] = (torch.randn(B, DIM["E"], generator=g), caps)
    feats, caps = _CASES["batch"]
    return feats.cuda(), caps.cuda(), list(LENGTHS)


def n_tokens():
    return sum(l - 1 for l in LENGTHS)


def state(ts):
    f = ts.flat
    return [t.clone() for t in (f.params, f.m, f.v)]


def plain_step():
    """(parameters, m, v) after one `step` from the common start, computed once"""
    if "plain" not in _CASES:
        ts = engine()
        ts.step(*batch())
        torch.cuda.synchronize()
        _CASES["plain"] = state(ts)
        assert ts.flat.acc is None and ts.accumulated == 0
    return _CASES["plain"]


class Spy:
    """the library object with every call recorded as (name, arguments)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call

    def names(self):
        return [name for name, _ in self.calls]


def test_one_fold_then_the_update_is_the_plain_step_bit_for_bit():
    ts = engine()
    ts.forward_backward(batch(), 1.0 / n_tokens())
    slot = ts.accumulate()
    assert ts.accumulated == 1 and ts.flat.acc.shape == ts.flat.grads.shape and ts.flat.acc.data_ptr() % 16 == 0
    assert same_bits(ts.flat.acc[:ts.flat.n + 2], ts.flat.grads[:ts.flat.n + 2]) and slot.data_ptr() == ts.flat.acc.data_ptr() + 4 * ts.flat.n
    ts.optimizer_step()
    torch.cuda.synchronize()
    assert ts.accumulated == 0 and ts.step_count == 1
    assert all(same_bits(a, b) for a, b in zip(state(ts), plain_step()))


def test_two_halves_of_the_same_batch_are_the_plain_step_bit_for_bit():
    ts = engine()
    for k in range(2):
        ts.forward_backward(batch(), 1.0 / n_tokens())
        ts.accumulate(0.5)
        assert ts.accumulated == k + 1
    ts.optimizer_step()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(state(ts), plain_step())) and ts.step_count == 1


def test_discard_starts_afresh_and_the_buffer_is_not_read():
    ts = engine()
    ts.forward_backward(batch(), 1.0 / n_tokens())
    ts.accumulate(3.0)
    ts.flat.acc.fill_(NAN)
    ts.discard_accumulated()
    assert ts.accumulated == 0
    ts.accumulate()
    ts.optimizer_step()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(state(ts), plain_step()))


def reference_big_batch():
    """float64 torch autograd of the mean CE over the whole batch, and the reference Adam (tests/optim_reference.py) from zero
    moments; computed once"""
    if "big" not in _CASES:
        feats, caps, lengths = (x.cpu() if torch.is_tensor(x) else x for x in batch())
        params = {k: v.double().requires_grad_(True) for k, v in dec_params().items()}
        l1 = [l - 1 for l in lengths]
        logits = OD.decoder_forward(params, feats.double(), caps[:, :-1], l1, DIM["L"])
        loss = torch.nn.functional.cross_entropy(logits, OD.pack_time_major(caps[:, 1:], l1))
        loss.backward()
        out = {}
        for k, p in params.items():
            g = p.grad.reshape(-1)
            new_p, _, m, v, _ = O.adamw_step(p.detach().reshape(-1), g, torch.zeros_like(g), torch.zeros_like(g), 1, 0.1, None, 0.0,
                                             [], **HP)
            out[k] = dict(g=g, p=new_p, m=m, v=v)
        _CASES["big"] = (float(loss.detach()), out)
    return _CASES["big"]


def shards(k=3):
    feats, caps, lengths = batch()
    return [sat.dp_shard(feats, caps, lengths, r, k)[:3] for r in range(k)]


def test_three_micro_batches_against_the_big_batch_in_float64():
    """bounds: those tests/test_gpu_parity.py applies to one step at small sizes -- loss 1e-4, gradients rtol 1e-3 + atol 1e-7,
    parameters 2e-6 absolute"""
    ref_loss, ref = reference_big_batch()
    # the gradients: the folds by hand, read before the update clamps them in place
    man = engine()
    for mb in shards():
        man.forward_backward(mb, 1.0 / n_tokens())
        man.accumulate()
    acc = man.flat.acc.clone()
    ts = engine()
    ts.ema_decay = 0.9
    start = ts.flat.params.cpu().numpy().copy()
    loss = ts.step_accumulated(shards())
    torch.cuda.synchronize()
    assert loss.shape == (1,) and loss.data_ptr() != ts.flat.acc[ts.flat.loss_slot:].data_ptr()
    print("loss %.7f accumulated by hand %.7f float64 %.7f" % (loss.item(), acc[ts.flat.loss_slot].item(), ref_loss))
    assert same_bits(loss, acc[ts.flat.loss_slot:ts.flat.loss_slot + 1]) and abs(loss.item() - ref_loss) < 1e-4
    assert ts.step_count == 1 and ts.accumulated == 0
    assert ts.last_nll.shape == (1,) and abs(ts.last_nll.item() - ref_loss) < 1e-4 and ts.last_ul is None
    worst_g = worst_p = 0.0
    for k, r in ref.items():
        o, n, _ = ts.flat.slices["decoder." + k]
        g = acc[o:o + n].cpu().double()
        worst_g = max(worst_g, float(((g - r["g"]).abs() / (1e-7 + 1e-3 * r["g"].abs())).max()))
        worst_p = max(worst_p, float((ts.flat.params[o:o + n].cpu().double() - r["p"]).abs().max()))
    print("gradient error / (1e-7 + 1e-3 |g|): %.3g; parameter error %.3g (bound 2e-6)" % (worst_g, worst_p))
    for k, r in ref.items():
        o, n, _ = ts.flat.slices["decoder." + k]
        np.testing.assert_allclose(acc[o:o + n].cpu().numpy(), r["g"].numpy(), rtol=1e-3, atol=1e-7, err_msg=k)
        np.testing.assert_allclose(ts.flat.params[o:o + n].cpu().numpy(), r["p"].numpy(), rtol=0, atol=2e-6, err_msg=k)
    # the average moved once, from the start to the one update's parameters
    assert E.matches(ts.flat.ema.cpu().numpy(), *E.ema_step(start, ts.flat.params.cpu().numpy(), 0.9)).all()
    # and the hand-made folds take the same update
    man.optimizer_step()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(state(man), state(ts)))


def test_step_accumulated_sums_nll_and_ul_into_fresh_tensors():
    ts = engine()
    ts.unlikelihood = 0.5
    parts = []
    for mb in shards(2):
        ts.forward_backward(mb, 1.0 / n_tokens())
        parts.append((ts.last_nll.item(), ts.last_ul.item()))
    other = engine()
    other.unlikelihood = 0.5
    other.step_accumulated(shards(2))
    nll, ul = other.last_nll, other.last_ul
    assert nll.shape == (1,) and ul.shape == (1,)
    assert nll.item() == np.float32(np.float32(parts[0][0]) + np.float32(parts[1][0]))
    assert ul.item() == np.float32(np.float32(parts[0][1]) + np.float32(parts[1][1])) and ul.item() > 0
    kept = (nll.item(), ul.item())
    other.forward_backward(shards(2)[0], 1.0 / n_tokens())          # a later call does not write into the sums
    assert (nll.item(), ul.item()) == kept


def tiny_corpus():
    """4 images x 2 references over ids 3..22 (tests/test_gpu_scst.py's)"""
    rng = np.random.Generator(np.random.PCG64(11))
    return [[[int(t) for t in rng.integers(3, 23, rng.integers(4, 9))] for _ in range(2)] for _ in range(4)]


def test_mixed_step_folds_half_of_each_objective():
    scorer = sat.CiderScorer(tiny_corpus())
    feats, caps, lengths = batch()
    # the two gradients on their own, from the same state and seed (the teacher-forced half draws nothing: ss_prob 0, no dropout)
    sep = engine()
    torch.manual_seed(21)
    sep.forward_backward((feats, caps, lengths), 1.0 / n_tokens())
    n = sep.flat.n
    g_xe = sep.flat.grads[:n + 2].cpu().numpy().copy()
    sep.scst_forward_backward(feats, IDX, scorer)
    g_rl = sep.flat.grads[:n + 2].cpu().numpy().copy()
    ids = sep.last_scst.last_ids.clone()
    assert g_xe[n + 1] == 0 and g_rl[n + 1] == 0 and not np.array_equal(g_xe, g_rl)
    ts = engine()
    seen, update = [], ts.optimizer_step

    def recording(lr=None, fixed_lag=None):
        seen.append((ts.accumulated, ts.flat.acc.clone()))
        return update(lr, fixed_lag)
    ts.optimizer_step = recording
    torch.manual_seed(21)
    loss = ts.mixed_step(feats, caps, lengths, IDX, scorer, 0.5)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][0] == 2 and ts.accumulated == 0 and ts.step_count == 1
    assert torch.equal(ts.last_scst.last_ids, ids)
    want = np.float32(0.5) * g_xe[:n + 1] + np.float32(0.5) * g_rl[:n + 1]
    got = seen[0][1].cpu().numpy()
    assert np.array_equal(u32(got[:n + 1]), u32(want)), "0.5 g_xe + 0.5 g_scst, loss slot included, bit for bit"
    assert got[n + 1] == 0.0
    print("mixed loss %.7f = 0.5 * %.7f + 0.5 * %.7f" % (loss.item(), g_xe[n], g_rl[n]))
    assert loss.shape == (1,) and u32([loss.item()])[0] == u32(want[n:])[0]
    assert ts.last_nll.item() == g_xe[n]
    assert not same_bits(ts.flat.params, sep.flat.params)


def recorded(run):
    ts = engine()
    ts.lib = spy = Spy(ts.lib)
    torch.manual_seed(33)
    loss = run(ts)
    torch.cuda.synchronize()
    return ts, spy, loss


def test_mixed_step_at_zero_and_one_is_step_and_scst_step():
    scorer = sat.CiderScorer(tiny_corpus())
    feats, caps, lengths = batch()
    for plain, mixed in ((lambda ts: ts.step(feats, caps, lengths), lambda ts: ts.mixed_step(feats, caps, lengths, IDX, scorer, 0)),
                         (lambda ts: ts.scst_step(feats, IDX, scorer, steps=12),
                          lambda ts: ts.mixed_step(feats, caps, lengths, IDX, scorer, 1.0, steps=12))):
        a, spy_a, loss_a = recorded(plain)
        b, spy_b, loss_b = recorded(mixed)
        assert spy_a.names() == spy_b.names() and "sat_grad_accumulate" not in spy_b.names()
        assert same_bits(loss_a, loss_b) and all(same_bits(x, y) for x, y in zip(state(a), state(b)))
        assert b.flat.acc is None and b.accumulated == 0


def update_calls(spy):
    return [(name, args) for name, args in spy.calls
            if name in ("sat_grad_accumulate", "sat_clamp_adam_step_guarded", "sat_grad_sumsq", "sat_adamw_step", "sat_ema_update")]


@pytest.mark.parametrize("settings", [{}, dict(max_grad_norm=1.0, weight_decay=0.01), dict(ema_decay=0.9)], ids=["adam", "adamw", "ema"])
def test_an_unused_accumulation_changes_no_call_and_an_open_one_swaps_two_pointers(settings):
    """with `accumulated == 0` the update makes the calls it made before the feature, on `flat.grads` and the step's fault word;
    with an open accumulation the SAME calls with `flat.acc` and its word in their places"""
    scorer = sat.CiderScorer(tiny_corpus())
    feats, caps, lengths = batch()

    def configured(run):
        def go(ts):
            for k, v in settings.items():
                setattr(ts, k, v)
            return run(ts)
        return go

    def folded(ts):
        ts.forward_backward((feats, caps, lengths), 1.0 / n_tokens())
        ts.accumulate()
        ts.optimizer_step()
    sequences = []
    for run in (lambda ts: ts.step(feats, caps, lengths), lambda ts: ts.scst_step(feats, IDX, scorer, steps=12), folded):
        ts, spy, _ = recorded(configured(run))
        f = ts.flat
        calls = update_calls(spy)
        open_one = run is folded
        g_ptr = (f.acc if open_one else f.grads).data_ptr()
        word = g_ptr + 4 * (f.n + 1)
        assert (f.acc is not None) == open_one
        names = [name for name, _ in calls]
        assert names[:1] == (["sat_grad_accumulate"] if open_one else names[:1]) and names.count("sat_grad_accumulate") == int(open_one)
        for name, args in calls:
            if name == "sat_clamp_adam_step_guarded":
                assert args[1] == g_ptr and args[11] == word
            elif name == "sat_grad_sumsq":
                assert args[0] == g_ptr and args[1] == f.n
            elif name == "sat_adamw_step":
                assert args[1] == g_ptr and args[18] == word
            elif name == "sat_ema_update":
                assert args[4] == word
        sequences.append([name for name in names if name != "sat_grad_accumulate"])
    want = {"adam": ["sat_clamp_adam_step_guarded"], "adamw": ["sat_grad_sumsq", "sat_adamw_step"],
            "ema": ["sat_clamp_adam_step_guarded", "sat_ema_update"]}["adamw" if "weight_decay" in settings else
                                                                     ("ema" if "ema_decay" in settings else "adam")]
    assert sequences == [want, want, want]


def test_a_set_fault_word_in_the_accumulated_buffer_drops_the_one_update():
    """the word is written by hand behind the fold, as a faulted micro-batch would have left it; nothing faults"""
    ts = engine()
    ts.ema_decay = 0.9
    ts.step(*batch())
    ts.check_ids()
    f = ts.flat
    ts.forward_backward(batch(), 1.0 / n_tokens())
    ts.accumulate()
    assert f.acc[f.n + 1].item() == 0.0
    f.acc[f.n + 1] = 1.0
    before = [t.clone() for t in (f.params, f.m, f.v, f.ema)]
    count = ts.step_count
    persist = ts.lib.sat_lstm_persist_enable(1)
    try:
        ts.optimizer_step()
        torch.cuda.synchronize()
        assert all(same_bits(t, was) for t, was in zip((f.params, f.m, f.v, f.ema), before))
        assert ts.step_count == count + 1 and ts.accumulated == 0 and ts.fault_slot.item() == 0.0
        ts._fault_sticky.zero_()
        with pytest.raises(RuntimeError, match="SKIPPED on the device"):
            ts.check_ids()
        assert ts.step_count == count, "the host rolled the step count back"
        ts.step(*batch())
        ts.check_ids()
        assert ts.step_count == count + 1 and not same_bits(f.params, before[0]) and not same_bits(f.ema, before[3])
    finally:
        ts.lib.sat_lstm_persist_enable(persist)


def test_an_inf_in_the_second_micro_batch_drops_the_one_update():
    ts = engine()
    ts.max_grad_norm, ts.ema_decay = 1.0, 0.9
    ts.step(*batch())
    f = ts.flat
    first, second = shards(2)
    ts.forward_backward(first, 1.0 / n_tokens())
    ts.accumulate()
    ts.forward_backward(second, 1.0 / n_tokens())
    f.grads[7] = INF                                         # a value in the gradient buffer, between backward and the fold
    ts.accumulate()
    before = [t.clone() for t in (f.params, f.m, f.v, f.ema)]
    ts.optimizer_step()
    torch.cuda.synchronize()
    assert all(same_bits(t, was) for t, was in zip((f.params, f.m, f.v, f.ema), before))
    assert ts.last_grad_norm[1].item() > 0 and ts.step_count == 2 and ts.accumulated == 0
    ts.step_accumulated([first, second])
    torch.cuda.synchronize()
    assert ts.last_grad_norm[1].item() == 0.0 and not same_bits(f.params, before[0]) and ts.step_count == 3


def test_entry_points_refuse_inside_averaged_weights_and_on_an_open_accumulation():
    scorer = sat.CiderScorer(tiny_corpus())
    feats, caps, lengths = batch()
    ts = engine()
    ts.ema_decay = 0.9
    ts.forward_backward((feats, caps, lengths), 1.0 / n_tokens())
    with ts.averaged_weights():
        for call in (ts.accumulate, lambda: ts.step_accumulated([(feats, caps, lengths)]),
                     lambda: ts.mixed_step(feats, caps, lengths, IDX, scorer, 0.5)):
            with pytest.raises(RuntimeError, match="averaged"):
                call()
    assert ts.accumulated == 0
    ts.accumulate()
    for call in (lambda: ts.step_accumulated([(feats, caps, lengths)]), lambda: ts.mixed_step(feats, caps, lengths, IDX, scorer, 0.5)):
        with pytest.raises(RuntimeError, match="accumulation is open"):
            call()
    assert ts.accumulated == 1
    with pytest.raises(ValueError, match="length"):
        ts.discard_accumulated()
        ts.step_accumulated([(feats, caps, lengths), (feats, caps, [1] * len(lengths))])
    assert ts.accumulated == 0, "a micro-batch that raises closes the accumulation"


# ---------------------------------------------------------------------------------------------- C. two ranks on the one device

def dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from test_gpu_dp import LENGTHS as DP_LENGTHS, make_batch, make_model
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    feats, caps = make_batch()
    model = make_model(sat)
    ts = sat.TrainStep(model)
    dp = sat.DataParallelStep(ts)
    losses = []
    for _ in range(2):
        f, c, ln, tokens = sat.dp_shard(feats.cuda(), caps.cuda(), DP_LENGTHS, rank, world)
        micro = [sat.dp_shard(f, c, ln, k, 2)[:3] for k in range(2)]
        losses.append(float(dp.step_accumulated(micro, tokens).item()))
    ts.check_ids()
    torch.cuda.synchronize()
    torch.save({"params": {k: v.detach().cpu() for k, v in model.decoder.named_parameters()}, "losses": losses,
                "step_count": ts.step_count, "accumulated": ts.accumulated}, "%s.%d" % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_of_two_micro_batches_on_one_gpu_equal_the_single_process_step(tmp_path):
    """tests/test_gpu_dp.py's comparison and its tolerances (loss 1e-5, parameters 2e-6 absolute after two updates), with every
    rank's shard split once more into two micro-batches and ONE exchange per update"""
    from test_gpu_dp import LENGTHS as DP_LENGTHS, make_batch, make_model
    out = str(tmp_path / "rank")
    port = 35600 + os.getpid() % 2000
    mp.spawn(dp_worker, args=(2, port, out), nprocs=2, join=True)
    got = [torch.load("%s.%d" % (out, r)) for r in range(2)]
    feats, caps = make_batch()
    model = make_model(sat)
    ts = sat.TrainStep(model)
    ref_losses = [float(ts.step(feats.cuda(), caps.cuda(), DP_LENGTHS).item()) for _ in range(2)]
    for g in got:
        assert g["step_count"] == 2 and g["accumulated"] == 0
        for a, b in zip(g["losses"], ref_losses):
            print("loss %.7f single process %.7f" % (a, b))
            assert abs(a - b) < 1e-5
    for k, p in model.decoder.named_parameters():
        assert torch.equal(got[0]["params"][k], got[1]["params"][k]), "the ranks hold the same bits: %s" % k
        np.testing.assert_allclose(got[0]["params"][k].numpy(), p.detach().cpu().numpy(), rtol=0, atol=2e-6, err_msg=k)
