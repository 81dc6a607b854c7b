"""Averaged weights on the MI355X: sat_ema_update and sat_swap_f32 against tests/ema_reference.py bit for bit, the paths that must
leave the average untouched, and the feature through TrainStep and FusedClampAdam.

Every comparison is on bits.  The one slack is ema_reference's: where the float64 value of the reference sits on a float32 midpoint
either neighbour passes.  No fault is provoked: the skip word and the {norm, non-finite} pair are written by hand."""
import importlib

import numpy as np
import pytest
import torch

import ema_reference as E

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

pytestmark = pytest.mark.gpu

GUARD = 64
INF, NAN = float("inf"), float("nan")
OFFSETS = (0, 4, 1028)                      # elements: FusedClampAdam addresses segments at base + 4 a bytes, a % 4 == 0
_CASES = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    return L.load()


def bits(t):
    return t.detach().contiguous().view(-1).cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def case(n, decay):
    """(e, p, expected, other) of one sweep case, computed once and never modified"""
    if (n, decay) not in _CASES:
        e, p = E.sweep_inputs(n, decay)
        _CASES[(n, decay)] = (e, p) + E.ema_step(e, p, decay)
    return _CASES[(n, decay)]


def pattern(count, seed):
    """a recognisable filler for guards and untouched buffers: finite, no two neighbours equal"""
    return (np.arange(count, dtype=np.float32) * np.float32(0.37) + np.float32(seed)).astype(np.float32)


def framed(values, offset, seed):
    """device buffer [GUARD | offset | values | GUARD] (its base is 16-byte aligned; offset % 4 == 0), host copy, start index"""
    n = len(values)
    host = pattern(GUARD + offset + n + GUARD, seed)
    lo = GUARD + offset
    host[lo:lo + n] = values
    return torch.from_numpy(host.copy()).cuda(), host, lo


def ema_call(lib, e_dev, lo_e, p_dev, lo_p, n, decay, skip=None, norm=None):
    L.check(lib.sat_ema_update(e_dev.data_ptr() + 4 * lo_e, p_dev.data_ptr() + 4 * lo_p, n, decay, L.ptr(skip), L.ptr(norm), L.stream()),
            "sat_ema_update")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- A. the kernels

@pytest.mark.parametrize("decay", E.SWEEP_DECAY)
@pytest.mark.parametrize("n", E.SWEEP_N)
def test_ema_update_equals_the_reference_bit_for_bit(lib, n, decay):
    e, p, expected, other = case(n, decay)
    results = []
    for offset in OFFSETS:
        e_dev, e_host, lo = framed(e, offset, 11.0)
        p_dev, p_host, lo_p = framed(p, offset, 23.0)
        ema_call(lib, e_dev, lo, p_dev, lo_p, n, decay)
        got = e_dev.cpu().numpy()
        ok = E.matches(got[lo:lo + n], expected, other)
        assert ok.all(), "offset %d: %d of %d elements differ, first at %d" % (offset, (~ok).sum(), n, int(np.argmin(ok)))
        assert np.array_equal(got[:lo].view(np.uint32), e_host[:lo].view(np.uint32)), "guard in front"
        assert np.array_equal(got[lo + n:].view(np.uint32), e_host[lo + n:].view(np.uint32)), "guard behind"
        assert np.array_equal(bits(p_dev), p_host.view(np.uint32)), "the parameters are only read"
        results.append(got[lo:lo + n].view(np.uint32).copy())
    for r in results[1:]:
        assert np.array_equal(r, results[0]), "the same data at another pointer offset gives the same bits"


def test_an_element_has_the_same_bits_under_every_n(lib):
    """the 16-byte loop, the scalar tail and the second grid-stride trip agree: the first 1023 elements of the largest case,
    computed again as a case of 1023 (tail of 3), of 1021 (tail of 1) and of 1020 (no tail)"""
    n, decay = E.SWEEP_N[-1], 0.9999
    e, p, _, _ = case(n, decay)
    e_dev, _, lo = framed(e, 0, 11.0)
    p_dev, _, lo_p = framed(p, 0, 23.0)
    ema_call(lib, e_dev, lo, p_dev, lo_p, n, decay)
    whole = bits(e_dev)[lo:lo + n]
    for m in (1023, 1021, 1020, 3):
        e_dev, _, lo = framed(e[:m], 0, 11.0)
        ema_call(lib, e_dev, lo, p_dev, lo_p, m, decay)
        assert np.array_equal(bits(e_dev)[lo:lo + m], whole[:m]), m
    # the last five -- there the chunk of a second grid-stride trip and the tail -- as a case of their own
    e_dev, _, lo = framed(e[n - 5:], 0, 11.0)
    p_last, _, lo_p = framed(p[n - 5:], 0, 23.0)
    ema_call(lib, e_dev, lo, p_last, lo_p, 5, decay)
    assert np.array_equal(bits(e_dev)[lo:lo + 5], whole[n - 5:])


SKIPS = [("skip word", 3.0, None, False), ("non-finite count", 0.0, (1.0, 1.0), False), ("inf norm", 0.0, (INF, 0.0), False),
         ("nan norm", 0.0, (NAN, 0.0), False), ("negative-zero word, clean norm", -0.0, (3.0, 0.0), True),
         ("zero word, clean norm", 0.0, (3.0, 0.0), True), ("skip word and clean norm", 1.0, (3.0, 0.0), False),
         ("no word, non-finite count", None, (0.5, 2.0), False), ("neither", None, None, True)]


@pytest.mark.parametrize("n", [5, 786437])
@pytest.mark.parametrize("what,word,norm,updated", SKIPS, ids=[s[0] for s in SKIPS])
def test_a_dropped_update_leaves_the_average_untouched(lib, n, what, word, norm, updated):
    e, p, expected, other = case(n, 0.999)
    e_dev, e_host, lo = framed(e, 4, 11.0)
    p_dev, _, lo_p = framed(p, 4, 23.0)
    skip = None if word is None else torch.full((1,), word, device="cuda")
    state = None if norm is None else torch.tensor(norm, dtype=torch.float64, device="cuda")
    ema_call(lib, e_dev, lo, p_dev, lo_p, n, 0.999, skip, state)
    got = e_dev.cpu().numpy()
    if updated:
        assert E.matches(got[lo:lo + n], expected, other).all()
        assert not np.array_equal(got[lo:lo + n].view(np.uint32), e.view(np.uint32))
        got[lo:lo + n] = e                                   # (the guards are compared below)
    assert np.array_equal(got.view(np.uint32), e_host.view(np.uint32)), what
    if state is not None:
        assert np.array_equal(state.cpu().numpy().view(np.uint64), np.array(norm, dtype=np.float64).view(np.uint64)), "only read"


@pytest.mark.parametrize("n", E.SWEEP_N)
def test_swap_is_exact_and_twice_is_the_identity(lib, n):
    e, p, _, _ = case(n, 0.9999)                             # the wide-range values: both signs, 1e-30 .. 1e30
    for offset in (0, 4):
        a_dev, a_host, lo = framed(e, offset, 11.0)
        b_dev, b_host, lo_b = framed(p, 0, 23.0)
        once_a, once_b = a_host.copy(), b_host.copy()
        once_a[lo:lo + n], once_b[lo_b:lo_b + n] = p, e
        for expect_a, expect_b in ((once_a, once_b), (a_host, b_host)):
            L.check(lib.sat_swap_f32(a_dev.data_ptr() + 4 * lo, b_dev.data_ptr() + 4 * lo_b, n, L.stream()), "sat_swap_f32")
            torch.cuda.synchronize()
            assert np.array_equal(bits(a_dev), expect_a.view(np.uint32)) and np.array_equal(bits(b_dev), expect_b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- B. TrainStep

SMOKE = dict(E=32, H=64, V=200, L=1, B=4, T=10)            # the smallest model test_gpu_optim.py builds


def smoke_model(seed=1):
    torch.manual_seed(seed)
    return sat.ShowAndTell(SMOKE["E"], SMOKE["H"], SMOKE["V"], SMOKE["L"], arch=dict(layers=(1, 1, 1, 1), width=8),
                           compute_dtype="f32").cuda().train()


def smoke_batch():
    g = torch.Generator().manual_seed(1)
    images = torch.randn(SMOKE["B"], 3, 64, 64, generator=g)
    caps = torch.randint(4, SMOKE["V"], (SMOKE["B"], SMOKE["T"]), generator=g)
    caps[:, 0], caps[:, -1] = 1, 2
    return images.cuda(), caps.cuda(), [SMOKE["T"]] * SMOKE["B"]


def host(t):
    return t.detach().cpu().numpy().copy()


def steps(ts, k):
    """k steps; the parameters after each"""
    out = []
    for _ in range(k):
        ts.step(*smoke_batch())
        torch.cuda.synchronize()
        out.append(host(ts.flat.params))
    return out


def plain_run():
    """the parameters after each of four steps of an engine with the feature off, computed once"""
    if "plain" not in _CASES:
        ts = sat.TrainStep(smoke_model())
        _CASES["plain"] = steps(ts, 4)
        assert ts.flat.ema is None and "ema" not in ts.optimizer_state_dict()
    return _CASES["plain"]


def check_recursion(start, snaps, emas, decays, tag=""):
    """the reference recursion from `start` over the parameter snapshots, against the average seen after each step.  Each step is
    taken from the average the device holds, so a midpoint at which it took the other neighbour does not carry into later steps"""
    e = start
    for k, (got, snap, d) in enumerate(zip(emas, snaps, decays), 1):
        expected, other = E.ema_step(e, snap, d)
        assert E.matches(got, expected, other).all(), "%s step %d" % (tag, k)
        e = got


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
def test_train_step_average_equals_the_reference_recursion_and_does_not_disturb_training(warmup):
    ts = sat.TrainStep(smoke_model())
    assert ts.flat.ema is None
    ts.ema_decay, ts.ema_warmup = 0.9, warmup
    start = host(ts.flat.params)
    assert same_bits(ts.flat.ema, ts.flat.params) and ts.flat.ema.data_ptr() != ts.flat.params.data_ptr()
    snaps, emas = [], []
    for _ in range(3):
        snaps += steps(ts, 1)
        emas.append(host(ts.flat.ema))
    decays = [2 / 11, 3 / 12, 4 / 13] if warmup else [0.9] * 3
    assert [sat.ema_decay_at(0.9, t, warmup) for t in (1, 2, 3)] == decays
    check_recursion(start, snaps, emas, decays)
    assert not np.array_equal(emas[0].view(np.uint32), start.view(np.uint32))
    for a, b in zip(snaps, plain_run()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the average must not disturb training"


def test_train_step_drops_the_average_with_a_non_finite_gradient():
    images, caps, lengths = smoke_batch()
    ts = sat.TrainStep(smoke_model())
    ts.ema_decay, ts.max_grad_norm = 0.9, 1.0
    ts.step(images, caps, lengths)
    ts.forward_backward((images, caps, lengths), 1.0 / sum(l - 1 for l in lengths))
    ts.flat.grads[11] = INF                                  # a value in the gradient buffer, between backward and the update
    f = ts.flat
    before = [t.clone() for t in (f.params, f.m, f.v, f.ema)]
    assert not same_bits(f.ema, f.params), "the first step moved both"
    ts.optimizer_step()
    torch.cuda.synchronize()
    assert all(same_bits(t, was) for t, was in zip((f.params, f.m, f.v, f.ema), before))
    assert ts.last_grad_norm[1].item() > 0 and ts.step_count == 2
    ts.step(images, caps, lengths)
    torch.cuda.synchronize()
    assert ts.last_grad_norm[1].item() == 0.0
    assert not any(same_bits(t, was) for t, was in zip((f.params, f.m, f.v, f.ema), before))


def test_train_step_drops_the_average_behind_a_set_fault_word():
    """the word is written by hand behind the backward, as the step's fault flag would; nothing faults"""
    images, caps, lengths = smoke_batch()
    ts = sat.TrainStep(smoke_model())
    ts.ema_decay = 0.9
    ts.step(images, caps, lengths)
    ts.forward_backward((images, caps, lengths), 1.0 / sum(l - 1 for l in lengths))
    f = ts.flat
    e_before, p_before = f.ema.clone(), f.params.clone()
    p_host, e_host = host(f.params), host(f.ema)
    ema_call(ts.lib, f.ema, 0, f.params, 0, f.n, 0.9, skip=torch.ones(1, device="cuda"))
    assert same_bits(f.ema, e_before) and same_bits(f.params, p_before)
    ema_call(ts.lib, f.ema, 0, f.params, 0, f.n, 0.9, skip=ts.fault_slot)
    assert ts.fault_slot.item() == 0.0 and E.matches(host(f.ema), *E.ema_step(e_host, p_host, 0.9)).all()


def test_averaged_weights_block_and_averaged_state_dict():
    images, caps, lengths = smoke_batch()
    ts = sat.TrainStep(smoke_model())
    with pytest.raises(RuntimeError, match="ema_decay has never been set"):
        with ts.averaged_weights():
            pass
    ts.ema_decay = 0.9
    steps(ts, 3)
    f, model = ts.flat, ts.model
    live, avg = f.params.clone(), f.ema.clone()
    assert not same_bits(live, avg)
    versions = [p._version for p in ts._params_list]
    sd = ts.averaged_state_dict()
    model_sd = model.state_dict()
    assert list(sd) == list(model_sd)
    trainable = [name for name, _ in ts._trainable()]
    assert set(trainable) == set(f.slices) and any(k.endswith("num_batches_tracked") for k in sd)
    for name in trainable:
        o, n, shape = f.slices[name]
        assert same_bits(sd[name], avg[o:o + n].view(shape)) and sd[name].data_ptr() != f.ema[o:o + n].data_ptr(), name
    for name in set(sd) - set(trainable):                    # frozen conv weights, BatchNorm buffers, num_batches_tracked
        assert torch.equal(sd[name], model_sd[name]) and sd[name].data_ptr() != model_sd[name].data_ptr(), name
    with ts.averaged_weights() as inside:
        assert inside is ts
        torch.cuda.synchronize()
        assert same_bits(f.params, avg) and same_bits(f.ema, live)
        for name, p in ts._trainable():
            o, n, shape = f.slices[name]
            assert same_bits(p.data, avg[o:o + n].view(shape)), name
        assert all(p._version > v for p, v in zip(ts._params_list, versions))
        ids = model.eval().sample(images, None)
        model.train()
        inner = ts.averaged_state_dict()
        assert all(same_bits(inner[k], sd[k]) for k in sd), "the same dict from inside the block"
        for call in (ts.optimizer_step, lambda: ts.step(images, caps, lengths), lambda: ts.forward_backward((images, caps, lengths), 0.1),
                     lambda: ts.scst_step(images, None, None), lambda: ts.averaged_weights().__enter__()):
            with pytest.raises(RuntimeError, match="averaged"):
                call()
        inside_versions = [p._version for p in ts._params_list]
    torch.cuda.synchronize()
    assert same_bits(f.params, live) and same_bits(f.ema, avg)
    assert all(p._version > v for p, v in zip(ts._params_list, inside_versions))
    fresh = smoke_model(seed=7)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.eval().sample(images, None), ids)
    live_ids = model.eval().sample(images, None)
    model.train()
    print("ids that differ between the live and the averaged weights: %d of %d" % ((live_ids != ids).sum().item(), ids.numel()))
    # an exception inside the block still swaps back
    with pytest.raises(KeyError):
        with ts.averaged_weights():
            raise KeyError("x")
    torch.cuda.synchronize()
    assert same_bits(f.params, live) and same_bits(f.ema, avg) and ts._averaged is False
    # one more step: the bits of a run that never entered the block
    after = steps(ts, 1)[0]
    assert np.array_equal(after.view(np.uint32), plain_run()[3].view(np.uint32))
    assert E.matches(host(f.ema), *E.ema_step(host(avg), after, 0.9)).all()


def test_zero_stops_the_updates_and_keeps_the_buffer_and_reset_copies():
    ts = sat.TrainStep(smoke_model())
    ts.ema_decay = 0.9
    steps(ts, 1)
    kept = ts.flat.ema.clone()
    ts.ema_decay = 0.0
    steps(ts, 1)
    assert same_bits(ts.flat.ema, kept) and "ema" in ts.optimizer_state_dict()
    ts.ema_decay = 0.5                                       # on again: the buffer is not copied anew
    assert same_bits(ts.flat.ema, kept)
    ts.reset_ema()
    assert same_bits(ts.flat.ema, ts.flat.params)


def test_checkpoint_round_trip_resumes_with_the_same_bits():
    ts = sat.TrainStep(smoke_model())
    ts.ema_decay, ts.ema_warmup = 0.9, True
    steps(ts, 2)
    osd = ts.optimizer_state_dict()
    msd = {k: v.detach().clone() for k, v in ts.model.state_dict().items()}
    assert osd["ema"]["decay"] == 0.9 and osd["ema"]["warmup"] is True and len(osd["ema"]["params"]) == len(osd["param_names"])
    steps(ts, 2)
    model = smoke_model(seed=9)
    model.load_state_dict(msd)
    other = sat.TrainStep(model)
    assert other.flat.ema is None
    other.load_optimizer_state_dict(osd)
    assert other.ema_decay == 0.9 and other.ema_warmup is True and other.step_count == 2
    steps(other, 2)
    assert same_bits(other.flat.params, ts.flat.params) and same_bits(other.flat.ema, ts.flat.ema)
    bad = dict(osd, ema=dict(osd["ema"], params=osd["ema"]["params"][:-1]))
    with pytest.raises(ValueError, match="averaged weights hold"):
        other.load_optimizer_state_dict(bad)


# ---------------------------------------------------------------------------------------------- C. FusedClampAdam

def four_tensors(seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in ((5, 3), (7,), (4, 4), (9,))]


def adam_steps(opt, ps, k, idle=2, emas=None):
    """k steps of a loss that parameter `idle` takes no part in: its gradient is None at every step(); the parameters after each
    step (and the averages, into `emas`)"""
    g = torch.Generator().manual_seed(6)
    out = []
    for _ in range(k):
        opt.zero_grad()
        loss = sum((p * torch.randn(p.shape, generator=g).cuda()).sum() + (p * p).sum() for i, p in enumerate(ps) if i != idle)
        loss.backward()
        ps[idle].grad = None
        opt.step()
        torch.cuda.synchronize()
        out.append([host(p) for p in ps])
        if emas is not None:
            emas.append([host(t) for t in opt.ema_params()])
    return out


@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["plain", "max_norm"])
def test_fused_clamp_adam_average(max_norm):
    ps = four_tensors()
    opt = sat.FusedClampAdam(ps, lr=1e-2, clip=0.1, max_norm=max_norm)
    assert opt.ema is None and "ema" not in opt.state_dict()
    with pytest.raises(RuntimeError, match="ema_decay has never been set"):
        with opt.averaged_weights():
            pass
    opt.ema_decay = 0.9
    start = [host(p) for p in ps]
    assert all(same_bits(a, p.data) for a, p in zip(opt.ema_params(), ps))
    emas = []
    snaps = adam_steps(opt, ps, 3, emas=emas)
    got = emas[-1]
    assert [tuple(t.shape) for t in opt.ema_params()] == [tuple(p.shape) for p in ps]
    for i in range(4):
        check_recursion(start[i], [s[i] for s in snaps], [e[i] for e in emas], [0.9] * 3, "parameter %d" % i)
        assert (i == 2) == np.array_equal(got[i].view(np.uint32), start[i].view(np.uint32))
    assert same_bits(opt.ema_params()[2], ps[2].data), "without a gradient neither the parameter nor its average moves"
    if max_norm is not None:
        assert opt.last_grad_norm[1].item() == 0.0
    # the same training with the feature off
    qs = four_tensors()
    plain = sat.FusedClampAdam(qs, lr=1e-2, clip=0.1, max_norm=max_norm)
    adam_steps(plain, qs, 3)
    assert all(same_bits(p.data, q.data) for p, q in zip(ps, qs)) and plain.ema is None
    # the block
    live, avg = opt.flat.clone(), opt.ema.clone()
    with opt.averaged_weights():
        torch.cuda.synchronize()
        assert same_bits(opt.flat, avg) and all(np.array_equal(bits(p.data), g.view(np.uint32).ravel()) for p, g in zip(ps, got))
        assert all(same_bits(a, p.data) for a, p in zip(opt.ema_params(), ps)), "ema_params() stay the averaged ones inside"
        with pytest.raises(RuntimeError, match="averaged"):
            opt.step()
        with pytest.raises(RuntimeError, match="averaged"):
            opt.reset_ema()
        with pytest.raises(RuntimeError, match="nest"):
            opt.averaged_weights().__enter__()
    torch.cuda.synchronize()
    assert same_bits(opt.flat, live) and same_bits(opt.ema, avg)
    # state dict round trip
    sd = opt.state_dict()
    assert sd["ema"]["decay"] == 0.9 and sd["ema"]["warmup"] is False
    rs = four_tensors(seed=5)
    other = sat.FusedClampAdam(rs, lr=1e-2, clip=0.1, max_norm=max_norm)
    other.load_state_dict(sd)
    assert other.ema_decay == 0.9 and other.step_count == 3 and all(same_bits(a, b) for a, b in zip(other.ema_params(), opt.ema_params()))
    plain.load_state_dict(plain.state_dict())
    assert plain.ema is None and plain.ema_decay == 0.0
    opt.reset_ema()
    assert same_bits(opt.ema, opt.flat) and opt.ema.data_ptr() != opt.flat.data_ptr()


def test_fused_clamp_adam_drops_the_average_with_a_non_finite_gradient():
    ps = four_tensors()
    opt = sat.FusedClampAdam(ps, lr=1e-2, max_norm=0.5)
    opt.ema_decay, opt.ema_warmup = 0.999, True
    adam_steps(opt, ps, 1, idle=3)
    opt.zero_grad()
    sum((p * p).sum() for p in ps).backward()
    ps[0].grad[0, 0] = NAN
    before = [t.clone() for t in (opt.flat, opt.exp_avg, opt.ema)]
    opt.step()
    torch.cuda.synchronize()
    assert all(same_bits(t, was) for t, was in zip((opt.flat, opt.exp_avg, opt.ema), before)) and opt.last_grad_norm[1].item() == 1.0
