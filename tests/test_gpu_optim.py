"""GPU: global-norm gradient clipping and AdamW weight decay (csrc/sat_optim.hip) through the C ABI, `FusedClampAdam` and `TrainStep`.

A. sat_grad_sumsq.  n = 1, 3 (tail only), 4, 5, 1023, 1024 (one workgroup exactly), 1028 (two), 786432 (768 x 256 chunks: one full
   trip), 786439 (second trip, tail of 3); clip 0 and 0.1; contents randn, magnitudes 1e-30 .. 3e19, zeros, a NaN as the last tail
   element, +Inf at element 0.  Bound: the f32 x f32 products are exact in f64 and an f64 sum of n terms errs by at most n 2^-53
   relative, the kernel's and the reference's alike, so the total of the partials lies within n 2^-52 relative of the reference.  The
   non-finite count is exact, two launches give the same partial bits, the number of pairs is the grid.
B. sat_adamw_step, three steps from non-zero moments at every case of optim_reference.adamw_cases().  p passes within the 2e-7 of
   test_clamp_adam_matches_torch OR p, m, v each within 8 x the frozen float32-restatement error of the case (the rule of
   test_gpu_elementwise_edges.py; its `close`).  The gradient written back is exact where the coefficient is 1 and within two
   roundings (2^-22 relative) where it scales; the norm is bounded as in A (half the total's relative bound, plus the square roots'
   roundings).  Bitwise pins in tests of their own.
C. FusedClampAdam against torch's clip_grad_norm_ + AdamW, TrainStep against the float64 reference on copies of its own buffers, two
   ranks over gloo.
Nothing here is set from a kernel's output."""
import ctypes
import importlib
import math
import os
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import elementwise_reference as R
import optim_reference as O
from test_gpu_elementwise_edges import GUARD, adam_buffers, all_nan, cached, close, lib, nans, same_bits, st, sync   # noqa: F401

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
HP = R.ADAM_HP
INF = float("inf")


# ---------------------------------------------------------------------------------------------- A. sum of squares

def partial_buffer(pairs):
    flat = nans(2 * pairs + GUARD, dtype=torch.float64)
    return flat, flat[:2 * pairs].view(pairs, 2)


def run_sumsq(lib, g, n, clip, flat, offset, capacity):
    L.check(lib.sat_grad_sumsq(g.data_ptr(), n, clip, flat.data_ptr(), offset, capacity, st()), "sat_grad_sumsq")
    sync()


@pytest.mark.parametrize("kind", O.SUMSQ_KINDS)
@pytest.mark.parametrize("clip", O.SUMSQ_CLIP)
@pytest.mark.parametrize("n", O.SUMSQ_N)
def test_grad_sumsq(lib, n, clip, kind):
    g = O.sumsq_inputs(kind, n)
    ref_total, ref_bad = O.sumsq(g.double(), clip)
    P = lib.sat_grad_sumsq_partials(n)
    assert P == O.sumsq_grid(n) and lib.sat_grad_sumsq_ws_bytes(n) == 16 * P
    gd = g.cuda()
    flat, pairs = partial_buffer(P)
    run_sumsq(lib, gd, n, clip, flat, 0, P)
    assert not torch.isnan(pairs[:, 1]).any() and all_nan(flat[2 * P:]), "every workgroup writes its pair and nothing else"
    again, _ = partial_buffer(P)
    run_sumsq(lib, gd, n, clip, again, 0, P)
    assert same_bits(flat, again), "two launches, the same bits"
    host = pairs.cpu()
    total, bad = math.fsum(host[:, 0].tolist()), sum(host[:, 1].tolist())
    print("sumsq n %d clip %g %s: total %.17g reference %.17g nonfinite %g" % (n, clip, kind, total, float(ref_total), bad))
    assert bad == ref_bad, "the count of non-finite elements is exact"
    if kind == "nan_last":
        assert clip > 0 or math.isnan(total)        # (the clamp turns a NaN into a bound: only the count speaks of it)
    elif kind == "inf_first" and clip == 0:
        assert total == INF
    elif kind == "zeros":
        assert total == 0.0
    else:
        assert abs(total - float(ref_total)) <= n * 2.0 ** -52 * float(ref_total)


def test_grad_sumsq_segments_fill_one_partial_array(lib):
    n1, n2 = 1028, 5
    g1, g2 = O.sumsq_inputs("randn", n1).cuda(), O.sumsq_inputs("randn", n2).cuda()
    flat, pairs = partial_buffer(4)
    run_sumsq(lib, g2, n2, 0.0, flat, 3, 4)
    assert all_nan(pairs[:3]) and not torch.isnan(pairs[3]).any()
    run_sumsq(lib, g1, n1, 0.0, flat, 1, 4)
    assert all_nan(pairs[0]) and not torch.isnan(pairs[1:]).any() and all_nan(flat[8:])
    want = float(O.sumsq(g1.cpu().double())[0] + O.sumsq(g2.cpu().double())[0])
    assert abs(math.fsum(pairs[1:, 0].cpu().tolist()) - want) <= (n1 + n2) * 2.0 ** -52 * want
    assert lib.sat_grad_sumsq(g1.data_ptr(), n1, 0.0, flat.data_ptr(), 3, 4, st()) == L.SAT_ERR_ARG      # 2 pairs from index 3 of 4


# ---------------------------------------------------------------------------------------------- B. sat_adamw_step

def ranges_arg(pairs):
    return ((ctypes.c_int64 * (2 * len(pairs)))(*[x for r in pairs for x in r]) if pairs else None), len(pairs)


class Norm:
    """the partial pairs of one buffer and the {norm, nonfinite} pair, NaN-filled with a guard behind"""

    def __init__(self, lib, n):
        self.P = lib.sat_grad_sumsq_partials(n)
        self.flat, self.pairs = partial_buffer(self.P)
        self.out_flat = nans(2 + GUARD, dtype=torch.float64)

    def intact(self):
        return all_nan(self.flat[2 * self.P:]) and all_nan(self.out_flat[2:])


def adamw_call(lib, b, n, clip, step, wd=0.0, ranges=(), max_norm=None, norm=None, skip=None):
    """sat_grad_sumsq (with a max_norm) + sat_adamw_step on the guarded buffers of adam_buffers"""
    ex, nex = ranges_arg(list(ranges))
    partials, P, out = None, 0, None
    if max_norm is not None:
        L.check(lib.sat_grad_sumsq(b["g"][0].data_ptr(), n, clip, norm.flat.data_ptr(), 0, norm.P, st()), "sat_grad_sumsq")
        partials, P, out = norm.flat.data_ptr(), norm.P, norm.out_flat.data_ptr()
    L.check(lib.sat_adamw_step(*[b[k][0].data_ptr() for k in ("p", "g", "m", "v")], n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"],
                               clip, step, wd, ex, nex, max_norm if max_norm is not None else 0.0, partials, P, out, L.ptr(skip),
                               st()), "sat_adamw_step")
    sync()


def three_steps(lib, n, clip, mode, wd, ex, check=None):
    d = R.adam_inputs(n)
    b, norm = adam_buffers(d, n), Norm(lib, n)
    mx, ranges = O.max_norm_of(mode, n, clip), O.exempt_ranges(ex, n)
    for step in (1, 2, 3):
        b["g"][1].copy_(d["grads"][step - 1])
        adamw_call(lib, b, n, clip, step, wd, ranges, mx, norm)
        if check is not None:
            check(step, b, norm)
    return b, norm


@pytest.mark.parametrize("n,clip,mode,wd,ex", O.adamw_cases(), ids=lambda v: str(v))
def test_adamw_three_steps_from_nonzero_moments(lib, n, clip, mode, wd, ex):
    case = (n, clip, mode, wd, ex)
    ref = O.adamw_case(*case)           # (one use per case: not kept)
    e = O.f32_err(*case)
    assert mode != "half" or not ref[0]["coef_is_one"], "half the first step's norm scales the first step"
    assert mode not in ("off", "inf", "twice") or ref[0]["coef_is_one"]

    def check(step, b, norm):
        tag = "adamw n %d clip %g %s wd %g %s step %d" % (case + (step,))
        r = ref[step - 1]
        g = b["g"][1].cpu().double()
        if r["coef_is_one"]:
            assert torch.equal(g, r["g"]), tag + ": clamp and a coefficient of 1 are exact"
        else:
            assert ((g - r["g"]).abs() <= 2.0 ** -22 * r["g"].abs()).all(), tag + ": the scaled gradient"
        close(tag + " p", b["p"][1], r["p"], e["p"], atol=2e-7)
        close(tag + " m", b["m"][1], r["m"], e["m"])
        close(tag + " v", b["v"][1], r["v"], e["v"])
        assert all(all_nan(b[k][0][n:]) for k in b), tag + ": wrote past element n"
        if mode == "off":
            assert all_nan(norm.out_flat) and all_nan(norm.flat), tag + ": no norm asked for, none written"
        else:
            got, bad = norm.out_flat[:2].tolist()
            want = float(r["norm"])
            print("%-52s norm %.17g reference %.17g" % (tag, got, want))
            assert bad == 0.0 and abs(got - want) <= (n * 2.0 ** -53 + 2.0 ** -52) * want and norm.intact(), tag

    three_steps(lib, *case, check=check)


def all_bits(b):
    return {k: b[k][0].clone() for k in b}


@pytest.mark.parametrize("clip", O.ADAMW_CLIP)
@pytest.mark.parametrize("n", O.ADAMW_N)
def test_adamw_without_norm_and_decay_is_clamp_adam_guarded_bit_for_bit(lib, n, clip):
    d = R.adam_inputs(n)
    old, new, table = adam_buffers(d, n), adam_buffers(d, n), adam_buffers(d, n)
    zero = torch.zeros(1, device="cuda")
    for step in (1, 2, 3):
        for b in (old, new, table):
            b["g"][1].copy_(d["grads"][step - 1])
        L.check(lib.sat_clamp_adam_step_guarded(*[old[k][0].data_ptr() for k in ("p", "g", "m", "v")], n, HP["lr"], HP["beta1"],
                                                HP["beta2"], HP["eps"], clip, step, L.ptr(zero), st()), "sat_clamp_adam_step_guarded")
        adamw_call(lib, new, n, clip, step, skip=zero)
        adamw_call(lib, table, n, clip, step, wd=0.0, ranges=O.exempt_ranges("many", n))      # a table without decay changes nothing
        for k in old:
            assert same_bits(new[k][0], old[k][0]) and same_bits(table[k][0], old[k][0]), (k, step)


@pytest.mark.parametrize("clip", O.ADAMW_CLIP)
@pytest.mark.parametrize("n", O.ADAMW_N)
def test_a_max_norm_above_the_norm_changes_no_bit(lib, n, clip):
    """max_norm = twice the first step's norm against no norm at all, with decay and ranges: equal bits for as long as the
    reference's coefficient is 1 (the later steps' norms are other numbers; the first step always counts), and so is +inf"""
    ref = cached(("adamw", n, clip, "twice", 0.01, "interior"), lambda: O.adamw_case(n, clip, "twice", 0.01, "interior"))
    ones = [r["coef_is_one"] for r in ref]
    assert ones[0]
    runs = {mode: [] for mode in ("off", "twice", "inf")}
    for mode, states in runs.items():
        three_steps(lib, n, clip, mode, 0.01, "interior", check=lambda step, b, norm: states.append(all_bits(b)))
    for step in range(3):
        for k in ("p", "g", "m", "v"):
            assert same_bits(runs["inf"][step][k], runs["off"][step][k]), (k, step)
            if all(ones[:step + 1]):
                assert same_bits(runs["twice"][step][k], runs["off"][step][k]), (k, step)


@pytest.mark.parametrize("ex", [x for x in O.ADAMW_EXEMPT if x != "none"])
@pytest.mark.parametrize("n", O.ADAMW_N)
def test_exempt_elements_do_not_decay_and_the_others_do(lib, n, ex):
    mask = O.exempt_mask(O.exempt_ranges(ex, n), n)
    first = {}

    def keep(wd):
        return lambda step, b, norm: first.setdefault(wd, b["p"][1].cpu()) if step == 1 else None

    plain, _ = three_steps(lib, n, 0.1, "half", 0.0, ex, check=keep(0.0))
    decayed, _ = three_steps(lib, n, 0.1, "half", 0.01, ex, check=keep(0.01))
    p0, p1 = plain["p"][1].cpu(), decayed["p"][1].cpu()
    assert mask.any()
    assert same_bits(p0[mask], p1[mask]), "an exempt element has the bits of the run without decay"
    assert same_bits(first[0.0][mask], first[0.01][mask])
    # after ONE step the two runs differ by lr wd |p| = 1e-5 |p| before rounding: that shows wherever it is above a few spacings
    # (2^-23 relative) of the floats near p and near the updated p; elements below that may round to the same bits
    init = R.adam_inputs(n)["p"]
    big = 1e-5 * init.abs() > 2.0 ** -20 * torch.maximum(init.abs(), first[0.0].abs())
    assert (~mask & big).any() or n < 8
    assert (first[0.0] != first[0.01])[~mask & big].all(), "every other element decayed"
    for k in ("g", "m", "v"):
        assert same_bits(plain[k][0], decayed[k][0]), "the decay touches the parameters only"


@pytest.mark.parametrize("n", [5, 1023, 786439])
def test_skip_word_and_nan_gradient_leave_everything_untouched(lib, n):
    """the NaN is an input value: the last tail element of the gradient.  A dropped step writes neither p, g, m nor v."""
    d = R.adam_inputs(n)
    mx = O.max_norm_of("half", n, 0.1)
    ranges = O.exempt_ranges("first", n)
    for what in ("skip", "nan", "inf_clamped"):
        b, norm = adam_buffers(d, n), Norm(lib, n)
        b["g"][1].copy_(d["grads"][0])
        if what == "nan":
            b["g"][1][n - 1] = float("nan")
        if what == "inf_clamped":
            b["g"][1][0] = INF                     # the clamp would hide it from the sum: the count still drops the step
        before = all_bits(b)
        skip = torch.full((1,), 3.0 if what == "skip" else 0.0, device="cuda")
        adamw_call(lib, b, n, 0.1, 1, 0.01, ranges, mx, norm, skip=skip)
        for k in b:
            assert same_bits(b[k][0], before[k]), "%s: %s changed" % (what, k)
        if what == "skip":
            assert all_nan(norm.out_flat), "the skip word comes first: no norm is reported"
        else:
            assert norm.out_flat[1].item() == 1.0 and norm.intact()
    # the same buffers without the fault: the step happens
    b, norm = adam_buffers(d, n), Norm(lib, n)
    b["g"][1].copy_(d["grads"][0])
    before = all_bits(b)
    adamw_call(lib, b, n, 0.1, 1, 0.01, ranges, mx, norm, skip=torch.zeros(1, device="cuda"))
    assert not same_bits(b["p"][0], before["p"]) and norm.out_flat[1].item() == 0.0


# ---------------------------------------------------------------------------------------------- C. modules

SMALL_VGG = [16, 16, "M", 32, "M", 64, 64, "M", 64]


def attend_model():
    torch.manual_seed(8)
    return sat.ShowAttendTellModel(96, 64, 50, 32, None, feature_size=(16, 64), compute_dtype="f32", vgg_cfg=SMALL_VGG).cuda()


def attend_batch():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(4, 3, 32, 32, generator=g).cuda()
    caps = torch.randint(1, 50, (4, 7), generator=g).cuda()
    lengths = [7, 6, 4, 3]
    targets, l1 = sat.pack_targets(caps, lengths)
    return x, caps, l1, targets


def torch_adamw(model, wd):
    ps = [p for p in model.parameters() if p.requires_grad]
    nd = {id(p) for p in sat.no_decay_params(model)}
    return ps, torch.optim.AdamW([dict(params=[p for p in ps if id(p) not in nd], weight_decay=wd),
                                  dict(params=[p for p in ps if id(p) in nd], weight_decay=0.0)], lr=1e-3)


@pytest.mark.parametrize("max_norm", [0.5, 0.02])
def test_fused_clamp_adam_equals_torch_clip_grad_norm_and_adamw(max_norm):
    """three steps of the Show-Attend-Tell drop-in loop; the elementwise clamp in front of the norm, as in the kernel"""
    x, caps, l1, targets = attend_batch()
    crit = torch.nn.CrossEntropyLoss()
    ma, mb = attend_model(), attend_model()
    pa, oa = torch_adamw(ma, 0.01)
    ob = sat.FusedClampAdam([p for p in mb.parameters() if p.requires_grad], lr=1e-3, clip=0.1, max_norm=max_norm, weight_decay=0.01,
                            no_decay=sat.no_decay_params(mb))
    assert ob.last_grad_norm is None and 0 < len(ob._exempt) <= 32
    for step in range(3):
        ma.zero_grad()
        crit(ma(x, caps[:, :-1], l1), targets).backward()
        for p in pa:
            p.grad.data.clamp_(-0.1, 0.1)
        norm = torch.nn.utils.clip_grad_norm_(pa, max_norm)
        oa.step()
        ob.zero_grad()
        crit(mb(x, caps[:, :-1], l1), targets).backward()
        ob.step()
        got = ob.last_grad_norm.tolist()
        print("step %d: norm %.9g torch %.9g" % (step, got[0], float(norm)))
        assert got[1] == 0.0 and abs(got[0] - float(norm)) <= 1e-6 * float(norm)
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert (a - b).abs().max().item() <= 2e-6, n
    sd = ob.state_dict()
    assert sd["max_grad_norm"] == max_norm and sd["grad_clip"] == 0.1
    assert sd["param_groups"][0]["weight_decay"] == 0.01 and sd["param_groups"][0]["decoupled_weight_decay"] is True
    oc = torch.optim.AdamW([p for p in attend_model().parameters() if p.requires_grad], lr=1e-3)
    oc.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})
    assert oc.param_groups[0]["weight_decay"] == 0.01 and float(oc.state[oc.param_groups[0]["params"][0]]["step"]) == 3.0
    ob2 = sat.FusedClampAdam([p for p in attend_model().parameters() if p.requires_grad], lr=5e-4)
    ob2.load_state_dict(sd)
    assert ob2.step_count == 3 and ob2.weight_decay == 0.01 and ob2.max_norm == max_norm and torch.equal(ob2.exp_avg, ob.exp_avg)


def test_fused_clamp_adam_ignores_a_parameter_without_gradient():
    x, caps, l1, targets = attend_batch()
    crit = torch.nn.CrossEntropyLoss()
    ma, mb = attend_model(), attend_model()
    pa, oa = torch_adamw(ma, 0.01)
    pb = [p for p in mb.parameters() if p.requires_grad]
    ob = sat.FusedClampAdam(pb, lr=1e-3, max_norm=0.02, weight_decay=0.01, no_decay=sat.no_decay_params(mb))
    for step in range(2):                                     # a first full step, so that the moments are not zero
        ma.zero_grad()
        crit(ma(x, caps[:, :-1], l1), targets).backward()
        ob.zero_grad()
        crit(mb(x, caps[:, :-1], l1), targets).backward()
        k = 1                                                 # (a parameter in the middle: two segments)
        if step == 1:
            pa[k].grad = None
            pb[k].grad = None
            o, n = ob._slices[k]
            before = [t[o:o + n].clone() for t in (ob.flat, ob.exp_avg, ob.exp_avg_sq)]
        norm = torch.nn.utils.clip_grad_norm_(pa, 0.02)
        oa.step()
        ob.step()
    got = ob.last_grad_norm.tolist()
    assert got[1] == 0.0 and abs(got[0] - float(norm)) <= 1e-6 * float(norm), (got, float(norm))
    for t, was in zip((ob.flat, ob.exp_avg, ob.exp_avg_sq), before):
        assert same_bits(t[o:o + n], was), "the parameter without a gradient, and its moments, stay"
    for a, b in zip(pa, pb):
        assert (a - b).abs().max().item() <= 2e-6


SMOKE = dict(E=32, H=64, V=200, L=1, B=4, T=10)


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


def test_train_step_equals_the_reference_on_its_own_buffers():
    """two steps (the second from non-zero moments); the norm is taken over flat.grads[:flat.n]: the loss slot behind it holds about
    ln V = 5.3, far above the gradient norm, so a norm that included it would give another coefficient"""
    model = smoke_model()
    ts = sat.TrainStep(model)
    names = sat.no_decay_names(model)
    ts.max_grad_norm, ts.weight_decay, ts.no_decay = 0.05, 0.01, names
    f = ts.flat
    ranges = ts._exempt
    assert ranges and all(any(lo <= f.slices[n][0] < hi for lo, hi in ranges) for n in names)
    images, caps, lengths = smoke_batch()
    for step in (1, 2):
        p0, m0, v0 = f.params.cpu(), f.m.cpu(), f.v.cpu()
        ts.forward_backward((images, caps, lengths), 1.0 / sum(l - 1 for l in lengths))
        g0 = f.grads[:f.n].cpu()
        loss = f.grads[f.loss_slot].item()
        ts.optimizer_step()
        torch.cuda.synchronize()
        hp = dict(lr=ts.lr, beta1=ts.betas[0], beta2=ts.betas[1], eps=ts.eps)
        r64 = O.adamw_step(p0.double(), g0.double(), m0.double(), v0.double(), step, ts.grad_clip, 0.05, 0.01, ranges, **hp)
        r32 = O.adamw_step(p0, g0, m0, v0, step, ts.grad_clip, 0.05, 0.01, ranges, **hp)
        norm = float(r64[4])
        got = ts.last_grad_norm.tolist()
        print("step %d: loss %.4f norm %.9g reference %.9g" % (step, loss, got[0], norm))
        assert math.hypot(norm, loss) > 1.5 * norm and float(O.coef(r64[4], 0.05)) < 1.0, "the slot would move the norm, and the norm scales"
        assert got[1] == 0.0 and abs(got[0] - norm) <= (f.n * 2.0 ** -53 + 2.0 ** -52) * norm
        for k, got_t, i in (("p", f.params, 0), ("m", f.m, 2), ("v", f.v, 3)):
            close("TrainStep step %d %s" % (step, k), got_t, r64[i], R.max_err(r32[i], r64[i]), atol=2e-7 if k == "p" else 0.0)
        assert ((f.grads[:f.n].cpu().double() - r64[1]).abs() <= 2.0 ** -22 * r64[1].abs()).all()
    assert ts.step_count == 2
    sd = ts.optimizer_state_dict()
    assert sd["max_grad_norm"] == 0.05 and sd["param_groups"][0]["weight_decay"] == 0.01
    torch.optim.AdamW([p for p in model.parameters() if p.requires_grad]).load_state_dict(
        {"state": sd["state"], "param_groups": sd["param_groups"]})


def test_train_step_with_the_attributes_at_their_defaults_keeps_its_bits():
    images, caps, lengths = smoke_batch()
    a, b = sat.TrainStep(smoke_model()), sat.TrainStep(smoke_model())
    b.max_grad_norm, b.weight_decay, b.no_decay = 0.0, 0.0, None
    for _ in range(2):
        a.step(images, caps, lengths)
        b.step(images, caps, lengths)
    torch.cuda.synchronize()
    assert same_bits(a.flat.params, b.flat.params) and same_bits(a.flat.m, b.flat.m) and same_bits(a.flat.v, b.flat.v)
    assert a.last_grad_norm is None and b.last_grad_norm is None


def test_train_step_drops_a_step_with_a_non_finite_gradient():
    """the NaN arrives as a value in the gradient buffer between backward and the optimizer step; no host read is needed to drop
    the update, `last_grad_norm[1]` tells afterwards and `step_count` has advanced"""
    images, caps, lengths = smoke_batch()
    ts = sat.TrainStep(smoke_model())
    ts.max_grad_norm = INF
    ts.step(images, caps, lengths)
    ts.forward_backward((images, caps, lengths), 1.0 / sum(l - 1 for l in lengths))
    ts.flat.grads[7] = float("nan")
    before = [t.clone() for t in (ts.flat.params, ts.flat.m, ts.flat.v, ts.flat.grads)]
    ts.optimizer_step()
    torch.cuda.synchronize()
    assert all(same_bits(t, was) for t, was in zip((ts.flat.params, ts.flat.m, ts.flat.v, ts.flat.grads), before))
    assert ts.last_grad_norm[1].item() == 1.0 and ts.step_count == 2
    ts.step(images, caps, lengths)
    assert ts.last_grad_norm[1].item() == 0.0 and not same_bits(ts.flat.params, before[0])


DP_SETTINGS = dict(max_grad_norm=0.05, weight_decay=0.01)
SPAWN_LIMIT = 240.0        # seconds for the two ranks together (each imports torch, builds a model and runs two steps)


def dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from test_gpu_dp import LENGTHS, make_batch, make_model
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    feats, caps = make_batch()
    model = make_model(sat)
    ts = sat.TrainStep(model)
    ts.max_grad_norm, ts.weight_decay = DP_SETTINGS["max_grad_norm"], DP_SETTINGS["weight_decay"]
    ts.no_decay = [n for n in sat.no_decay_names(model) if n in ts.flat.slices]
    dp = sat.DataParallelStep(ts)
    losses, norms = [], []
    for _ in range(2):
        f, c, ln, tokens = sat.dp_shard(feats.cuda(), caps.cuda(), LENGTHS, rank, world)
        losses.append(float(dp.step((f, c, ln), tokens).item()))
        norms.append(ts.last_grad_norm.cpu().clone())
    torch.cuda.synchronize()
    torch.save({"params": {k: v.detach().cpu() for k, v in model.decoder.named_parameters()}, "losses": losses, "norms": norms},
               "%s.%d" % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_share_one_norm_and_equal_the_single_process_step(tmp_path):
    from test_gpu_dp import LENGTHS, make_batch, make_model
    out = str(tmp_path / "rank")
    port = 31600 + os.getpid() % 2000
    ctx = mp.spawn(dp_worker, args=(2, port, out), nprocs=2, join=False)
    deadline = time.monotonic() + SPAWN_LIMIT
    while not ctx.join(timeout=1.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish within %g s" % SPAWN_LIMIT)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    for a, b in zip(r0["norms"], r1["norms"]):
        assert same_bits(a, b) and a[1].item() == 0.0 and a[0].item() > 0, "every rank computes the same bits from the same buffer"
    for k in r0["params"]:
        assert same_bits(r0["params"][k], r1["params"][k]), k
    feats, caps = make_batch()
    model = make_model(sat)
    ts = sat.TrainStep(model)
    ts.max_grad_norm, ts.weight_decay = DP_SETTINGS["max_grad_norm"], DP_SETTINGS["weight_decay"]
    ts.no_decay = [n for n in sat.no_decay_names(model) if n in ts.flat.slices]
    ref_losses, ref_norms = [], []
    for _ in range(2):
        ref_losses.append(float(ts.step(feats.cuda(), caps.cuda(), LENGTHS).item()))
        ref_norms.append(ts.last_grad_norm[0].item())
    for a, b in zip(r0["losses"], ref_losses):
        assert abs(a - b) < 1e-5
    for a, b in zip(r0["norms"], ref_norms):
        print("norm: two ranks %.9g single process %.9g" % (a[0].item(), b))
        assert abs(a[0].item() - b) <= 1e-5 * b            # the reduced gradient is another f32 sum than the single batch's
    for k, p in model.decoder.named_parameters():
        np.testing.assert_allclose(r0["params"][k].numpy(), p.detach().cpu().numpy(), rtol=0, atol=2e-6, err_msg=k)
