"""GPU (MI355X): the kernels of csrc/sat_elementwise.hip at the shapes where their launchers, paths and tails change, each through
the C ABI or a one-op program against the float64 reference of tests/elementwise_reference.py (validated on the CPU by
tests/test_elementwise_reference_host.py).

Buffers a kernel promises to overwrite start as NaN; pad columns, the elements past the end and the other-parity accumulators are
guards that must survive bit for bit; a buffer a kernel must not touch (write_grad = 0 logits, everything under a non-zero skip
word, the running statistics in eval mode) must keep its bits.

Shapes and the path each reaches, from the launchers (V = 4 f32 / 8 bf16 elements per 16-byte chunk, cch = C / V chunks per pixel,
grid = min(768, ceil(chunks / 256)) workgroups of 256 threads, stride = grid * block; the fast path needs stride % cch == 0):

BN normalise, bn_act_kernel (f32 | bf16):
  (1,1,1,8)        2 | 1 chunks, grid 1: one live thread (two in f32), fast path, slot 0 only
  (3,10,10,32)     2400 | 1200 chunks, grid 10 | 5, cch 8 | 4: the shape of test_bn_finalize_apply_pool, fast path, slot 0 only --
                   but with a derived table the bf16 launch becomes 5 / 2 = 2 workgroups of 512: 1024 threads for 1200 chunks, so
                   slot 1 of the pipelined loop is live for 176 threads
  (2,5,5,24) f32, (2,5,5,48) bf16   cch = 6, 300 chunks, grid 2, stride 512, 512 % 6 = 2: the SLOW path, one trip
  (2,7,7,2048) f32   cch = 512 > 256: grid 196 kept a multiple of 512 / 256 = 2 by the rounding branch, stride 50176 = 98 * 512: fast
  (2,7,7,2048) bf16  cch = 256, 25088 chunks, grid 98, fast
  every one with: table given; table derived from integer sums (512-thread workgroups where 512 % cch == 0 and grid >= 2; both
  parities; running statistics; the other parity's accumulators cleared); residual plain, with scale1/shift1, with stat_acc1
  (has_b1 from integer sums); out == in0
  (13,56,56,64) f32, (13,56,56,128) bf16   652,288 chunks, grid 768, stride 196,608: slots 0..2 full, slot 3 partial (first trip of
                   the 4-slot loop); the residual form's 2-slot loop makes a second trip
  (17,56,56,64|128)  852,992 chunks > 4 * 196,608: second trip of the 4-slot loop, third of the 2-slot loop
  (7,56,56,40) f32   cch = 10, 219,520 chunks, 196,608 % 10 = 8: the slow path's second grid-stride trip
  groups = 3 x (2,5,5,32), derived tables: normalise, normalise+add, channel slice (bn_relu_strided_kernel), maxpool (bf16: the f32
  maxpool launcher refuses groups, asserted); the channel slice alone: C = 32 at offset 16 of ldc = 80
Maxpool, bn_relu_maxpool_kernel: (1,1,1,8) one window of one pixel; (1,2,2,8) one output, 4 of 9 taps; (2,5,7,8) odd sizes, the last
  window clipped on the right in W only; (1,9,12,16) even W: the last window has its right column outside; (1,10,10,32) the
  existing shape; (4,112,112,64) f32: 200,704 items > 196,608, the grid-stride loop's second trip; an all-negative input: exact 0
Avgpool: HW 1 (tail only), 3 (tail only), 4 (unrolled only), 49 (12 x 4 + 1), 50 (12 x 4 + 2); C = 8 (one or two chunks per image)
  and 2048; N = 1, 3
BN finalize, bn_finalize_kernel (32 row groups; the unrolled loop runs while t + 96 < tiles_m): tiles_m 1 (31 idle row groups), 31,
  32, 33 (the second trip of the plain loop), 127 (unrolled once for row groups 0..30, then not at all for 31), 128 (unrolled once
  for all), 129 (unrolled + one plain trip), 300 (two unrolled trips + a tail); C = 4, 40 (a second workgroup with 8 live
  channels), 64; training with and without running statistics, training = 0 (NaN slabs: never read), count = 1 (var = rounding
  noise, clamped at 0 where negative), a constant channel (var exactly 0)
Slab reducer, bn_slab_to_acc_kernel (128 tiles per workgroup): tiles_m 1, 127, 128, 129 (a second workgroup with 1 tile), 300;
  groups 1, 2; both parities
bn_eval_batch / sat_bn_running_apply: one launch over C = 1, 255, 256, 257, 600 (the c += 256 loop: 1, 1, 1, 2, 3 trips)
sat_ce_rows (register path: ldl % 4 == 0, V / 4 <= 3072, aligned base):
  V = 1, 3       nq = 0: the scalar tail only (register path at ldl = 4), fallback at ldl = V
  V = 4, 5       one chunk (+ 1 tail element)
  V = 255, 1003  tail of 3; 1003 fills chunks 0 and part of 1 per thread (250 chunks)
  V = 1024       exactly one chunk per thread, no tail; V = 12288: all 12 register chunks full
  V = 12289      12 chunks full + 1 tail element (register path at ldl = 12292); V = 12292: 3073 chunks > 3072: fallback
  ldl = pad4(V), V (fallback unless V % 4 == 0), V + 4 (NaN pads; fallback when (V + 4) % 4 != 0); base + 1 float: fallback
  targets placed at 0, V - 1, 4 * (V / 4) (`tail == tgt && tq >= nq`), 1023, 1024 (the chunk boundary of thread 255 / 0), -1, V
sat_colsum_f32 (unrolled while r + 24 < rows, r = row group 0..7): rows 1, 7, 8, 9, 24 (no unrolled trip), 25 (row group 0 only),
  32 (row groups 0..6), 33 (all, + a plain trip for group 0), 57 (two unrolled trips for group 0); cols 1, 31, 32, 33, 100
sat_clamp_adam_step: n 1, 3 (tail only), 4 (no tail), 5, 1023 (255 chunks + 3), 786439 (196,609 chunks > 768 * 256: second trip,
  n % 4 = 3)
sat_fc_bn1d_fwd / _bwd (32 features x 8 row groups): B 1 (var = 0), 2, 7 (< 8 row groups), 8, 9, 12; E 4, 31, 32, 33, 40
Embedding: T = 1 (no token rows, captions NULL), ragged batch sizes, E 1, 255, 256, 257, one token everywhere, 4 tokens over 24 rows,
  ids -1, V, V + 5

Tolerances.  An f32 output passes when it meets the tolerance the existing one-shape test uses for it (test_bn_finalize_apply_pool:
scale rtol 2e-5, shift rtol 2e-4 + 2e-5, running mean rtol 1e-5 + 1e-6, running var rtol 1e-5, y 1e-5, 2e-5 with the residual
table, avgpool 1e-5; test_ce_rows_and_colsum: gradient 2e-8 + 1e-6 inv, loss 1e-5 relative, column sums 1e-7;
test_clamp_adam_matches_torch: p 2e-7; test_fc_bn1d_fwd_bwd: feats 2e-5, running statistics rtol 1e-5 + 1e-7, dgamma / dbeta rtol
1e-4 + 1e-5, dw rtol 1e-3 + 2e-5, db 5e-4) OR lies within 8 x the error of the float32 torch restatement of the same formula
against float64 at that shape and seed (elementwise_reference.F32_ERR, frozen from the host test's measurement; outputs no
existing test bounds -- row losses, Adam's moments, xhat, rstd -- have the second rule only).  A bf16 output gets one bf16
rounding of the result on top: 2^-8 |ref|.  Bitwise where the arithmetic is pinned: the clamp, the gathers, pads and guards, the
integer accumulators on dyadic slabs, the eval table against finalize, the running-statistics apply, zero-weight rows, the skipped
Adam step, in-place against out-of-place.  Nothing here is set from a kernel's output."""
import importlib

import numpy as np
import pytest
import torch

import elementwise_reference as R

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

NAN = float("nan")
DT = {"f32": L.SAT_F32, "bf16": L.SAT_BF16}
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    return L.load()


def st():
    return L.stream()


def sid(v):
    return "x".join(str(i) for i in v) if isinstance(v, (tuple, list)) else str(v)


def sync():
    torch.cuda.synchronize()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def guarded(shape, dtype=torch.float32):
    """(flat, view): a NaN buffer of prod(shape) + GUARD elements and the view of its head; flat[n:] is the guard past the end"""
    n = int(np.prod(shape))
    flat = nans(n + GUARD, dtype=dtype)
    return flat, flat[:n].view(*shape)


def bits(t):
    t = t.contiguous().cpu()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def all_nan(t):
    return bool(torch.isnan(t).all())


def dev(t, dtype=None):
    return t.cuda() if dtype is None else t.to(dtype).cuda()


def close(tag, got, ref, e32, rtol=0.0, atol=0.0, bf16=False):
    """got (device or host) against ref (f64): the existing tolerance |err| <= atol + rtol |ref|, or 8 x the f32 restatement's error
    e32; a bf16 output gets 2^-8 |ref| on top of either; prints the figures before it asserts"""
    got = got.detach().float().cpu().double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert torch.isfinite(got).all(), tag + ": inf or NaN in the output"
    err = (got - ref).abs()
    extra = R.BF16_ROUND * ref.abs() if bf16 else torch.zeros_like(ref)
    legacy = (atol > 0 or rtol > 0) and bool((err <= atol + rtol * ref.abs() + extra).all())
    second = bool((err <= R.TOL_FACTOR * e32 + extra).all())
    worst = err.max().item() if err.numel() else 0.0
    print("%-52s err %.3g   f32 restatement %.3g   existing tolerance %s" % (tag, worst, e32, "met" if legacy else "not met"))
    assert legacy or second, "%s: err %.3g > %g x %.3g%s" % (tag, worst, R.TOL_FACTOR, e32, " + 2^-8 |ref|" if bf16 else "")


def run(lib, ops, parity=0):
    arr = (L.SatOp * len(ops))(*ops)
    L.check(lib.sat_run_ops_parity(arr, len(ops), parity, st()), "sat_run_ops_parity")
    sync()


def bn_op(kind, dtn, shape, **kw):
    N, H, W, Cc = shape
    kw.setdefault("Hout", H)
    kw.setdefault("Wout", W)
    return L.op(kind, DT[dtn], N=N, Cout=Cc, momentum=R.BN_MOMENTUM, eps=R.BN_EPS, **kw)


_REF = {}


def cached(key, fn):
    """float64 references are computed once, shared, and never modified"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def acc_pair(acc_this, parity, junk=12345):
    """device [2 parities][2][C] accumulators: the step's parity holds the sums, the other one junk the consumer must clear"""
    a = torch.full((2,) + tuple(acc_this.shape), junk, dtype=torch.int64)
    a[parity] = acc_this
    return a.cuda()


# ---------------------------------------------------------------------------------------------- A. normalise

RS = dict(rtol=1e-5, atol=1e-6)          # running mean; running var: rtol 1e-5 (test_bn_finalize_apply_pool)


def check_running(tag, rm, rv, ref, e, suffix=""):
    close(tag + " running_mean" + suffix, rm, ref["running_mean" + suffix], e.get("running_mean" + suffix, 0.0), **RS)
    close(tag + " running_var" + suffix, rv, ref["running_var" + suffix], e.get("running_var" + suffix, 0.0), rtol=1e-5)


@pytest.mark.parametrize("dtn,shape", [(dn, s) for dn in ("f32", "bf16") for s in R.BN_SMALL[dn]], ids=lambda v: sid(v))
def test_bn_act_every_form_at_the_small_shapes(lib, dtn, shape):
    d = R.bn_inputs(dtn, shape)
    ref = cached(("bn", dtn, shape), lambda: R.bn_case(dtn, shape, names=R.BN_OUTPUTS))
    e = R.f32_err("bn", dtn, shape)
    bf, td, Cc, tag = dtn == "bf16", TD[dtn], shape[3], "bn %s %s" % (dtn, sid(shape))
    x, z = dev(d["x"], td), dev(d["z"], td)
    t = {k: dev(d[k]) for k in ("scale", "shift", "scale1", "shift1", "gamma", "beta", "gamma1", "beta1")}
    given = dict(scale0=t["scale"], shift0=t["shift"])
    # table given: relu, + residual, + residual with its own table
    outs = {}
    for form, kind, kw, tol in (("relu", L.OP_BN_RELU, {}, 1e-5), ("add", L.OP_BN_ADD_RELU, dict(in1=z), 1e-5),
                                ("add_b1", L.OP_BN_ADD_RELU, dict(in1=z, scale1=t["scale1"], shift1=t["shift1"]), 2e-5)):
        flat, y = guarded(shape, td)
        run(lib, [bn_op(kind, dtn, shape, in0=x, out=y, **given, **kw)])
        close("%s %s" % (tag, form), y, ref[form], e[form], atol=tol, bf16=bf)
        assert all_nan(flat[y.numel():]), "wrote past the end"
        outs[form] = y
    # out == in0: the same bits as out of place
    for form, kind, kw in (("relu", L.OP_BN_RELU, {}), ("add", L.OP_BN_ADD_RELU, dict(in1=z))):
        flat, y = guarded(shape, td)
        y.copy_(x)
        run(lib, [bn_op(kind, dtn, shape, in0=y, out=y, **given, **kw)])
        assert same_bits(y, outs[form]) and all_nan(flat[y.numel():]), form + " in place"
    # table derived from integer sums, both parities
    for parity in (0, 1):
        acc, rm, rv = acc_pair(d["acc"], parity), dev(d["rm"]), dev(d["rv"])
        flat, y = guarded(shape, td)
        run(lib, [bn_op(L.OP_BN_RELU, dtn, shape, in0=x, out=y, stat_acc=acc, gamma=t["gamma"], beta=t["beta"], running_mean=rm,
                        running_var=rv, count=d["count"])], parity)
        close("%s relu derived p%d" % (tag, parity), y, ref["relu_derived"], e["relu_derived"], atol=1e-5, bf16=bf)
        check_running(tag + " derived", rm, rv, ref, e)
        assert all_nan(flat[y.numel():])
        assert torch.equal(acc[parity].cpu(), d["acc"]) and int(acc[1 - parity].abs().sum()) == 0
        # residual whose table comes from integer sums too (has_b1 through stat_acc1); without running statistics for b0
        acc, acc1, rm1, rv1 = acc_pair(d["acc"], parity), acc_pair(d["acc1"], parity, 777), dev(d["rm1"]), dev(d["rv1"])
        flat, y = guarded(shape, td)
        run(lib, [bn_op(L.OP_BN_ADD_RELU, dtn, shape, in0=x, in1=z, out=y, stat_acc=acc, gamma=t["gamma"], beta=t["beta"],
                        stat_acc1=acc1, gamma1=t["gamma1"], beta1=t["beta1"], running_mean1=rm1, running_var1=rv1,
                        count=d["count"])], parity)
        close("%s add derived p%d" % (tag, parity), y, ref["add_derived"], e["add_derived"], atol=2e-5, bf16=bf)
        check_running(tag + " derived", rm1, rv1, ref, e, "1")
        assert all_nan(flat[y.numel():])
        for a, want in ((acc, d["acc"]), (acc1, d["acc1"])):
            assert torch.equal(a[parity].cpu(), want) and int(a[1 - parity].abs().sum()) == 0


@pytest.mark.parametrize("dtn,shape", [(dn, s) for dn in ("f32", "bf16") for s in R.BN_LARGE[dn]], ids=lambda v: sid(v))
def test_bn_act_pipelined_loop_and_second_trips(lib, dtn, shape):
    d = R.bn_inputs(dtn, shape)
    ref = cached(("bn_large", dtn, shape), lambda: R.bn_case(dtn, shape, names=("relu", "add_b1")))
    e = R.f32_err("bn_large", dtn, shape)
    bf, td, tag = dtn == "bf16", TD[dtn], "bn %s %s" % (dtn, sid(shape))
    x, z = dev(d["x"], td), dev(d["z"], td)
    t = {k: dev(d[k]) for k in ("scale", "shift", "scale1", "shift1")}
    flat, y = guarded(shape, td)
    run(lib, [bn_op(L.OP_BN_RELU, dtn, shape, in0=x, out=y, scale0=t["scale"], shift0=t["shift"])])
    close(tag + " relu", y, ref["relu"], e["relu"], atol=1e-5, bf16=bf)
    assert all_nan(flat[y.numel():])
    flat, y = guarded(shape, td)
    run(lib, [bn_op(L.OP_BN_ADD_RELU, dtn, shape, in0=x, in1=z, out=y, scale0=t["scale"], shift0=t["shift"], scale1=t["scale1"],
                    shift1=t["shift1"])])
    close(tag + " add_b1", y, ref["add_b1"], e["add_b1"], atol=2e-5, bf16=bf)
    assert all_nan(flat[y.numel():])


@pytest.mark.parametrize("form", R.GROUPED_FORMS)
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_bn_grouped_launch_with_per_group_statistics(lib, dtn, form):
    shape, G = R.BN_GROUPED, R.BN_GROUPS
    N, H, W, Cc = shape
    ds = R.grouped_inputs(dtn)
    td, bf, tag = TD[dtn], dtn == "bf16", "grouped %s %s" % (dtn, form)
    x = dev(torch.cat([d["x"] for d in ds]), td)
    z = dev(torch.cat([d["z"] for d in ds]), td)
    parity = 1
    acc = torch.stack([acc_pair(d["acc"], parity) for d in ds])                     # [G][2][2][C]
    acc1 = torch.stack([acc_pair(d["acc1"], parity, 777) for d in ds])
    log = torch.stack([torch.stack([d["rm"], d["rv"]]) for d in ds]).cuda()         # [G][2][C]
    g0 = {k: dev(ds[0][k]) for k in ("gamma", "beta", "gamma1", "beta1")}
    stats = dict(stat_acc=acc, gamma=g0["gamma"], beta=g0["beta"], running_mean=log, running_var=log.data_ptr() + 4 * Cc,
                 count=ds[0]["count"], groups=G)
    if form == "pool":
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        flat, y = guarded((G, N, Ho, Wo, Cc), td)
        o = bn_op(L.OP_BN_RELU_MAXPOOL, dtn, shape, in0=x, out=y, Hin=H, Win=W, Hout=Ho, Wout=Wo, **stats)
        if dtn == "f32":        # by design: the f32 maxpool launcher has no grouped form and says so
            arr = (L.SatOp * 1)(o)
            assert lib.sat_run_ops_parity(arr, 1, parity, st()) == L.SAT_ERR_UNSUPPORTED
            return
    elif form == "slice":
        wide = nans(G, N * H * W, R.SLICE_LDC, dtype=td)
        o = bn_op(L.OP_BN_RELU, dtn, shape, in0=x, out=wide.data_ptr() + R.SLICE_OFF * wide.element_size(), ldc=R.SLICE_LDC, **stats)
    else:
        flat, y = guarded((G,) + shape, td)
        kw = dict(in1=z, stat_acc1=acc1, gamma1=g0["gamma1"], beta1=g0["beta1"]) if form == "add" else {}
        o = bn_op(L.OP_BN_ADD_RELU if form == "add" else L.OP_BN_RELU, dtn, shape, in0=x, out=y, **stats, **kw)
    run(lib, [o], parity)
    ref = cached(("grouped", dtn, form), lambda: R.grouped_case(dtn, form))
    e = R.f32_err("grouped", dtn, form)
    if form == "slice":
        y = wide[:, :, R.SLICE_OFF:R.SLICE_OFF + Cc].reshape((G,) + shape)
        assert all_nan(wide[:, :, :R.SLICE_OFF]) and all_nan(wide[:, :, R.SLICE_OFF + Cc:]), "the rest of the wide tensor"
    else:
        assert all_nan(flat[y.numel():])
    for g in range(G):      # each group against float64 on its own
        close("%s group %d" % (tag, g), y[g], ref["y"][g], e["y"], atol=2e-5 if form == "add" else 1e-5, bf16=bf)
    close(tag + " running_mean", log[:, 0], ref["running_mean"], e["running_mean"], **RS)
    close(tag + " running_var", log[:, 1], ref["running_var"], e["running_var"], rtol=1e-5)
    for g in range(G):
        assert torch.equal(acc[g, parity].cpu(), ds[g]["acc"]) and int(acc[g, 1 - parity].abs().sum()) == 0
        if form == "add":
            assert torch.equal(acc1[g, parity].cpu(), ds[g]["acc1"]) and int(acc1[g, 1 - parity].abs().sum()) == 0


@pytest.mark.parametrize("derived", [False, True])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_bn_relu_into_a_channel_slice(lib, dtn, derived):
    shape = R.SLICE_SHAPES[0]
    N, H, W, Cc = shape
    d = R.bn_inputs(dtn, shape)
    ref = cached(("bn", dtn, shape), lambda: R.bn_case(dtn, shape, names=R.BN_OUTPUTS))
    e = R.f32_err("bn", dtn, shape)
    td = TD[dtn]
    x = dev(d["x"], td)
    wide = nans(N * H * W + 1, R.SLICE_LDC, dtype=td)           # one more pixel row: the guard past the end
    acc, rm, rv = acc_pair(d["acc"], 0), dev(d["rm"]), dev(d["rv"])
    t = {k: dev(d[k]) for k in ("scale", "shift", "gamma", "beta")}
    src = dict(stat_acc=acc, gamma=t["gamma"], beta=t["beta"], running_mean=rm, running_var=rv, count=d["count"]) if derived else \
        dict(scale0=t["scale"], shift0=t["shift"])
    run(lib, [bn_op(L.OP_BN_RELU, dtn, shape, in0=x, out=wide.data_ptr() + R.SLICE_OFF * wide.element_size(), ldc=R.SLICE_LDC, **src)])
    form = "relu_derived" if derived else "relu"
    got = wide[:-1, R.SLICE_OFF:R.SLICE_OFF + Cc].reshape(shape)
    close("slice %s %s" % (dtn, form), got, ref[form], e[form], atol=1e-5, bf16=dtn == "bf16")
    assert all_nan(wide[:, :R.SLICE_OFF]) and all_nan(wide[:, R.SLICE_OFF + Cc:]) and all_nan(wide[-1])
    if derived:
        check_running("slice %s" % dtn, rm, rv, ref, e)
        assert int(acc[1].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------- B. pools

@pytest.mark.parametrize("dtn,shape", [(dn, s) for dn in ("f32", "bf16") for s in R.POOL_SHAPES] + [("f32", R.POOL_LARGE)],
                         ids=lambda v: sid(v))
def test_bn_relu_maxpool(lib, dtn, shape):
    N, H, W, Cc = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = R.bn_inputs(dtn, shape)
    ref = cached(("pool", dtn, shape), lambda: R.bn_case(dtn, shape, names=("pool", "pool_derived")))
    e = R.f32_err("pool", dtn, shape)
    td, bf, tag = TD[dtn], dtn == "bf16", "maxpool %s %s" % (dtn, sid(shape))
    x = dev(d["x"], td)
    t = {k: dev(d[k]) for k in ("scale", "shift", "gamma", "beta")}
    geo = dict(in0=x, Hin=H, Win=W, Hout=Ho, Wout=Wo)
    flat, y = guarded((N, Ho, Wo, Cc), td)
    run(lib, [bn_op(L.OP_BN_RELU_MAXPOOL, dtn, shape, out=y, scale0=t["scale"], shift0=t["shift"], **geo)])
    close(tag, y, ref["pool"], e["pool"], atol=1e-5, bf16=bf)
    assert all_nan(flat[y.numel():])
    acc, rm, rv = acc_pair(d["acc"], 1), dev(d["rm"]), dev(d["rv"])
    flat, y = guarded((N, Ho, Wo, Cc), td)
    run(lib, [bn_op(L.OP_BN_RELU_MAXPOOL, dtn, shape, out=y, stat_acc=acc, gamma=t["gamma"], beta=t["beta"], running_mean=rm,
                    running_var=rv, count=d["count"], **geo)], 1)
    close(tag + " derived", y, ref["pool_derived"], e["pool_derived"], atol=1e-5, bf16=bf)
    check_running(tag, rm, rv, ref, e)
    assert all_nan(flat[y.numel():]) and int(acc[0].abs().sum()) == 0 and torch.equal(acc[1].cpu(), d["acc"])
    # every normalised value negative: the output is exactly +0
    flat, y = guarded((N, Ho, Wo, Cc), td)
    run(lib, [bn_op(L.OP_BN_RELU_MAXPOOL, dtn, shape, out=y, scale0=dev(torch.ones(Cc)), shift0=dev(torch.full((Cc,), -100.0)), **geo)])
    assert int(bits(y).abs().sum()) == 0 and all_nan(flat[y.numel():])


@pytest.mark.parametrize("Cc", R.AVG_C)
@pytest.mark.parametrize("N", R.AVG_N)
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_avgpool_tail_loop(lib, dtn, N, Cc):
    for HW in R.AVG_HW:
        x = R.avgpool_inputs(dtn, N, HW, Cc)
        flat, y = guarded((N, Cc))
        xd = dev(x, TD[dtn])
        run(lib, [L.op(L.OP_AVGPOOL, DT[dtn], in0=xd, out=y, N=N, Hin=HW, Win=1, Cout=Cc)])
        close("avgpool %s N %d HW %d C %d" % (dtn, N, HW, Cc), y, R.avgpool(x.double()), R.f32_err("avg", dtn, N, HW, Cc)["out"], atol=1e-5)
        assert all_nan(flat[y.numel():])


# ---------------------------------------------------------------------------------------------- C. statistics

FIN_TOL = dict(scale=dict(rtol=2e-5), shift=dict(rtol=2e-4, atol=2e-5), running_mean=RS, running_var=dict(rtol=1e-5))


def fin_op(d, Cc, tiles, part, training, rm, rv, sc, sh):
    return L.op(L.OP_BN_FINALIZE, L.SAT_F32, stat_partial=part, gamma=d["gd"], beta=d["bd"], running_mean=rm, running_var=rv,
                scale_out=sc, shift_out=sh, Cout=Cc, count=d["count"], tiles_m=tiles, training=training, momentum=R.BN_MOMENTUM,
                eps=R.BN_EPS)


def finalize_modes(lib, tag, d, ref, e, tiles, Cc):
    d["gd"], d["bd"] = dev(d["gamma"]), dev(d["beta"])
    part = dev(d["partial"])
    # training, running statistics given
    rm, rv, (f1, sc), (f2, sh) = dev(d["rm"]), dev(d["rv"]), guarded((Cc,)), guarded((Cc,))
    run(lib, [fin_op(d, Cc, tiles, part, 1, rm, rv, sc, sh)])
    for k, got in (("scale", sc), ("shift", sh), ("running_mean", rm), ("running_var", rv)):
        close("%s %s" % (tag, k), got, ref[k], e[k], **FIN_TOL[k])
    assert all_nan(f1[Cc:]) and all_nan(f2[Cc:])
    # training, no running statistics: the same table, bit for bit
    (f1, sc2), (f2, sh2) = guarded((Cc,)), guarded((Cc,))
    run(lib, [fin_op(d, Cc, tiles, part, 1, None, None, sc2, sh2)])
    assert same_bits(sc2, sc) and same_bits(sh2, sh) and all_nan(f1[Cc:]) and all_nan(f2[Cc:])
    # training = 0: the table of the running statistics; the slabs (NaN) are never read, the statistics keep their bits
    rm, rv, (f1, sc), (f2, sh) = dev(d["rm"]), dev(d["rv"]), guarded((Cc,)), guarded((Cc,))
    run(lib, [fin_op(d, Cc, tiles, nans(tiles, 2, Cc), 0, rm, rv, sc, sh)])
    close(tag + " eval scale", sc, ref["eval_scale"], e["eval_scale"], **FIN_TOL["scale"])
    close(tag + " eval shift", sh, ref["eval_shift"], e["eval_shift"], **FIN_TOL["shift"])
    assert same_bits(rm.cpu(), d["rm"]) and same_bits(rv.cpu(), d["rv"]) and all_nan(f1[Cc:]) and all_nan(f2[Cc:])
    return sc


@pytest.mark.parametrize("Cc", R.FIN_C)
@pytest.mark.parametrize("tiles", R.FIN_TILES)
def test_bn_finalize_tiles_channels_modes(lib, tiles, Cc):
    d = R.finalize_inputs(tiles, Cc)
    ref = R.finalize_case(tiles, Cc)
    # the constant channel: variance exactly 0 in float64 too
    assert ref["scale"][1].item() == d["gamma"][1].double().item() / np.sqrt(R.f32v(R.BN_EPS))
    finalize_modes(lib, "finalize tiles %d C %d" % (tiles, Cc), d, ref, R.f32_err("fin", tiles, Cc), tiles, Cc)


@pytest.mark.parametrize("Cc", R.FIN_C)
def test_bn_finalize_count_of_one(lib, Cc):
    d = R.finalize_inputs(1, Cc, rows=1)
    assert d["count"] == 1
    finalize_modes(lib, "finalize count 1 C %d" % Cc, d, R.finalize_case(1, Cc, rows=1), R.f32_err("fin_count1", Cc), 1, Cc)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("tiles", R.SLAB_TILES)
def test_slab_reducer_adds_exact_integers(lib, tiles, groups):
    Cc = R.SLAB_C
    part, start = R.slab_inputs(tiles, Cc, groups)
    pd = dev(part)
    for parity in (0, 1):
        acc = start.clone().cuda()                                   # [G][2 parities][2][C]
        run(lib, [L.op(L.OP_BN_FINALIZE, L.SAT_F32, stat_partial=pd, stat_acc=acc, tiles_m=tiles, Cout=Cc, groups=groups)], parity)
        for g in range(groups):
            assert torch.equal(acc[g, parity].cpu(), start[g, parity] + R.slabs_to_acc(part[g])), (tiles, g, parity)
            assert torch.equal(acc[g, 1 - parity].cpu(), start[g, 1 - parity])


def device_items(items):
    raw = bytes(items)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def test_bn_eval_batch_equals_finalize_and_running_apply_is_exact(lib):
    g = R.gen(12)
    n = len(R.EVAL_C)
    host = [dict(gamma=torch.rand(c, generator=g) + 0.5, beta=torch.randn(c, generator=g) * 0.1, rm=torch.randn(c, generator=g) * 0.2,
                 rv=torch.rand(c, generator=g) + 0.5, bm=torch.randn(c, generator=g), bv=torch.rand(c, generator=g) * 2) for c in R.EVAL_C]
    dv = [{k: dev(v) for k, v in h.items()} for h in host]
    outs = [(guarded((c,)), guarded((c,))) for c in R.EVAL_C]
    items = (L.SatBnEvalItem * n)()
    for it, d, ((_, sc), (_, sh)), c in zip(items, dv, outs, R.EVAL_C):
        it.gamma, it.beta, it.running_mean, it.running_var = (d[k].data_ptr() for k in ("gamma", "beta", "rm", "rv"))
        it.scale_out, it.shift_out, it.C = sc.data_ptr(), sh.data_ptr(), c
    di = device_items(items)
    run(lib, [L.op(L.OP_BN_EVAL_BATCH, L.SAT_F32, in0=di, count=n, eps=R.BN_EPS)])
    for h, d, ((f1, sc), (f2, sh)), c in zip(host, dv, outs, R.EVAL_C):
        ref = R.bn_finalize(None, 1, h["gamma"], h["beta"], h["rm"], h["rv"], R.BN_MOMENTUM, R.BN_EPS, 0)
        r32 = R.bn_finalize(None, 1, h["gamma"], h["beta"], h["rm"], h["rv"], R.BN_MOMENTUM, R.BN_EPS, 0, R.F32)
        close("eval batch C %d scale" % c, sc, ref["scale"], R.max_err(r32["scale"], ref["scale"]), **FIN_TOL["scale"])
        close("eval batch C %d shift" % c, sh, ref["shift"], R.max_err(r32["shift"], ref["shift"]), **FIN_TOL["shift"])
        sc2, sh2 = nans(c), nans(c)
        run(lib, [L.op(L.OP_BN_FINALIZE, L.SAT_F32, gamma=d["gamma"], beta=d["beta"], running_mean=d["rm"], running_var=d["rv"],
                       scale_out=sc2, shift_out=sh2, Cout=c, count=1, tiles_m=1, training=0, momentum=R.BN_MOMENTUM, eps=R.BN_EPS)])
        assert same_bits(sc, sc2) and same_bits(sh, sh2), "eval table != finalize(training = 0) at C = %d" % c
        assert all_nan(f1[c:]) and all_nan(f2[c:])
        assert same_bits(d["rm"].cpu(), h["rm"]) and same_bits(d["rv"].cpu(), h["rv"])
    # the deferred running-statistics update: one f64 expression, rounded once
    run_items = (L.SatBnRunningItem * n)()
    flats = [(guarded((c,)), guarded((c,))) for c in R.EVAL_C]
    for it, h, d, ((_, rm), (_, rv)), c in zip(run_items, host, dv, flats, R.EVAL_C):
        rm.copy_(d["rm"])
        rv.copy_(d["rv"])
        it.running_mean, it.running_var, it.batch_mean, it.batch_var, it.C = rm.data_ptr(), rv.data_ptr(), d["bm"].data_ptr(), d["bv"].data_ptr(), c
    di2 = device_items(run_items)
    L.check(lib.sat_bn_running_apply(di2.data_ptr(), n, R.BN_MOMENTUM, st()))
    sync()
    for h, ((f1, rm), (f2, rv)), c in zip(host, flats, R.EVAL_C):
        wm, wv = R.running_apply(h["rm"], h["rv"], h["bm"], h["bv"], R.BN_MOMENTUM)
        assert same_bits(rm.cpu(), wm) and same_bits(rv.cpu(), wv), "running apply at C = %d" % c
        assert all_nan(f1[c:]) and all_nan(f2[c:])


# ---------------------------------------------------------------------------------------------- D. cross entropy, column sums

def ce_call(lib, logits, targets, V, ldl, write_grad, offset=0, inv=R.CE_INV):
    """logits [N, V] into a NaN buffer of pitch ldl starting `offset` floats into an aligned allocation; returns the buffer before
    and after, the view of the rows, the row losses (+ guard) and the loss (+ guard)"""
    N = logits.shape[0]
    buf = nans(offset + N * ldl + GUARD)
    view = buf[offset:offset + N * ldl].view(N, ldl)
    view[:, :V] = logits.cuda()
    before = buf.clone()
    rl, lo, tg = nans(N + 1), nans(2), targets.cuda()
    L.check(lib.sat_ce_rows(buf.data_ptr() + 4 * offset, ldl, L.ptr(tg), N, V, inv, write_grad, L.ptr(rl), L.ptr(lo), st()), "sat_ce_rows")
    sync()
    return before, buf, view, rl, lo


@pytest.mark.parametrize("V", R.CE_V)
def test_ce_rows_paths_tails_and_placed_targets(lib, V):
    logits, targets, _ = R.ce_inputs(V)
    ref = cached(("ce", V), lambda: R.ce_rows(logits.double(), targets, R.CE_INV))
    e = R.f32_err("ce", V)
    N = logits.shape[0]
    variants = [(ldl, 0) for ldl in sorted({L.pad4(V), V, V + 4})] + [(L.pad4(V), 1)]
    for ldl, offset in variants:
        for write_grad in (1, 0):
            tag = "ce V %d ldl %d%s grad %d" % (V, ldl, " base+1" if offset else "", write_grad)
            before, buf, view, rl, lo = ce_call(lib, logits, targets, V, ldl, write_grad, offset)
            close(tag + " row_loss", rl[:N], ref["row_loss"], e["row_loss"])
            close(tag + " loss", lo[:1], ref["loss"].reshape(1), e["loss"], rtol=1e-5)
            assert all_nan(rl[N:]) and all_nan(lo[1:])
            if write_grad:
                close(tag + " grad", view[:, :V], ref["grad"], e["grad"], atol=2e-8 + 1e-6 * R.CE_INV)
                view[:, :V] = before[offset:offset + N * ldl].view(N, ldl)[:, :V]         # then only pads and guards can differ
            assert same_bits(buf, before), tag + ": pads, guards or (write_grad = 0) logits changed"


@pytest.mark.parametrize("N", R.CE_LOSS_N)
def test_ce_loss_out_over_row_counts(lib, N):
    logits, targets = R.ce_loss_inputs(N)
    ref, e = R.ce_rows(logits.double(), targets, R.CE_INV), R.f32_err("ce_loss", N)
    V = R.CE_LOSS_V
    before, buf, view, rl, lo = ce_call(lib, logits, targets, V, L.pad4(V), 1)
    close("ce N %d row_loss" % N, rl[:N], ref["row_loss"], e["row_loss"])
    close("ce N %d loss" % N, lo[:1], ref["loss"].reshape(1), e["loss"], rtol=1e-5)
    close("ce N %d grad" % N, view[:, :V], ref["grad"], e["grad"], atol=2e-8 + 1e-6 * R.CE_INV)
    assert all_nan(rl[N:]) and all_nan(lo[1:]) and all_nan(view[:, V:])


def test_ce_rows_weighted_tail_targets_and_zero_weight_rows(lib):
    d = R.ce_weighted_inputs()
    B, T, V, N = d["B"], d["T"], d["V"], d["B"] * d["T"]
    live = d["w"] != 0
    ref = R.ce_rows(d["logits"][live].double(), d["targets"][live], d["w"][live])
    e = R.f32_err("ce_weighted")
    ldl = L.pad4(V)
    for write_grad in (1, 0):
        buf = nans(N * ldl + GUARD)
        view = buf[:N * ldl].view(N, ldl)
        view[:, :V] = d["logits"].cuda()
        before = buf.clone()
        rl, lo, ids, w = nans(N + 1), nans(2), d["ids"].cuda(), d["w"].cuda()
        L.check(lib.sat_ce_rows_weighted(L.ptr(buf), ldl, L.ptr(ids), d["ids"].shape[1], B, N, V, L.ptr(w), write_grad, L.ptr(rl),
                                         L.ptr(lo), st()), "sat_ce_rows_weighted")
        sync()
        close("ce weighted row_loss", rl[:N][live.cuda()], ref["row_loss"], e["row_loss"])
        close("ce weighted loss", lo[:1], ref["loss"].reshape(1), e["loss"], rtol=1e-5)
        assert all_nan(rl[N:]) and all_nan(lo[1:])
        if write_grad:
            close("ce weighted grad", view[:, :V][live.cuda()], ref["grad"], e["grad"], atol=2e-8 + 1e-6 * d["w"].abs().max().item())
            dead = view[:, :V][(~live).cuda()]
            assert dead.shape[0] == 2 and int(bits(dead).abs().sum()) == 0, "a zero-weight row's gradient is exactly +0"
            view[:, :V] = before[:N * ldl].view(N, ldl)[:, :V]
        assert same_bits(buf, before)


@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_unroll_boundary(lib, rows):
    for cols in R.COLSUM_COLS:
        x = R.colsum_inputs(rows, cols)
        for ld in (cols, cols + 5):
            xd = nans(rows + 1, ld)
            xd[:rows, :cols] = x.cuda()
            flat, out = guarded((cols,))
            L.check(lib.sat_colsum_f32(L.ptr(xd), ld, rows, cols, L.ptr(out), st()), "sat_colsum_f32")
            sync()
            close("colsum %d x %d ld %d" % (rows, cols, ld), out, x.double().sum(0), R.f32_err("colsum", rows, cols)["out"], atol=1e-7)
            assert all_nan(flat[cols:])


# ---------------------------------------------------------------------------------------------- E. clamp + Adam

def adam_buffers(d, n):
    out = {}
    for k in ("p", "g", "m", "v"):
        flat, view = guarded((n,))
        if k != "g":
            view.copy_(d[k])
        out[k] = (flat, view)
    return out


def adam_call(lib, b, n, clip, step, skip=None):
    hp = R.ADAM_HP
    args = [b[k][0].data_ptr() for k in ("p", "g", "m", "v")] + [n, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], clip, step]
    if skip is None:
        L.check(lib.sat_clamp_adam_step(*args, st()), "sat_clamp_adam_step")
    else:
        L.check(lib.sat_clamp_adam_step_guarded(*args, L.ptr(skip), st()), "sat_clamp_adam_step_guarded")
    sync()


@pytest.mark.parametrize("clip", R.ADAM_CLIP)
@pytest.mark.parametrize("n", R.ADAM_N)
def test_clamp_adam_three_steps_from_nonzero_moments(lib, n, clip):
    d = R.adam_inputs(n)
    ref = cached(("adam", n, clip), lambda: R.adam_case(n, clip))
    e = R.f32_err("adam", n, clip)
    b = adam_buffers(d, n)
    for step in (1, 2, 3):
        tag = "adam n %d clip %g step %d" % (n, clip, step)
        b["g"][1].copy_(d["grads"][step - 1])
        adam_call(lib, b, n, clip, step)
        r = ref[step - 1]
        assert torch.equal(b["g"][1].cpu().double(), r["g"]), tag + ": the clamp is exact"
        close(tag + " p", b["p"][1], r["p"], e["p"], atol=2e-7)
        close(tag + " m", b["m"][1], r["m"], e["m"])
        close(tag + " v", b["v"][1], r["v"], e["v"])
        assert all(all_nan(b[k][0][n:]) for k in b), tag + ": wrote past element n"


@pytest.mark.parametrize("n", [5, 1023])
def test_clamp_adam_guarded_skip_word(lib, n):
    d = R.adam_inputs(n)
    plain, guard0, guard1 = adam_buffers(d, n), adam_buffers(d, n), adam_buffers(d, n)
    for b in (plain, guard0, guard1):
        b["g"][1].copy_(d["grads"][0])
    before = {k: guard1[k][0].clone() for k in guard1}
    adam_call(lib, plain, n, 0.1, 1)
    adam_call(lib, guard0, n, 0.1, 1, skip=torch.zeros(1, device="cuda"))
    adam_call(lib, guard1, n, 0.1, 1, skip=torch.full((1,), 3.0, device="cuda"))
    for k in plain:
        assert same_bits(guard0[k][0], plain[k][0]), "skip word 0: the unguarded step"
        assert same_bits(guard1[k][0], before[k]), "non-zero skip word: %s changed" % k
    assert not same_bits(plain["p"][0], before["p"])


# ---------------------------------------------------------------------------------------------- F. BatchNorm1d head

@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("shape", R.BN1D_SHAPES, ids=sid)
def test_fc_bn1d_fwd_bwd(lib, shape, training):
    B, Fd, E = shape
    d = R.bn1d_inputs(*shape)
    ref = cached(("bn1d", shape, training), lambda: R.bn1d_case(shape, training))
    e = R.f32_err("bn1d", shape, training)
    tag = "bn1d %s training %d" % (sid(shape), training)
    dv = {k: dev(v) for k, v in d.items()}
    (f1, feats), (f2, xhat), (f3, rstd) = guarded((B, E)), guarded((B, E)), guarded((E,))
    wsb = lib.sat_fc_bn1d_ws_bytes(B, Fd, E)
    ws = nans(max(wsb // 4, B * E))
    L.check(lib.sat_fc_bn1d_fwd(L.ptr(dv["pooled"]), L.ptr(dv["w"]), L.ptr(dv["b"]), L.ptr(dv["gamma"]), L.ptr(dv["beta"]), L.ptr(dv["rm"]),
                                L.ptr(dv["rv"]), R.BN1D_MOMENTUM, R.BN_EPS, training, B, Fd, E, L.ptr(feats), L.ptr(xhat), L.ptr(rstd),
                                L.ptr(ws), ws.numel() * 4, st()), "sat_fc_bn1d_fwd")
    sync()
    close(tag + " feats", feats, ref["feats"], e["feats"], atol=2e-5)
    close(tag + " xhat", xhat, ref["xhat"], e["xhat"])
    close(tag + " rstd", rstd, ref["rstd"], e["rstd"])
    if training:
        close(tag + " running_mean", dv["rm"], ref["running_mean"], e["running_mean"], rtol=1e-5, atol=1e-7)
        close(tag + " running_var", dv["rv"], ref["running_var"], e["running_var"], rtol=1e-5, atol=1e-7)
    else:
        assert same_bits(dv["rm"].cpu(), d["rm"]) and same_bits(dv["rv"].cpu(), d["rv"]), "eval mode changed the running statistics"
    assert all_nan(f1[B * E:]) and all_nan(f2[B * E:]) and all_nan(f3[E:])
    # backward from the float32 values of the reference tape (the kernel's own operands), every output NaN first
    xh, rs = dev(ref["xhat"].float()), dev(ref["rstd"].float())
    (g1, dw), (g2, db), (g3, dg), (g4, dbe) = guarded((E, Fd)), guarded((E,)), guarded((E,)), guarded((E,))
    ws = nans(max(wsb // 4, B * E))
    L.check(lib.sat_fc_bn1d_bwd(L.ptr(dv["dy"]), L.ptr(dv["pooled"]), L.ptr(xh), L.ptr(rs), L.ptr(dv["gamma"]), B, Fd, E, L.ptr(dw),
                                L.ptr(db), L.ptr(dg), L.ptr(dbe), L.ptr(ws), ws.numel() * 4, st()), "sat_fc_bn1d_bwd")
    sync()
    close(tag + " dgamma", dg, ref["dgamma"], e["dgamma"], rtol=1e-4, atol=1e-5)
    close(tag + " dbeta", dbe, ref["dbeta"], e["dbeta"], rtol=1e-4, atol=1e-5)
    close(tag + " dw", dw, ref["dw"], e["dw"], rtol=1e-3, atol=2e-5)
    close(tag + " db", db, ref["db"], e["db"], atol=5e-4)
    assert all_nan(g1[E * Fd:]) and all_nan(g2[E:]) and all_nan(g3[E:]) and all_nan(g4[E:])


# ---------------------------------------------------------------------------------------------- G. embedding and ids

@pytest.mark.parametrize("name", list(R.EMBED_CASES))
def test_embedding_gather_scatter_and_ids(lib, name):
    d = R.embed_inputs(name)
    B, T, E, V, N, bs = d["B"], d["T"], d["E"], d["V"], d["N"], d["bs"]
    cap, stride = d["captions"].cuda(), d["captions"].shape[1]
    capp = None if T == 1 else L.ptr(cap)                              # T = 1: no token rows, captions may be NULL
    prefix, feats, emb, dX = d["prefix"].cuda(), dev(d["features"]), dev(d["embed"]), dev(d["dX"])
    # gather: bit-exact
    flat, X = guarded((N, E))
    L.check(lib.sat_embed_concat_fwd(L.ptr(feats), L.ptr(emb), capp, stride, L.ptr(prefix), T, N, B, E, V, L.ptr(X), st()), "embed fwd")
    sync()
    assert same_bits(X.cpu(), R.embed_concat_fwd(d["features"], d["embed"], d["captions"], bs)) and all_nan(flat[N * E:])
    # scatter: float64, and bit for bit the float32 sum in row order
    (f1, de), (f2, df) = guarded((V, E)), guarded((B, E))
    L.check(lib.sat_embed_concat_bwd(L.ptr(dX), capp, stride, L.ptr(prefix), T, N, B, E, V, L.ptr(de), L.ptr(df), st()), "embed bwd")
    sync()
    df64, de64 = R.embed_concat_bwd(d["dX"], d["captions"], bs, V)
    df32, de32 = R.embed_concat_bwd(d["dX"], d["captions"], bs, V, row_ordered_f32=True)
    close("embed %s d_embed" % name, de, de64, R.f32_err("embed", name)["d_embed"])
    assert same_bits(de.cpu(), de32), "d_embed is not the row-ordered float32 sum"
    assert same_bits(df.cpu(), df32) and all_nan(f1[V * E:]) and all_nan(f2[B * E:])
    # one step's rows by id, ids read with a stride
    if T > 1:
        col = min(1, T - 1)
        flat, out = guarded((B, E))
        L.check(lib.sat_embed_rows(L.ptr(emb), cap.data_ptr() + 8 * col, stride, B, E, V, L.ptr(out), st()), "embed rows")
        sync()
        assert same_bits(out.cpu(), d["embed"][d["captions"][:, col].clamp(0, V - 1)]) and all_nan(flat[B * E:])
    # packed targets
    tg = torch.full((N + 1,), -7, dtype=torch.int64, device="cuda")
    L.check(lib.sat_pack_targets(L.ptr(cap), stride, L.ptr(prefix), T, N, L.ptr(tg), st()), "pack targets")
    sync()
    assert torch.equal(tg[:N].cpu(), R.pack_targets(d["captions"], bs)) and tg[N].item() == -7
    # the range check reports what the kernels above only clamp
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    L.check(lib.sat_validate_ids(L.ptr(cap), stride, B, stride, 0, V, L.ptr(status), st()), "validate ids")
    sync()
    bad = bool(((d["captions"] < 0) | (d["captions"] >= V)).any())
    assert status.cpu().tolist() == [int(bad), 0] and bad == (name == "clamped")
