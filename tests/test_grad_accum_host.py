"""Host side of gradient accumulation (csrc/sat_optim.hip: sat_grad_accumulate; optim.py, trainer.py); no GPU.

The yardstick first (grad_accum_reference against numpy's own float32 arithmetic), then the C ABI (symbol, argument errors before
any launch), the argument checks of the new TrainStep entry points, and `DataParallelStep.step_accumulated` over gloo with a CPU
engine built on oracle/: two ranks with K = 2 micro-batches each equal the single-process update on the union, with exactly one
all-reduce per bucket and update."""
import importlib
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import grad_accum_reference as A
from flat_adam_host import bare
from oracle import decoder as OD
from oracle import train_step as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

ARG = 1001
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------- 1. the yardstick

def test_reference_is_numpy_float32_where_that_is_exact():
    a, g = A.inputs(1027, 2)
    first, other = A.fold(a, g, 1.0, True)
    assert np.array_equal(first[:-1].view(np.uint32), g[:-1].view(np.uint32)) and np.array_equal(first, other)
    summed, _ = A.fold(a, g, 1.0, False)
    assert np.array_equal(summed[:-1].view(np.uint32), (a[:-1] + g[:-1]).view(np.uint32))
    half, _ = A.fold(g, g, 0.5, True)
    back, _ = A.fold(half, g, 0.5, False)
    assert np.array_equal(back[:-1].view(np.uint32), g[:-1].view(np.uint32))


def test_reference_midpoint_and_fault_table():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    # 1 + 2^-24 sits on the midpoint of 1 and 1 + 2^-23: both neighbours pass, the expected one is the tie to even
    acc, g = np.array([one, 0, 0], np.float32), np.array([np.float32(2.0 ** -24), 0, 0], np.float32)
    r, o = A.fold(acc, g, 1.0, False)
    assert r[0] == one and o[0] == up and A.matches([up, 0, 0], r, o).all()
    r, o = A.fold(acc, np.array([0.25, 0, 0], np.float32), 1.0, False)
    assert r[0] == np.float32(1.25) and o[0] == r[0]
    for first in (True, False):
        for aw in (0.0, 1.0):
            for gw in (0.0, 1.0):
                assert A.fault(first, aw, gw) == (1.0 if (gw or (aw and not first)) else 0.0)
    assert A.fault(False, 2.0, 0.0) == 1.0 and A.fault(True, NAN, 0.0) == 0.0 and A.fault(False, -0.0, 0.0) == 0.0
    assert A.grid(1) == 1 and A.grid(A.SPAN + 2) == 1 and A.grid(A.SPAN + 3) == 2 and A.grid(A.SIZES[-1]) == A.GRID_CAP


# ---------------------------------------------------------------------------------------------- 2. the symbol

def test_new_symbol_is_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    lib = L.load()
    name = "sat_grad_accumulate"
    assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name)
    fn = getattr(lib, name)
    assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0] and len(fn.argtypes) == 6
    assert lib.sat_version() == L.ABI_VERSION == 18
    src = open(os.path.join(ROOT, "show-and-tell_amd", "csrc", "sat_optim.hip")).read()
    assert "OPT_BLOCK = %d" % A.BLOCK in src and "OPT_GRID_CAP = %d" % A.GRID_CAP in src and "f32x4" in src


def test_argument_errors_come_back_before_any_launch():
    """no GPU here: every call below must return SAT_ERR_ARG without launching (fake non-null addresses are never dereferenced)"""
    lib = L.load()
    P, Q = 4096, 1 << 20

    def call(acc=P, g=Q, n=100, weight=1.0, first=0):
        return lib.sat_grad_accumulate(acc, g, n, weight, first, None)

    for kw in (dict(acc=None), dict(g=None), dict(n=-1), dict(n=-(1 << 40)), dict(acc=P + 4), dict(acc=P + 8), dict(g=Q + 4),
               dict(g=Q + 12), dict(weight=NAN), dict(weight=INF), dict(weight=-INF), dict(g=P), dict(g=P + 16, n=100),
               dict(acc=P + 400, g=P, n=100), dict(acc=Q, g=Q - 16, n=3), dict(weight=NAN, first=1), dict(acc=None, first=1)):
        assert call(**kw) == ARG, kw


# ---------------------------------------------------------------------------------------------- 3. argument checks

def test_accumulate_refuses_a_weight_that_is_not_a_finite_number():
    ts = bare(sat.TrainStep)
    assert ts.accumulated == 0
    for bad in (NAN, INF, -INF, True, None, "1", [1.0]):
        with pytest.raises(ValueError, match="weight"):
            ts.accumulate(bad)
    assert ts.accumulated == 0
    ts._averaged = True
    with pytest.raises(RuntimeError, match="averaged"):
        ts.accumulate()
    ts.discard_accumulated()
    assert ts.accumulated == 0


def test_mixed_step_refuses_an_rl_weight_outside_the_unit_interval():
    ts = object.__new__(sat.TrainStep)
    for bad in (-0.1, 1.5, NAN, INF, True, None, "0.5"):
        with pytest.raises(ValueError, match="rl_weight"):
            ts.mixed_step(None, None, [3], None, None, bad)
    with pytest.raises(TypeError, match="unexpected"):
        ts.mixed_step(None, None, [3], None, None, 0.5, beam=3)


def test_step_accumulated_refuses_an_empty_sequence():
    ts = object.__new__(sat.TrainStep)
    with pytest.raises(ValueError, match="at least one"):
        ts.step_accumulated([])
    dp = object.__new__(sat.DataParallelStep)
    dp.engine, dp.dist = ts, dist
    with pytest.raises(ValueError, match="at least one"):
        dp.step_accumulated([], 10)


def test_nothing_new_is_exported_and_the_buffer_starts_absent():
    assert not hasattr(sat, "grad_accumulate") and not hasattr(sat, "check_accumulate_weight")
    assert isinstance(sat.TrainStep.accumulated, property) and sat.TrainStep._accumulated == 0
    for name in ("accumulate", "discard_accumulated", "step_accumulated", "mixed_step"):
        assert callable(getattr(sat.TrainStep, name)), name
    assert callable(sat.DataParallelStep.step_accumulated)


# ---------------------------------------------------------------------------------------------- 4. two ranks over gloo

DIMS = dict(E=16, H=24, V=120, L=1)
LENGTHS = [12, 12, 11, 10, 9, 9, 8, 7, 6, 5, 4, 3]
K = 2


class AccumulatingOracleEngine:
    """The engine interface `DataParallelStep.step_accumulated` needs, arithmetic from oracle/ (tests only): test_dp_gloo.py's
    OracleEngine plus accumulate / acc_grad / accumulated and an optimizer_step that reads the accumulated buffer while one is open"""

    def __init__(self, params):
        self.params = params
        self.offsets, off = {}, 0
        groups = [[n for n in params if n.startswith("linear")], [n for n in params if n.startswith("lstm")],
                  [n for n in params if n.startswith("embed")]]
        self.buckets = []
        for g in groups:
            s = off
            for n in g:
                self.offsets[n] = off
                off += params[n].numel()
            self.buckets.append((s, off))
        self.buckets[-1] = (self.buckets[-1][0], off + 4)
        self.flat_grad = torch.zeros(off + 4)
        self.acc_grad = None
        self.accumulated = 0
        self.state = {}
        self.callbacks = 0

    def forward_backward(self, batch, inv_denom, on_bucket_ready=None):
        feats, caps, lengths = batch
        loss, grads, _, _ = OT.decoder_loss_and_grads(self.params, feats, caps, lengths, DIMS["L"], denom=1.0 / inv_denom)
        for n, g in grads.items():
            o = self.offsets[n]
            self.flat_grad[o:o + g.numel()] = g.reshape(-1)
        self.flat_grad[-4] = loss
        if on_bucket_ready:
            self.callbacks += 1
        return self.flat_grad[-4:-3]

    def accumulate(self, weight=1.0):
        if self.acc_grad is None:
            self.acc_grad = torch.full_like(self.flat_grad, NAN)           # the first fold must not read it
        n1 = self.flat_grad.numel() - 3                                    # gradients and the loss slot
        word = 1.0 if ((self.accumulated and self.acc_grad[n1] != 0) or self.flat_grad[n1] != 0) else 0.0
        if self.accumulated == 0:
            self.acc_grad[:n1] = weight * self.flat_grad[:n1]
            self.acc_grad[n1 + 1:] = 0.0
        else:
            self.acc_grad[:n1] += weight * self.flat_grad[:n1]
        self.acc_grad[n1] = word
        self.accumulated += 1

    def optimizer_step(self, lr=None):
        src = self.acc_grad if self.accumulated else self.flat_grad
        self.accumulated = 0
        grads = {n: src[self.offsets[n]:self.offsets[n] + p.numel()].view(p.shape).clone() for n, p in self.params.items()}
        OT.clamp_(grads, 0.1)
        OT.adam_step_(self.params, grads, self.state, lr=1e-3 if lr is None else lr)


class CountingDist:
    """torch.distributed with its all_reduce calls counted (sizes kept)"""

    def __init__(self):
        self.sizes = []
        self.ReduceOp = dist.ReduceOp

    def all_reduce(self, tensor, **kw):
        self.sizes.append(tensor.numel())
        return dist.all_reduce(tensor, **kw)

    def __getattr__(self, name):
        return getattr(dist, name)


def make_batch():
    g = torch.Generator().manual_seed(7)
    B, T = len(LENGTHS), LENGTHS[0]
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(LENGTHS):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, DIMS["V"], (l - 2,), generator=g)
        caps[b, l - 1] = 2
    return torch.randn(B, DIMS["E"], generator=g), caps


def fresh_params():
    return OD.init_decoder_params(DIMS["E"], DIMS["H"], DIMS["V"], DIMS["L"], generator=torch.Generator().manual_seed(5))


def worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    feats, caps = make_batch()
    eng = AccumulatingOracleEngine(fresh_params())
    dp = sat.DataParallelStep(eng)
    dp.dist = counter = CountingDist()
    losses = []
    for _ in range(2):
        f, c, ln, tokens = sat.dp_shard(feats, caps, LENGTHS, rank, world)
        micro = [sat.dp_shard(f, c, ln, k, K)[:3] for k in range(K)]
        assert sum(sum(l - 1 for l in m[2]) for m in micro) == sum(l - 1 for l in ln) and tokens == sum(l - 1 for l in LENGTHS)
        losses.append(float(dp.step_accumulated(micro, tokens)))
        assert eng.accumulated == 0
    if rank == 0:
        torch.save({"params": eng.params, "losses": losses, "reduces": counter.sizes, "callbacks": eng.callbacks,
                    "buckets": eng.buckets}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_of_two_micro_batches_equal_the_single_process_update_with_one_exchange(tmp_path):
    """tolerances: those test_dp_gloo.py applies to its own comparison of two ranks with the single process (loss 1e-5, parameters
    2e-6 absolute after two updates)"""
    out = str(tmp_path / "r0.pt")
    port = 33500 + os.getpid() % 2000
    mp.spawn(worker, args=(2, port, out), nprocs=2, join=True)
    got = torch.load(out)
    feats, caps = make_batch()
    params, state, ref_losses = fresh_params(), {}, []
    for _ in range(2):
        loss, grads, _, _ = OT.decoder_loss_and_grads(params, feats, caps, LENGTHS, DIMS["L"])
        ref_losses.append(loss.item())
        OT.clamp_(grads, 0.1)
        OT.adam_step_(params, grads, state, lr=1e-3)
    for a, b in zip(got["losses"], ref_losses):
        print("loss %.7f reference %.7f" % (a, b))
        assert abs(a - b) < 1e-5
    for k in params:
        assert torch.allclose(got["params"][k], params[k], rtol=0, atol=2e-6), k
    sizes = [e - s for s, e in got["buckets"]]
    assert got["reduces"] == sizes * 2, "one all-reduce per bucket and update, K = 2 micro-batches or not"
    assert got["callbacks"] == 0, "the micro-batches run without bucket callbacks"


def test_single_process_accumulation_issues_no_exchange():
    feats, caps = make_batch()
    eng = AccumulatingOracleEngine(fresh_params())
    dp = sat.DataParallelStep(eng)
    dp.dist = counter = CountingDist()
    assert dp.world == 1
    tokens = sum(l - 1 for l in LENGTHS)
    micro = [sat.dp_shard(feats, caps, LENGTHS, k, 3)[:3] for k in range(3)]
    loss = float(dp.step_accumulated(micro, tokens))
    ref, _, _, _ = OT.decoder_loss_and_grads(fresh_params(), feats, caps, LENGTHS, DIMS["L"])
    assert abs(loss - ref.item()) < 1e-6 and counter.sizes == [] and eng.accumulated == 0
