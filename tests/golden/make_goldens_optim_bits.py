#!/usr/bin/env python3
"""Generate tests/golden/optim/G15_flat_adam_bits.npz: the BITS the two optimizers (`sat.TrainStep`, `sat.FusedClampAdam`) leave in
their flat buffers, recorded before their update sequence, averaging and state dicts moved into one shared class, so that
tests/test_gpu_optim_bits.py can hold every later tree to them.

    python tests/golden/make_goldens_optim_bits.py [out_dir]          (needs the GPU and the built library)

Only public names are used (constructors, the settable attributes, `step` / `forward_backward` / `accumulate` / `optimizer_step` /
`check_ids`, the state dicts and the buffer attributes), so the script runs unchanged on any tree that has them.  Every kernel in
the path reduces in a fixed order, so two runs write the same bytes -- but the values are those of gfx950 and of the ROCm build
that recorded them; after a toolchain change the fixture is regenerated from a tree whose other optimizer tests pass.

`TrainStep` cases: the tiny engine of tests/test_gpu_grad_accum.py (TINY arch, E = H = 32, V = 53, one layer, f32 decoder mode) on
six cached [6, 32] feature rows, three updates unless stated:

    ts_defaults, ts_clip0 (grad_clip 0), ts_norm (max_grad_norm below the norm), ts_norm_inf, ts_decay (weight_decay 0.01, the 1-D
    parameters exempt), ts_norm_decay, ts_ema, ts_ema_warmup,
    ts_ema_norm_nan   a NaN written into the gradient in front of the second update: update and average dropped
    ts_accum          two folds of weight 0.5, one update
    ts_fault          update, then an update with the fault word set BY HAND in `fault_slot` (no kernel faults): dropped, the step
                      count rolled back when `check_ids()` raises, then one more update
    ts_state_dict     two updates with norm + decay + EMA, `optimizer_state_dict` into a fresh engine, one more update there

`FusedClampAdam` cases: parameters of shapes (2, 3), (3,), (5, 7), (1,) -- no size a multiple of 4 -- with seeded values and one
seeded gradient per step, three steps unless stated:

    fca_defaults, fca_clip (0.1, the gradients handed over as stray tensors), fca_norm, fca_decay (the 1-D parameters exempt),
    fca_none_first / _middle / _last   the parameter's `.grad` is None in steps two and three, under max_norm
    fca_ema_norm_nan  ema_decay 0.9 with max_norm and a NaN in the second step's gradient
    fca_state_dict    two steps with clip + norm + decay + EMA, `state_dict` into a fresh optimizer, one more step there

Arrays per case: <case>__params / __m / __v, __ema where an average is kept, __norm (`last_grad_norm`, f64 [2]) where a norm is
set, __steps (i64 [1]).  The FusedClampAdam buffers (52 floats) are stored as they are.  A TrainStep buffer has about 20 000
floats of full entropy, 48 buffers of them: they are stored as SHA-256 digests, u8 [1 + parameters, 32] -- row 0 over the bytes of
the whole buffer (padding included), one row per parameter slice in the order of sorted(flat.slices) -- so a difference in any
bit of any element changes the array and the failing row names the parameter."""
import hashlib
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import decoder as OD  # noqa: E402

NAME = "G15_flat_adam_bits.npz"
NAN = float("nan")

TINY = dict(layers=(1, 1, 1, 1), width=8)
DIM = dict(E=32, H=32, V=53, L=1)
LENGTHS = [9, 8, 7, 5, 4, 3]                 # whole captions, <start> included: 30 target tokens
INV_TOKENS = 1.0 / sum(l - 1 for l in LENGTHS)
LOW_NORM = 0.01                              # below the gradient norm of every update here (checked while recording)

# case: (constructor keywords, attributes, script)
TS_CASES = dict(
    ts_defaults=({}, {}, "three"),
    ts_clip0=(dict(grad_clip=0), {}, "three"),
    ts_norm=({}, dict(max_grad_norm=LOW_NORM), "three"),
    ts_norm_inf=({}, dict(max_grad_norm=float("inf")), "three"),
    ts_decay=({}, dict(weight_decay=0.01, no_decay=True), "three"),
    ts_norm_decay=({}, dict(max_grad_norm=LOW_NORM, weight_decay=0.01, no_decay=True), "three"),
    ts_ema=({}, dict(ema_decay=0.9), "three"),
    ts_ema_warmup=({}, dict(ema_decay=0.9, ema_warmup=True), "three"),
    ts_ema_norm_nan=({}, dict(ema_decay=0.9, max_grad_norm=LOW_NORM), "nan"),
    ts_accum=({}, {}, "accum"),
    ts_fault=({}, dict(ema_decay=0.9), "fault"),
    ts_state_dict=({}, dict(max_grad_norm=LOW_NORM, weight_decay=0.01, no_decay=True, ema_decay=0.9), "state_dict"),
)

SHAPES = [(2, 3), (3,), (5, 7), (1,)]
# case: (constructor keywords, ema_decay, script)
FCA_CASES = dict(
    fca_defaults=({}, 0.0, "three"),
    fca_clip=(dict(clip=0.1), 0.0, "stray"),
    fca_norm=(dict(max_norm=0.05), 0.0, "three"),
    fca_decay=(dict(weight_decay=0.01, no_decay=True), 0.0, "three"),
    fca_none_first=(dict(max_norm=0.05), 0.0, "none0"),
    fca_none_middle=(dict(max_norm=0.05), 0.0, "none2"),
    fca_none_last=(dict(max_norm=0.05), 0.0, "none3"),
    fca_ema_norm_nan=(dict(max_norm=0.05), 0.9, "nan"),
    fca_state_dict=(dict(clip=0.1, max_norm=0.05, weight_decay=0.01, no_decay=True), 0.9, "state_dict"),
)


def fields(name):
    """the arrays case `name` records"""
    if name in TS_CASES:
        _, attrs, _ = TS_CASES[name]
        ema, norm = "ema_decay" in attrs, "max_grad_norm" in attrs
    else:
        kw, decay, _ = FCA_CASES[name]
        ema, norm = decay > 0, "max_norm" in kw
    return ("params", "m", "v") + (("ema",) if ema else ()) + (("norm",) if norm else ()) + ("steps",)


# ---------------------------------------------------------------------------------------------- TrainStep

def engine(sat, kw, attrs):
    torch.manual_seed(1)                                     # (the encoder head's parameters live in the flat buffer too)
    model = sat.ShowAndTell(DIM["E"], DIM["H"], DIM["V"], DIM["L"], arch=TINY, compute_dtype="f32")
    model.decoder.load_state_dict(OD.init_decoder_params(DIM["E"], DIM["H"], DIM["V"], DIM["L"],
                                                         generator=torch.Generator().manual_seed(4)))
    ts = sat.TrainStep(model.cuda().train(), lr=1e-3, **dict(dict(grad_clip=0.1), **kw))
    assert ts.decoder_gemm_dtype == "f32"
    for k, v in attrs.items():
        setattr(ts, k, sat.no_decay_names(model) if k == "no_decay" else v)
    return ts


def batch():
    g = torch.Generator().manual_seed(6)
    B, T = len(LENGTHS), LENGTHS[0]
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(LENGTHS):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, DIM["V"], (l - 2,), generator=g)
        caps[b, l - 1] = 2
    return torch.randn(B, DIM["E"], generator=g).cuda(), caps.cuda(), list(LENGTHS)


def digests(flat, t):
    raw = t.detach().cpu().numpy()
    rows = [raw.tobytes()] + [raw[o:o + n].tobytes() for o, n, _ in (flat.slices[k] for k in sorted(flat.slices))]
    return np.stack([np.frombuffer(hashlib.sha256(r).digest(), dtype=np.uint8) for r in rows])


def run_train_step(sat, name):
    """one TrainStep case on the device -> {array name: numpy array}"""
    kw, attrs, script = TS_CASES[name]
    ts, b = engine(sat, kw, attrs), batch()
    if script == "three":
        for _ in range(3):
            ts.step(*b)
            assert "max_grad_norm" not in attrs or ts.last_grad_norm[0].item() > LOW_NORM
    elif script == "nan":
        ts.step(*b)
        ts.forward_backward(b, INV_TOKENS)
        ts.flat.grads[7] = NAN
        ts.optimizer_step()
        ts.step(*b)
    elif script == "accum":
        for _ in range(2):
            ts.forward_backward(b, INV_TOKENS)
            ts.accumulate(0.5)
        ts.optimizer_step()
    elif script == "fault":
        ts.step(*b)
        ts.check_ids()
        ts.forward_backward(b, INV_TOKENS)
        ts.fault_slot.fill_(1.0)                             # the word a faulted step would have left; nothing faults
        persist = ts.lib.sat_lstm_persist_enable(1)          # (the host's answer to a fault switches the persistent form off)
        try:
            ts.optimizer_step()
            assert ts.step_count == 2
            try:
                ts.check_ids()
                raise AssertionError("check_ids() did not raise for the set fault word")
            except RuntimeError as e:
                assert "SKIPPED on the device" in str(e)
            assert ts.step_count == 1
            ts.step(*b)
            ts.check_ids()
        finally:
            ts.lib.sat_lstm_persist_enable(persist)
    elif script == "state_dict":
        ts.step(*b)
        ts.step(*b)
        sd = ts.optimizer_state_dict()
        ts = engine(sat, kw, dict(no_decay=True))
        ts.load_optimizer_state_dict(sd)
        ts.step(*b)
    torch.cuda.synchronize()
    f = ts.flat
    out = {"params": digests(f, f.params), "m": digests(f, f.m), "v": digests(f, f.v), "steps": np.array([ts.step_count], np.int64)}
    if f.ema is not None:
        out["ema"] = digests(f, f.ema)
    if ts.last_grad_norm is not None:
        out["norm"] = ts.last_grad_norm.cpu().numpy()
    return {"%s__%s" % (name, k): v for k, v in out.items()}


# ---------------------------------------------------------------------------------------------- FusedClampAdam

def optimizer(sat, kw, decay):
    g = torch.Generator().manual_seed(8)
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.5).cuda()) for s in SHAPES]
    kw = dict(kw)
    if kw.pop("no_decay", False):
        kw["no_decay"] = [p for p in params if p.dim() <= 1]
    opt = sat.FusedClampAdam(params, lr=1e-3, **kw)
    opt.ema_decay = decay
    return opt, params


def gradients(steps=3):
    g = torch.Generator().manual_seed(9)
    return [[(torch.randn(s, generator=g) * 0.3).cuda() for s in SHAPES] for _ in range(steps)]


def run_fused_clamp_adam(sat, name):
    """one FusedClampAdam case on the device -> {array name: numpy array}"""
    kw, decay, script = FCA_CASES[name]
    opt, params = optimizer(sat, kw, decay)
    grads = gradients()
    missing = int(script[4:]) if script.startswith("none") else None

    def step(k, opt, params):
        opt.zero_grad()
        for i, (p, g) in enumerate(zip(params, grads[k])):
            if script == "stray":
                p.grad = g.clone()
            else:
                p.grad.copy_(g)
            if script == "nan" and k == 1 and i == 2:
                p.grad[1, 1] = NAN
            if i == missing and k > 0:
                p.grad = None
        opt.step()

    if script == "state_dict":
        step(0, opt, params)
        step(1, opt, params)
        sd = opt.state_dict()
        opt, params = optimizer(sat, dict(no_decay=True), 0.0)
        opt.load_state_dict(sd)
        step(2, opt, params)
    else:
        for k in range(3):
            step(k, opt, params)
    torch.cuda.synchronize()
    out = {"params": opt.flat.cpu().numpy(), "m": opt.exp_avg.cpu().numpy(), "v": opt.exp_avg_sq.cpu().numpy(),
           "steps": np.array([opt.step_count], np.int64)}
    if opt.ema is not None:
        out["ema"] = opt.ema.cpu().numpy()
    if opt.last_grad_norm is not None:
        out["norm"] = opt.last_grad_norm.cpu().numpy()
    return {"%s__%s" % (name, k): v for k, v in out.items()}


def run_all():
    sat = importlib.import_module("show-and-tell_amd")
    out = {}
    for name in TS_CASES:
        out.update(run_train_step(sat, name))
    for name in FCA_CASES:
        out.update(run_fused_clamp_adam(sat, name))
    return out


def main(out_dir=os.path.join(HERE, "optim")):
    os.makedirs(out_dir, exist_ok=True)
    out = run_all()
    np.savez_compressed(os.path.join(out_dir, NAME), **out)
    print("wrote", os.path.join(out_dir, NAME), "(%d arrays)" % len(out))


if __name__ == "__main__":
    main(*sys.argv[1:2])
