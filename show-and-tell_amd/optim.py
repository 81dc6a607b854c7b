"""`clip_gradient(optimizer, grad_clip)` + `optim.Adam(...).step()` (`/root/reference/train.py:55-56, 88-91, 145-146`) as ONE
launch for the drop-in training loop (the loop that keeps `model(...)`, `criterion`, `loss.backward()` as they are).

`FusedClampAdam(params, lr, clip=0.1)` is a `torch.optim.Optimizer`: `param_groups[0]["lr"]` is what `set_lr` (train.py:93-95)
writes, `step()` / `zero_grad()` / `state_dict()` / `load_state_dict()` keep their meaning and the state dict has
`torch.optim.Adam`'s layout.  The parameters are re-homed into one flat f32 buffer (so build it AFTER `model.cuda()`), with
flat gradient / exp_avg / exp_avg_sq twins; `step()` is `sat_clamp_adam_step` over the whole buffer -- torch's single-tensor
Adam arithmetic in its order, elementwise clamp first when `clip` is set (then drop the separate `clip_gradient` call).
A torch Adam over the 12 Show-Attend-Tell parameters is ~10 multi-tensor launches + 19 clamp launches per step.

`max_norm=`, `weight_decay=`, `no_decay=` (keywords) turn the step into `torch.nn.utils.clip_grad_norm_(params, max_norm)` +
`torch.optim.AdamW(..., weight_decay=)` with `no_decay` (parameter tensors, matched by identity; `no_decay_params(module)` lists
the 1-D ones) as the group of weight decay 0: one `sat_grad_sumsq` launch over the flat gradient (after the clamp, when `clip`
is set too), then one `sat_adamw_step`.  Nothing is read back: `last_grad_norm` is a 2-element f64 DEVICE tensor {norm, number of
Inf / NaN gradient elements} (None until a step with `max_norm` has run; `max_norm=float("inf")` measures without clipping).
A step whose gradient holds an Inf or NaN is DROPPED on the device -- parameters, moments and gradient stay bit for bit what they
were -- while `step_count` still advances (the bias correction of later steps sees one step more); `last_grad_norm[1] > 0` tells.
With `max_norm=None` and `weight_decay=0` the step makes exactly the calls it makes without the keywords.

`ema_decay`, `ema_warmup` (checked, settable ATTRIBUTES, not constructor keywords; 0.0 = off, otherwise a float in (0, 1)) keep an
exponential moving average of the parameters in a twin of the flat buffer (`ema`, None until the attribute first becomes non-zero,
then a copy of the parameters): ONE `sat_ema_update` launch over the whole buffer behind the update(s) of a `step()`,
ema += (1 - d) (p - ema) with d = `ema_decay_at(ema_decay, step_count, ema_warmup)`.  A parameter whose gradient is None does not
move, and an average that equals it does not either; with `max_norm` the launch reads `last_grad_norm`, so a step dropped for a
non-finite gradient leaves the average alone.  `with opt.averaged_weights():` exchanges parameters and averages in place
(`sat_swap_f32`; `step()` inside raises), `ema_params()` are views of the averages in the order of the parameters, `reset_ema()`
copies the parameters again, and `state_dict()` has an `"ema"` entry {"decay", "warmup", "params"} only once the buffer exists."""
import contextlib
import ctypes
import math

import torch

from . import _lib as L

MAX_EXEMPT = 32         # sat_adamw_step's table of ranges that do not decay


def no_decay_params(module):
    """The parameters of `module` that AdamW recipes leave out of the weight decay: the 1-D ones (biases, BatchNorm weight / bias)."""
    return [p for p in module.parameters() if p.requires_grad and p.dim() <= 1]


def no_decay_names(module):
    """`no_decay_params` by name (`TrainStep.no_decay` takes names)."""
    return [n for n, p in module.named_parameters() if p.requires_grad and p.dim() <= 1]


def check_weight_decay(value):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not value >= 0 or math.isinf(value):
        raise ValueError("weight_decay must be a finite number >= 0 (got %r)" % (value,))
    return float(value)


def group_weight_decay(group):
    """the weight decay of a loaded param group; torch.optim.Adam's COUPLED (L2) decay is not what the kernel computes"""
    wd = check_weight_decay(group.get("weight_decay", 0))
    if wd > 0 and group.get("decoupled_weight_decay", True) is False:
        raise ValueError("the optimizer state has a coupled (L2) weight_decay; only AdamW's decoupled decay is implemented")
    return wd


def check_max_norm(value, what="max_norm"):
    """a number > 0; float("inf") measures the norm without clipping"""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not value > 0:
        raise ValueError("%s must be a number > 0 (got %r)" % (what, value))
    return float(value)


def check_ema_decay(value, what="ema_decay"):
    """0 (off), or a finite float in (0, 1)"""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (value == 0 or 0.0 < value < 1.0):
        raise ValueError("%s must be 0 (off) or a number in (0, 1) (got %r)" % (what, value))
    return float(value)


def check_ema_warmup(value):
    if not isinstance(value, bool):
        raise ValueError("ema_warmup must be a bool (got %r)" % (value,))
    return value


def ema_decay_at(decay, t, warmup=False):
    """The decay of the update that follows optimizer step `t` (1-based: `step_count` after its increment).  With warm-up
    min(decay, (1 + t) / (10 + t)) -- TensorFlow's `num_updates` rule for ExponentialMovingAverage, which timm's ModelEma uses too: the
    first averages follow the parameters closely instead of remembering the initial ones for 1 / (1 - decay) steps."""
    return min(decay, (1 + t) / (10 + t)) if warmup else decay


def ema_update(lib, ema, params, n, decay, skip=None, norm_state=None):
    """one sat_ema_update launch on the current stream (addresses or tensors; `skip`, `norm_state`: the words of the update in front)"""
    L.check(lib.sat_ema_update(L.ptr(ema), L.ptr(params), n, decay, L.ptr(skip), L.ptr(norm_state), L.stream()), "sat_ema_update")


def check_accumulate_weight(value, what="weight"):
    """a finite float: the factor of one folded backward"""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
        raise ValueError("%s must be a finite number (got %r)" % (what, value))
    return float(value)


def grad_accumulate(lib, acc, grads, n, weight, first):
    """one sat_grad_accumulate launch on the current stream (addresses or tensors of n + 2 floats: gradients, loss slot, fault word)"""
    L.check(lib.sat_grad_accumulate(L.ptr(acc), L.ptr(grads), n, weight, 1 if first else 0, L.stream()), "sat_grad_accumulate")


def ema_entry(decay, warmup, tensors):
    """the "ema" entry of an optimizer state dict"""
    return {"decay": decay, "warmup": warmup, "params": tensors}


def check_ema_entry(entry, shapes):
    """(decay, warmup, tensors) of a loaded "ema" entry, checked like the moments (ValueError)"""
    tensors = list(entry["params"])
    if len(tensors) != len(shapes):
        raise ValueError("the averaged weights hold %d parameters, expected %d" % (len(tensors), len(shapes)))
    for i, (t, shape) in enumerate(zip(tensors, shapes)):
        if tuple(t.shape) != tuple(shape):
            raise ValueError("averaged parameter %d has shape %s, expected %s" % (i, tuple(t.shape), tuple(shape)))
    return check_ema_decay(entry["decay"]), check_ema_warmup(entry["warmup"]), tensors


@contextlib.contextmanager
def swapped_in(owner, live, ema, n, params):
    """`averaged_weights()` of both optimizers: `live` <-> `ema` in place (sat_swap_f32) with the version counters of `params` (views
    of `live`) bumped, and back on the way out.  `owner._averaged` is set in between: its update entry points refuse then."""
    if ema is None:
        raise RuntimeError("averaged_weights(): no average is kept (ema_decay has never been set)")
    if owner._averaged:
        raise RuntimeError("averaged_weights() is already active: the blocks do not nest")

    def swap():
        L.check(owner.lib.sat_swap_f32(L.ptr(live), L.ptr(ema), n, L.stream()), "sat_swap_f32")
        torch.autograd.graph.increment_version(params)       # caches keyed on `_version` see the exchange

    swap()
    owner._averaged = True
    try:
        yield owner
    finally:
        owner._averaged = False
        swap()


AVERAGED_NOTE = "inside averaged_weights() the parameters are the averaged ones: %s is refused until the block is left"


def merge_ranges(ranges):
    """[(lo, hi)] element ranges of flat slices (every lo a multiple of 4) sorted, with neighbours whose padded end meets the next
    start merged; ValueError for more than sat_adamw_step's 32"""
    out = []
    for lo, hi in sorted(ranges):
        if out and L.pad4(out[-1][1]) >= lo:
            out[-1] = (out[-1][0], max(hi, out[-1][1]))
        else:
            out.append((lo, hi))
    if len(out) > MAX_EXEMPT:
        raise ValueError("no_decay makes %d separate ranges of the flat buffer, the kernel takes %d" % (len(out), MAX_EXEMPT))
    return out


def exempt_array(ranges, a=0, b=None):
    """(ctypes int64 array or None, count): `ranges` cut to the segment [a, b) of the flat buffer, relative to a"""
    cut = [(max(lo, a) - a, (hi if b is None else min(hi, b)) - a) for lo, hi in ranges if hi > a and (b is None or lo < b)]
    if not cut:
        return None, 0
    return (ctypes.c_int64 * (2 * len(cut)))(*[x for r in cut for x in r]), len(cut)


class FusedClampAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, clip=None, *, max_norm=None, weight_decay=0.0, no_decay=()):
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("no trainable parameters")
        if any(p.dtype != torch.float32 for p in params):
            raise TypeError("FusedClampAdam holds f32 parameters")
        self.max_norm = None if max_norm is None else check_max_norm(max_norm)
        self.weight_decay = check_weight_decay(weight_decay)
        ids = {id(p): i for i, p in enumerate(params)}
        exempt = []
        for t in no_decay:
            if id(t) not in ids:
                raise ValueError("a no_decay entry is not one of the optimizer's parameters")
            exempt.append(ids[id(t)])
        self._slices, off = [], 0
        for p in params:
            self._slices.append((off, p.numel()))
            off += L.pad4(p.numel())
        self._exempt = merge_ranges([(self._slices[i][0], sum(self._slices[i])) for i in set(exempt)])
        L.require_gpu(params[0], "parameters")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))
        self.clip = clip
        self.lib = L.load()
        dev = params[0].device
        self.n = off
        self.flat = torch.zeros(off, device=dev)
        self.flat_grad = torch.zeros(off, device=dev)
        self.exp_avg = torch.zeros(off, device=dev)
        self.exp_avg_sq = torch.zeros(off, device=dev)
        self.step_count = 0
        self.last_grad_norm = None
        self._partials = None
        self._params = params
        self._views = []
        for p, (o, n) in zip(params, self._slices):
            self.flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + n].view(p.shape)
            self._views.append(self.flat_grad[o:o + n].view(p.shape))
            p.grad = self._views[-1]

    # -- averaged weights: ema_decay / ema_warmup are checked, settable attributes (0.0 = off; see the module docstring) ------------
    _ema_decay, _ema_warmup, _averaged, ema = 0.0, False, False, None

    @property
    def ema_decay(self):
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value):
        self._ema_decay = check_ema_decay(value)
        # (an optimizer made without __init__ has no flat buffer: the first step() copies)
        if self._ema_decay > 0 and self.ema is None and getattr(self, "flat", None) is not None:
            self.ema = self.flat.clone()

    @property
    def ema_warmup(self):
        return self._ema_warmup

    @ema_warmup.setter
    def ema_warmup(self, value):
        self._ema_warmup = check_ema_warmup(value)

    def reset_ema(self):
        """the average starts again from the parameters as they are now"""
        if self.ema is None:
            raise RuntimeError("reset_ema(): no average is kept (ema_decay has never been set)")
        if self._averaged:
            raise RuntimeError(AVERAGED_NOTE % "reset_ema()")
        self.ema.copy_(self.flat)

    def ema_params(self):
        """views of the averaged weights, in the order (and shapes) of the optimizer's parameters"""
        if self.ema is None:
            raise RuntimeError("ema_params(): no average is kept (ema_decay has never been set)")
        src = self.flat if self._averaged else self.ema        # (inside averaged_weights() the two buffers have changed places)
        return [src[o:o + n].view(p.shape) for p, (o, n) in zip(self._params, self._slices)]

    def averaged_weights(self):
        """`with opt.averaged_weights():` -- the parameters hold the averaged weights inside the block (exchanged in place, version
        counters bumped) and their own values again after it; `step()` inside and a nested entry raise RuntimeError"""
        return swapped_in(self, self.flat, self.ema, self.n, self._params)

    def zero_grad(self, set_to_none=False):
        """One memset; the `.grad` of every parameter stays the view into the flat gradient buffer, so the backward
        accumulates in place.  (`model.zero_grad()` -- train.py:137 -- drops the views; `step()` then copies the gradients in.)"""
        self.flat_grad.zero_()
        for p, v in zip(self._params, self._views):
            p.grad = v

    @torch.no_grad()
    def step(self, closure=None):
        if self._averaged:
            raise RuntimeError(AVERAGED_NOTE % "step()")
        if self._ema_decay > 0 and self.ema is None:
            self.ema = self.flat.clone()                      # (the attribute was set before the buffers existed)
        loss = closure() if closure is not None else None
        src, dst, missing = [], [], []
        for i, (p, v) in enumerate(zip(self._params, self._views)):
            if p.grad is None:
                missing.append(i)
            elif p.grad.data_ptr() != v.data_ptr():
                src.append(p.grad)
                dst.append(v)
        if src:
            torch._foreach_copy_(dst, src)
        g = self.param_groups[0]
        self.step_count += 1
        clip = float(self.clip) if self.clip else 0.0
        # torch skips a parameter whose grad is None: run the segments between such parameters
        segs, start = [], 0
        for i in missing:
            o, n = self._slices[i]
            if o > start:
                segs.append((start, o))
            start = o + L.pad4(n)
        if start < self.n:
            segs.append((start, self.n))
        if self.max_norm is None and self.weight_decay == 0:
            for a, b in segs:
                L.check(self.lib.sat_clamp_adam_step(self.flat.data_ptr() + a * 4, self.flat_grad.data_ptr() + a * 4,
                                                     self.exp_avg.data_ptr() + a * 4, self.exp_avg_sq.data_ptr() + a * 4, b - a,
                                                     float(g["lr"]), g["betas"][0], g["betas"][1], float(g["eps"]), clip,
                                                     self.step_count, L.stream()), "sat_clamp_adam_step")
        elif segs:
            self._adamw_segments(segs, g, clip)
        if self._ema_decay > 0:
            # ONE launch over the whole buffer behind the update(s): a parameter without a gradient did not move, and an average
            # that equals it does not either; a step dropped for a non-finite gradient (max_norm) leaves the average alone too
            ema_update(self.lib, self.ema, self.flat, self.n, ema_decay_at(self._ema_decay, self.step_count, self._ema_warmup),
                       norm_state=self.last_grad_norm if self.max_norm is not None else None)
        # the kernel wrote the parameters through raw pointers: move their version counters as an in-place torch update
        # would, so that caches keyed on `_version` (kernel-layout weight copies of a conv stack) see the step
        torch.autograd.graph.increment_version(self._params)
        return loss

    def _adamw_segments(self, segs, g, clip):
        """the step with a global norm and / or weight decay: every present segment's sum of squares into ONE array of partial pairs
        (so the norm covers every present gradient and nothing else), then one sat_adamw_step per segment reading all of them"""
        lib, st = self.lib, L.stream()
        partials, total, norm_out = None, 0, None
        if self.max_norm is not None:
            counts = [lib.sat_grad_sumsq_partials(b - a) for a, b in segs]
            total = sum(counts)
            if self._partials is None or self._partials.numel() < 2 * total:
                self._partials = torch.empty(2 * total, dtype=torch.float64, device=self.flat.device)
            if self.last_grad_norm is None:
                self.last_grad_norm = torch.zeros(2, dtype=torch.float64, device=self.flat.device)
            partials, norm_out, off = self._partials.data_ptr(), self.last_grad_norm.data_ptr(), 0
            for (a, b), c in zip(segs, counts):
                L.check(lib.sat_grad_sumsq(self.flat_grad.data_ptr() + a * 4, b - a, clip, partials, off, total, st), "sat_grad_sumsq")
                off += c
        for a, b in segs:
            ex, nex = exempt_array(self._exempt, a, b) if self.weight_decay > 0 else (None, 0)
            L.check(lib.sat_adamw_step(self.flat.data_ptr() + a * 4, self.flat_grad.data_ptr() + a * 4,
                                       self.exp_avg.data_ptr() + a * 4, self.exp_avg_sq.data_ptr() + a * 4, b - a,
                                       float(g["lr"]), g["betas"][0], g["betas"][1], float(g["eps"]), clip, self.step_count,
                                       self.weight_decay, ex, nex, self.max_norm or 0.0, partials, total, norm_out, None, st),
                    "sat_adamw_step")

    def state_dict(self):
        state = {}
        if self.step_count > 0:
            for i, (p, (o, n)) in enumerate(zip(self._params, self._slices)):
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": self.exp_avg[o:o + n].view(p.shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).clone()}
        g = self.param_groups[0]
        wd = self.weight_decay
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": wd if wd > 0 else 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": wd > 0, "params": list(range(len(self._params)))}
        sd = {"state": state, "param_groups": [group], "grad_clip": self.clip, "max_grad_norm": self.max_norm}
        if self.ema is not None:
            sd["ema"] = ema_entry(self._ema_decay, self._ema_warmup, [t.clone() for t in self.ema_params()])
        return sd

    def load_state_dict(self, sd):
        group = sd["param_groups"][0]
        if len(group["params"]) != len(self._params):
            raise ValueError("optimizer state has %d parameters, this optimizer %d" % (len(group["params"]), len(self._params)))
        g = self.param_groups[0]
        g["lr"], g["betas"], g["eps"] = float(group["lr"]), tuple(group["betas"]), float(group["eps"])
        self.weight_decay = group_weight_decay(group)
        if "max_grad_norm" in sd:
            off = sd["max_grad_norm"] is None or sd["max_grad_norm"] == 0          # (0.0: TrainStep's "off")
            self.max_norm = None if off else check_max_norm(sd["max_grad_norm"])
        if "ema" in sd:                                       # (absent: the averaging state stays what it is)
            if self._averaged:
                raise RuntimeError(AVERAGED_NOTE % "load_state_dict() with averaged weights")
            decay, warmup, tensors = check_ema_entry(sd["ema"], [p.shape for p in self._params])
            if self.ema is None:
                self.ema = torch.zeros_like(self.flat)
            for t, (o, n) in zip(tensors, self._slices):
                self.ema[o:o + n].copy_(t.reshape(-1))
            self._ema_decay, self._ema_warmup = decay, warmup
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        steps = set()
        for i, (p, (o, n)) in enumerate(zip(self._params, self._slices)):
            st = sd["state"].get(group["params"][i])
            if st is None:
                continue
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError("optimizer state %d has shape %s, expected %s" % (i, tuple(st["exp_avg"].shape), tuple(p.shape)))
            self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter Adam step counts differ (%s): one flat step count is kept" % sorted(steps))
        self.step_count = steps.pop() if steps else 0
