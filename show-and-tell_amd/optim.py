"""`clip_gradient(optimizer, grad_clip)` + `optim.Adam(...).step()` (`/root/reference/train.py:55-56, 88-91, 145-146`) over ONE flat
f32 buffer.  `FlatAdam` owns that buffer, its gradient / exp_avg / exp_avg_sq / averaged twins, every optimizer setting and the one
launch sequence that updates them; its docstring is the place that states the sequence and the drop rules.  Two facades sit on it:
`TrainStep` (trainer.py: the fused Show-and-Tell step) and, here, `FusedClampAdam` for the drop-in training loop (the loop that
keeps `model(...)`, `criterion`, `loss.backward()` as they are).

`FusedClampAdam(params, lr, clip=0.1)` is a `torch.optim.Optimizer`: `param_groups[0]["lr"]` is what `set_lr` (train.py:93-95)
writes, `step()` / `zero_grad()` / `state_dict()` / `load_state_dict()` keep their meaning and the state dict has
`torch.optim.Adam`'s layout.  The parameters are re-homed into the flat buffer (so build it AFTER `model.cuda()`); `step()` is torch's
single-tensor Adam arithmetic in its order, elementwise clamp first when `clip` is set (then drop the separate `clip_gradient`
call).  A torch Adam over the 12 Show-Attend-Tell parameters is ~10 multi-tensor launches + 19 clamp launches per step.

`max_norm=`, `weight_decay=`, `no_decay=` (keywords) turn the step into `torch.nn.utils.clip_grad_norm_(params, max_norm)` +
`torch.optim.AdamW(..., weight_decay=)` with `no_decay` (parameter tensors, matched by identity; `no_decay_params(module)` lists
the 1-D ones) as the group of weight decay 0.  `max_norm=float("inf")` measures without clipping; with `max_norm=None` and
`weight_decay=0` the step makes exactly the calls it makes without the keywords.  A parameter whose `.grad` is None is skipped as
torch skips it: the update runs over the segments of the buffer between such parameters, and the norm covers those alone.

`ema_decay`, `ema_warmup` (checked, settable ATTRIBUTES, not constructor keywords; 0.0 = off, otherwise a float in (0, 1)) keep an
exponential moving average of the parameters (`ema`, None until the attribute first becomes non-zero).  `with
opt.averaged_weights():` exchanges parameters and averages in place (`step()` inside raises), `ema_params()` are views of the
averages in the order of the parameters, `reset_ema()` copies the parameters again, and `state_dict()` has an `"ema"` entry
{"decay", "warmup", "params"} only once the buffer exists."""
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


def is_number(value):
    return not isinstance(value, bool) and isinstance(value, (int, float))


def check_weight_decay(value):
    if not is_number(value) or not value >= 0 or math.isinf(value):
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
    if not is_number(value) or not value > 0:
        raise ValueError("%s must be a number > 0 (got %r)" % (what, value))
    return float(value)


def check_ema_decay(value, what="ema_decay"):
    """0 (off), or a finite float in (0, 1)"""
    if not is_number(value) or not (value == 0 or 0.0 < value < 1.0):
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


def check_accumulate_weight(value, what="weight"):
    """a finite float: the factor of one folded backward"""
    if not is_number(value) or not math.isfinite(value):
        raise ValueError("%s must be a finite number (got %r)" % (what, value))
    return float(value)


def grad_accumulate(lib, acc, grads, n, weight, first):
    """one sat_grad_accumulate launch on the current stream (addresses or tensors of n + 2 floats: gradients, loss slot, fault word)"""
    L.check(lib.sat_grad_accumulate(L.ptr(acc), L.ptr(grads), n, weight, 1 if first else 0, L.stream()), "sat_grad_accumulate")


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


def packed_layout(shapes):
    """[(offset, numel, shape)] of tensors of `shapes` laid one behind the other, every offset a multiple of 4"""
    out, off = [], 0
    for shape in shapes:
        out.append((off, math.prod(shape), tuple(shape)))
        off += L.pad4(out[-1][1])
    return out


def delegated(name, to):
    """a facade's attribute that lives on its FlatAdam (the attribute `to` of the facade)"""
    return property(lambda self: getattr(getattr(self, to), name), lambda self, value: setattr(getattr(self, to), name, value))


class FlatAdam:
    """The flat Adam state behind `TrainStep` and `FusedClampAdam`, and the only place that knows the update.

    Layout: `layout` is [(offset, numel, shape)] in the order of the optimizer's parameters (the order of a state dict), offsets
    multiples of 4; `params`, `m`, `v` hold `n` floats, `grads` n + `tail` (TrainStep's loss and fault slots), `ema` is None until an
    average is first wanted.  The buffers are allocated on `device`, or handed in as `buffers` = (params, grads, m, v); on the CPU
    nothing needs the library, which is fetched by the first launch.  `tensors` (set by `rehome`) are the parameter tensors, views of
    `params`, whose version counters an update bumps.

    Settings (plain or checked attributes): lr, betas, eps; clip (None / 0 = no elementwise clamp); max_norm (None = no global norm,
    inf = measure only); weight_decay (AdamW's, 0.0 = off) and `exempt`, the merged ranges that do not decay (`set_exempt`);
    ema_decay (0.0 = off), ema_warmup.

    `update(grads, segments, skip, lr)` advances `step_count` and issues, on the current stream:
      * max_norm None and weight_decay 0: per segment ONE clamp + Adam launch -- `sat_clamp_adam_step_guarded` behind the word `skip`,
        `sat_clamp_adam_step` where there is none;
      * otherwise, with a norm, one `sat_grad_sumsq` per segment (after the clamp, when `clip` is set) into ONE array of partial pairs,
        so that the norm covers every present gradient and nothing else -- not the slots behind `n` either --, then one
        `sat_adamw_step` per segment that reads all of them, scales, decays outside `exempt` and writes `last_grad_norm`;
      * with ema_decay > 0 ONE `sat_ema_update` over the whole buffer, ema += (1 - d) (p - ema), d = `ema_decay_at(ema_decay,
        step_count, ema_warmup)`, behind the same `skip` word and, with a norm, `last_grad_norm`;
      * last, the version counters of `tensors` move, as an in-place torch update would move them: the kernels wrote through raw
        pointers, and caches keyed on `_version` (kernel-layout weight copies of a conv stack) must see the step.
    The partials workspace and `last_grad_norm` are made by the first update that needs them.

    Drop rules.  Nothing is read back.  A non-zero `skip` word drops the whole update on the device: parameters, moments and
    average stay bit for bit what they were.  With a norm, a gradient that holds an Inf or NaN does the same by itself;
    `last_grad_norm` is a 2-element f64 DEVICE tensor {norm, number of Inf / NaN gradient elements}, so `last_grad_norm[1] > 0`, read
    whenever the loop likes, tells.  `step_count` advances all the same (the bias correction of later steps sees one step more)
    unless the owner rolls it back.  A parameter outside every segment does not move, and an average that equals it does not either.

    Averaging.  `averaged_weights(owner)` exchanges `params` and `ema` in place (`sat_swap_f32`, no third buffer) and bumps the version
    counters, on the way in and out; in between `averaged` is set, `update`, `reset_ema` and loading an "ema" entry refuse, and
    `averages()` -- the buffer that holds the averaged weights right now -- is `params`."""

    WORDS = ("max_norm", "this optimizer %d", "load_state_dict()")      # how the owner's messages name what the core checks

    def __init__(self, layout, device=None, tail=0, buffers=None):
        self.layout = [(o, n, tuple(shape)) for o, n, shape in layout]
        self.n = max(o + L.pad4(n) for o, n, _ in self.layout)
        if buffers is None:
            buffers = [torch.zeros(self.n + (tail if k == 1 else 0), device=device) for k in range(4)]
        self.params, self.grads, self.m, self.v = buffers
        self.ema = self.lib = self.last_grad_norm = self._partials = None
        self.tensors, self.exempt, self.step_count, self.averaged = [], [], 0, False
        self.lr, self.betas, self.eps, self.clip = 1e-3, (0.9, 0.999), 1e-8, None
        self._max_norm, self._weight_decay, self._ema_decay, self._ema_warmup = None, 0.0, 0.0, False

    def rehome(self, tensors):
        """copy the parameter `tensors` (in `layout` order) into `params`, make them views of it and their `.grad` views of `grads`;
        returns the gradient views"""
        self.tensors = list(tensors)
        for p, (o, n, shape) in zip(self.tensors, self.layout):
            self.params[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.params[o:o + n].view(shape)
            p.grad = self.grads[o:o + n].view(shape)
        return self.views(self.grads)

    def views(self, buf):
        """the slices of `buf` in the order and shapes of the parameters"""
        return [buf[o:o + n].view(shape) for o, n, shape in self.layout]

    # -- settings ---------------------------------------------------------------------------------------------------------------
    @property
    def max_norm(self):
        return self._max_norm

    @max_norm.setter
    def max_norm(self, value):
        self._max_norm = None if value is None else check_max_norm(value, self.WORDS[0])

    @property
    def weight_decay(self):
        return self._weight_decay

    @weight_decay.setter
    def weight_decay(self, value):
        self._weight_decay = check_weight_decay(value)

    def set_exempt(self, slices):
        """`slices` ((offset, numel, ...) entries of the layout) do not decay"""
        self.exempt = merge_ranges([(s[0], s[0] + s[1]) for s in slices])

    @property
    def ema_decay(self):
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value):
        self._ema_decay = check_ema_decay(value)
        if self._ema_decay > 0 and self.ema is None:
            self.ema = self.params.clone()

    @property
    def ema_warmup(self):
        return self._ema_warmup

    @ema_warmup.setter
    def ema_warmup(self, value):
        self._ema_warmup = check_ema_warmup(value)

    # -- the update -------------------------------------------------------------------------------------------------------------
    def update(self, grads, segments=None, skip=None, lr=None):
        """grads: the buffer to read (`grads`, or TrainStep's accumulated twin); segments: [(a, b)] element ranges to cover, None =
        the whole buffer; skip: 1-element device tensor, the word that drops the update, or None; lr: instead of `lr`, once"""
        if self.averaged:
            raise RuntimeError(AVERAGED_NOTE % "an update")
        lib, st = self.lib or L.load(), L.stream()
        self.step_count += 1
        segments = [(0, self.n)] if segments is None else segments
        p, g, m, v, word = self.params.data_ptr(), grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), L.ptr(skip)
        hyper = (float(self.lr if lr is None else lr), self.betas[0], self.betas[1], float(self.eps),
                 float(self.clip) if self.clip else 0.0, self.step_count)
        norm, wd = self._max_norm is not None, self._weight_decay
        if not norm and wd == 0:
            for a, b in segments:
                if skip is None:
                    L.check(lib.sat_clamp_adam_step(p + a * 4, g + a * 4, m + a * 4, v + a * 4, b - a, *hyper, st), "sat_clamp_adam_step")
                else:
                    L.check(lib.sat_clamp_adam_step_guarded(p + a * 4, g + a * 4, m + a * 4, v + a * 4, b - a, *hyper, word, st),
                            "sat_clamp_adam_step_guarded")
        elif segments:
            partials, total, norm_out = None, 0, None
            if norm:
                counts = [lib.sat_grad_sumsq_partials(b - a) for a, b in segments]
                total = sum(counts)
                if self._partials is None or self._partials.numel() < 2 * total:
                    self._partials = torch.empty(2 * total, dtype=torch.float64, device=self.params.device)
                if self.last_grad_norm is None:
                    self.last_grad_norm = torch.zeros(2, dtype=torch.float64, device=self.params.device)
                partials, norm_out, off = self._partials.data_ptr(), self.last_grad_norm.data_ptr(), 0
                for (a, b), c in zip(segments, counts):
                    L.check(lib.sat_grad_sumsq(g + a * 4, b - a, hyper[4], partials, off, total, st), "sat_grad_sumsq")
                    off += c
            for a, b in segments:
                ex, nex = exempt_array(self.exempt, a, b) if wd > 0 else (None, 0)
                L.check(lib.sat_adamw_step(p + a * 4, g + a * 4, m + a * 4, v + a * 4, b - a, *hyper, wd, ex, nex, self._max_norm or 0.0,
                                           partials, total, norm_out, word, st), "sat_adamw_step")
        if self._ema_decay > 0:
            L.check(lib.sat_ema_update(self.ema.data_ptr(), p, self.n, ema_decay_at(self._ema_decay, self.step_count, self._ema_warmup),
                                       word, L.ptr(self.last_grad_norm) if norm else None, st), "sat_ema_update")
        torch.autograd.graph.increment_version(self.tensors)

    # -- averaged weights -------------------------------------------------------------------------------------------------------
    def averages(self, what):
        """the buffer that holds the averaged weights right now (inside `averaged_weights()` the two have changed places)"""
        if self.ema is None:
            raise RuntimeError("%s: no average is kept (ema_decay has never been set)" % what)
        return self.params if self.averaged else self.ema

    def reset_ema(self):
        """the average starts again from the parameters as they are now"""
        self.averages("reset_ema()")
        if self.averaged:
            raise RuntimeError(AVERAGED_NOTE % "reset_ema()")
        self.ema.copy_(self.params)

    @contextlib.contextmanager
    def averaged_weights(self, owner):
        """`with owner.averaged_weights():` -- yields `owner`; the blocks do not nest"""
        self.averages("averaged_weights()")
        if self.averaged:
            raise RuntimeError("averaged_weights() is already active: the blocks do not nest")

        def swap():
            L.check((self.lib or L.load()).sat_swap_f32(L.ptr(self.params), L.ptr(self.ema), self.n, L.stream()), "sat_swap_f32")
            torch.autograd.graph.increment_version(self.tensors)       # caches keyed on `_version` see the exchange

        swap()
        self.averaged = True
        try:
            yield owner
        finally:
            self.averaged = False
            swap()

    # -- state dicts in torch.optim.Adam's layout ---------------------------------------------------------------------------------
    def state_dict(self, names=None):
        """loads into a torch Adam / AdamW over the same parameters and back; `names`: a "param_names" entry"""
        state = {}
        if self.step_count > 0:
            for i, (m, v) in enumerate(zip(self.views(self.m), self.views(self.v))):
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        wd = self._weight_decay
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": wd if wd > 0 else 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": wd > 0, "params": list(range(len(self.layout)))}
        sd = {"state": state, "param_groups": [group]}
        if names is not None:
            sd["param_names"] = list(names)
        sd["grad_clip"], sd["max_grad_norm"] = self.clip, self._max_norm
        if self.ema is not None:             # the averaged weights, one tensor per parameter
            sd["ema"] = {"decay": self._ema_decay, "warmup": self._ema_warmup,
                         "params": [t.clone() for t in self.views(self.averages("state_dict()"))]}
        return sd

    def load_state_dict(self, sd, names=None):
        """every check is a ValueError; "max_grad_norm" off is None or 0, an absent key or "ema" entry leaves what is set"""
        group = sd["param_groups"][0]
        if len(group["params"]) != len(self.layout):
            raise ValueError(("optimizer state has %d parameters, " + self.WORDS[1]) % (len(group["params"]), len(self.layout)))
        self.lr, self.betas, self.eps = float(group["lr"]), tuple(group["betas"]), float(group["eps"])
        self.weight_decay = group_weight_decay(group)
        if "max_grad_norm" in sd:
            value = sd["max_grad_norm"]
            self.max_norm = None if (is_number(value) and value == 0) else value
        if "ema" in sd:
            if self.averaged:
                raise RuntimeError(AVERAGED_NOTE % (self.WORDS[2] + " with averaged weights"))
            tensors = list(sd["ema"]["params"])
            if len(tensors) != len(self.layout):
                raise ValueError("the averaged weights hold %d parameters, expected %d" % (len(tensors), len(self.layout)))
            for i, (t, (_, _, shape)) in enumerate(zip(tensors, self.layout)):
                if tuple(t.shape) != shape:
                    raise ValueError("averaged parameter %d has shape %s, expected %s" % (i, tuple(t.shape), shape))
            decay, warmup = check_ema_decay(sd["ema"]["decay"]), check_ema_warmup(sd["ema"]["warmup"])
            if self.ema is None:
                self.ema = torch.zeros_like(self.params)
            for t, view in zip(tensors, self.views(self.ema)):
                view.copy_(t)
            self._ema_decay, self._ema_warmup = decay, warmup
        self.m.zero_()
        self.v.zero_()
        steps = set()
        for i, (m, v) in enumerate(zip(self.views(self.m), self.views(self.v))):
            st = sd["state"].get(group["params"][i])
            if st is None:
                continue
            if tuple(st["exp_avg"].shape) != tuple(m.shape):
                raise ValueError("optimizer state %s has shape %s, expected %s"
                                 % ("of %s" % names[i] if names else "%d" % i, tuple(st["exp_avg"].shape), tuple(m.shape)))
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter Adam step counts differ (%s): one flat step count is kept" % sorted(steps))
        self.step_count = steps.pop() if steps else 0


class FusedClampAdam(torch.optim.Optimizer):
    """the `torch.optim.Optimizer` facade of a `FlatAdam` (`core`): `param_groups[0]` is the home of lr / betas / eps"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, clip=None, *, max_norm=None, weight_decay=0.0, no_decay=()):
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("no trainable parameters")
        if any(p.dtype != torch.float32 for p in params):
            raise TypeError("FusedClampAdam holds f32 parameters")
        layout = packed_layout([p.shape for p in params])
        max_norm = None if max_norm is None else check_max_norm(max_norm)
        weight_decay = check_weight_decay(weight_decay)
        ids = {id(p): i for i, p in enumerate(params)}
        if any(id(t) not in ids for t in no_decay):
            raise ValueError("a no_decay entry is not one of the optimizer's parameters")
        exempt = merge_ranges([(layout[i][0], layout[i][0] + layout[i][1]) for i in {ids[id(t)] for t in no_decay}])
        L.require_gpu(params[0], "parameters")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))
        self.core = c = FlatAdam(layout, params[0].device)
        c.lib, c.clip, c.max_norm, c.weight_decay, c.exempt = L.load(), clip, max_norm, weight_decay, exempt
        self._views = c.rehome(params)

    lib, clip, max_norm, weight_decay = (delegated(k, "core") for k in ("lib", "clip", "max_norm", "weight_decay"))
    flat, flat_grad, exp_avg, exp_avg_sq = (delegated(k, "core") for k in ("params", "grads", "m", "v"))
    ema, n, step_count, last_grad_norm = (delegated(k, "core") for k in ("ema", "n", "step_count", "last_grad_norm"))
    ema_decay, ema_warmup, _exempt, _averaged = (delegated(k, "core") for k in ("ema_decay", "ema_warmup", "exempt", "averaged"))
    _slices = property(lambda self: [s[:2] for s in self.core.layout])

    def reset_ema(self):
        """the average starts again from the parameters as they are now"""
        self.core.reset_ema()

    def ema_params(self):
        """views of the averaged weights, in the order (and shapes) of the optimizer's parameters"""
        return self.core.views(self.core.averages("ema_params()"))

    def averaged_weights(self):
        """`with opt.averaged_weights():` -- the parameters hold the averaged weights inside the block (exchanged in place, version
        counters bumped) and their own values again after it; `step()` inside and a nested entry raise RuntimeError"""
        return self.core.averaged_weights(self)

    def zero_grad(self, set_to_none=False):
        """One memset; the `.grad` of every parameter stays the view into the flat gradient buffer, so the backward
        accumulates in place.  (`model.zero_grad()` -- train.py:137 -- drops the views; `step()` then copies the gradients in.)"""
        c = self.core
        c.grads.zero_()
        for p, v in zip(c.tensors, self._views):
            p.grad = v

    @torch.no_grad()
    def step(self, closure=None):
        c = self.core
        if c.averaged:
            raise RuntimeError(AVERAGED_NOTE % "step()")
        loss = closure() if closure is not None else None
        src, dst, segs, start = [], [], [], 0
        # torch skips a parameter whose grad is None: run the segments between such parameters
        for p, v, (o, n, _) in zip(c.tensors, self._views, c.layout):
            if p.grad is None:
                if o > start:
                    segs.append((start, o))
                start = o + L.pad4(n)
            elif p.grad.data_ptr() != v.data_ptr():
                src.append(p.grad)
                dst.append(v)
        if start < c.n:
            segs.append((start, c.n))
        if src:
            torch._foreach_copy_(dst, src)
        g = self.param_groups[0]
        c.lr, c.betas, c.eps = g["lr"], g["betas"], g["eps"]
        c.update(c.grads, segs)
        return loss

    def state_dict(self):
        c, g = self.core, self.param_groups[0]
        c.lr, c.betas, c.eps = g["lr"], g["betas"], g["eps"]
        return c.state_dict()

    def load_state_dict(self, sd):
        c, g = self.core, self.param_groups[0]
        c.load_state_dict(sd)
        g["lr"], g["betas"], g["eps"] = c.lr, c.betas, c.eps
