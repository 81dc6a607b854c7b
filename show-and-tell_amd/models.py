"""Drop-in `models` module: `EncoderCNN` / `DecoderRNN` with the reference's constructor and forward()/sample()
signatures (`/root/reference/models.py:9-67`), every tensor op behind them a libsat_hip.so kernel.

    EncoderCNN(embed_size).forward(images f32[B,3,H,W]) -> f32[B,embed_size]              (models.py:10,25)
    DecoderRNN(embed_size, hidden_size, vocab_size, num_layers)
        .forward(features, captions i64[B,T'], lengths list[int] desc) -> f32[sum(lengths), V]   (models.py:47-54)
        .sample(features, states=None) -> i64[B,20]                                        (models.py:56-67)
    ShowAndTell(...)(images, captions, lengths) / .sample(images, state): the single-module contract the
        reference trainer uses (train.py:139, eval.py:93,99).

`state_dict()` key names equal the reference's (`resnet.*`, `bn.*`, `embed.weight`, `lstm.weight_ih_l{k}`, ...,
`linear.weight`, `linear.bias`).  Parameters are ordinary nn.Parameters with `.grad`, so the reference's
`clip_gradient` + `optim.Adam` loop works unchanged; `trainer.TrainStep` is the fused HIP replacement.
The modules run on the GPU only: there is no CPU fallback.
"""
import os

import torch
import torch.nn as nn

from . import _lib as L
from .pack import PackInfo
from .decoder import decoder_backward, decoder_forward, rollout_forward
from .resnet import RESNET152, ConvStackProgram, ResNetStack, weights_signature
from .watch import IdGuard  # noqa: F401  (also imported from here by callers)

BN1D_MOMENTUM = 0.01   # models.py:17
BN_EPS = 1e-5


def _f32c(t, name):
    L.require_gpu(t, name)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32" % name)
    return t.contiguous()


# ------------------------------------------------------------------------------------------------------
# encoder
def fc_bn1d_forward(lib, pooled, w_fc, b_fc, gamma, beta, running_mean, running_var, training, feats, xhat, rstd, ws):
    """resnet.fc + BatchNorm1d (models.py:16-17,27-28), sat_fc_bn1d_fwd, into the caller's buffers: feats, xhat f32 [B, E], rstd
    [E], ws f32 of at least sat_fc_bn1d_ws_bytes"""
    B, F = pooled.shape
    L.check(lib.sat_fc_bn1d_fwd(L.ptr(pooled), L.ptr(w_fc), L.ptr(b_fc), L.ptr(gamma), L.ptr(beta), L.ptr(running_mean),
                                L.ptr(running_var), BN1D_MOMENTUM, BN_EPS, 1 if training else 0, B, F, w_fc.shape[0], L.ptr(feats),
                                L.ptr(xhat), L.ptr(rstd), L.ptr(ws), ws.numel() * 4, L.stream()), "sat_fc_bn1d_fwd")


def fc_bn1d_backward(lib, dy, pooled, xhat, rstd, gamma, dw, db, dg, dbe, ws):
    """its backward (sat_fc_bn1d_bwd, batch statistics) into the caller's gradient buffers; ws f32 of at least B * E"""
    B, F = pooled.shape
    L.check(lib.sat_fc_bn1d_bwd(L.ptr(dy), L.ptr(pooled), L.ptr(xhat), L.ptr(rstd), L.ptr(gamma), B, F, gamma.shape[0], L.ptr(dw),
                                L.ptr(db), L.ptr(dg), L.ptr(dbe), L.ptr(ws), ws.numel() * 4, L.stream()), "sat_fc_bn1d_bwd")


class _HeadFn(torch.autograd.Function):
    """resnet.fc + BatchNorm1d (models.py:16-17,27-28) -- sat_fc_bn1d_fwd / sat_fc_bn1d_bwd."""

    @staticmethod
    def forward(ctx, pooled, w_fc, b_fc, gamma, beta, running_mean, running_var, training):
        lib = L.load()
        B, F = pooled.shape
        E = w_fc.shape[0]
        dev = pooled.device
        feats, xhat, rstd = torch.empty(B, E, device=dev), torch.empty(B, E, device=dev), torch.empty(E, device=dev)
        ws = torch.empty(lib.sat_fc_bn1d_ws_bytes(B, F, E) // 4, device=dev)
        fc_bn1d_forward(lib, pooled, w_fc, b_fc, gamma, beta, running_mean, running_var, training, feats, xhat, rstd, ws)
        ctx.save_for_backward(pooled, xhat, rstd, gamma)
        ctx.training = training
        return feats

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise RuntimeError("EncoderCNN backward is only defined in training mode (batch statistics)")
        pooled, xhat, rstd, gamma = ctx.saved_tensors
        B, F = pooled.shape
        E = gamma.shape[0]
        dev = pooled.device
        dw, db, dg, dbe = torch.empty(E, F, device=dev), torch.empty(E, device=dev), torch.empty(E, device=dev), torch.empty(E, device=dev)
        fc_bn1d_backward(L.load(), dy.contiguous(), pooled, xhat, rstd, gamma, dw, db, dg, dbe, torch.empty(B * E, device=dev))
        return None, dw, db, dg, dbe, None, None, None


class _BN1d(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long))


_LOOKAHEAD_STREAMS = {}


def lookahead_stream(device, i):
    """Side stream i of `device` for look-ahead work, ONE set per process: HIP multiplexes streams onto a few hardware queues
    (4 by default), so per-model streams end up sharing a queue with the main stream from the second model on -- measured: the
    second model of a process lost the whole look-ahead gain (12.0 k -> 9.8 k img/s) until the streams became process-wide."""
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), i)
    st = _LOOKAHEAD_STREAMS.get(key)
    if st is None:
        st = _LOOKAHEAD_STREAMS[key] = torch.cuda.Stream(device=device)
    return st


class EncoderCNN(nn.Module):
    """models.py:9-29.  `arch`/`compute_dtype` are build extensions (defaults = the reference: ResNet-152).
    compute_dtype: 'bf16' (MFMA bf16, f32 accumulate; throughput) or 'f32' (exact-f32 MFMA; parity)."""

    def __init__(self, embed_size, arch=RESNET152, compute_dtype="bf16"):
        super().__init__()
        if arch == "inception_v3":                          # BASELINE configs[3]; the attribute keeps the reference's name
            from .inception import InceptionStack
            self.resnet = InceptionStack(embed_size)
        else:
            self.resnet = ResNetStack(embed_size, arch)     # frozen stack + trainable fc (models.py:13-16)
        self.bn = _BN1d(embed_size)                         # models.py:17
        self.compute_dtype = compute_dtype
        # GROUPED look-ahead (ResNet stacks, bf16, train mode): `lookahead_groups` = G later batches run as ONE op program
        # (`ConvStackProgram(groups=G)`: every launch covers G batches, per-batch BatchNorm statistics, results bit-identical per
        # batch) -- half the launch boundaries and twice the workgroups per launch of the frozen stack.  1 = one program per batch.
        env_g = os.environ.get("SAT_LOOKAHEAD_GROUPS")
        arch_name = arch if isinstance(arch, str) else ""
        self.lookahead_groups = max(1, int(env_g)) if env_g else self.LOOKAHEAD_GROUPS_BY_ARCH.get(arch_name, self.LOOKAHEAD_GROUPS)
        env = os.environ.get("SAT_LOOKAHEAD_DEPTH")
        self.lookahead_depth = int(env) if env else self.LOOKAHEAD_DEPTH.get(arch if isinstance(arch, str) else "",
                                                                              3 * self.lookahead_groups)
        # side streams the stacks in flight are spread over (round robin in prefetch order); None = one per stack in flight.  Fewer
        # streams than stacks queue a later batch's stack BEHIND an earlier one's on the same hardware queue (it starts the moment
        # that one ends, without waiting for the host) -- for steps that need a hardware queue for something else (RCCL: trainer.py)
        env_s = os.environ.get("SAT_LOOKAHEAD_STREAMS")
        self.lookahead_streams = int(env_s) if env_s else None
        self._pf_seq = 0
        self._programs = {}      # insertion-ordered: least recently used first (`_program` re-inserts on a hit)
        self._lead_sigs = {}     # (shape, mode, weights): BatchNorm statistics signatures of the first program built (`_program`)
        self._inflight = []      # look-ahead (prefetch): [dict(images, taken, inst, ev, prog, sig, vers)], one per program run in flight
        self.register_load_state_dict_post_hook(lambda m, k: m._invalidate())
        # `encoder.resnet.load_state_dict(torchvision_sd)` -- the natural way to load the pretrained ResNet-152 the
        # reference uses (models.py:13) -- does not fire the parent's hook: hook the stack too
        self.resnet.register_load_state_dict_post_hook(lambda m, k: self._invalidate())

    def _invalidate(self):
        """cached op programs AND batches in flight belong to the old weights / device / mode"""
        self._programs.clear()
        self._lead_sigs.clear()
        self.resnet.__dict__.pop("_sig_params", None)       # weights_signature's cached parameter list
        if self._inflight:
            self.drop_lookahead()

    def train(self, mode=True):
        if bool(mode) != self.training and getattr(self, "_inflight", None):
            self.drop_lookahead()           # a stack prefetched with batch statistics must not feed an eval-mode forward
        return super().train(mode)

    def init_weights(self):
        """models.py:20-23."""
        self.resnet.fc.weight.data.normal_(0.0, 0.02)
        self.resnet.fc.bias.data.fill_(0)

    def _apply(self, fn, *a, **k):
        self._invalidate()          # device / dtype moves invalidate cached device pointers
        return super()._apply(fn, *a, **k)

    def _program(self, images, instance=None, groups=1):
        """instance None: the program `forward` runs (updates running statistics itself).  instance 0, 1, ...: independent
        copies (own activations, statistics accumulators, graphs) with DEFERRED running-statistics updates, for batches in
        flight next to each other on side streams (TrainStep.prefetch_encoder); groups > 1: a copy that runs that many batches
        per launch (`prefetch_many`)."""
        N, _, H, W = images.shape
        dt = L.SAT_BF16 if self.compute_dtype == "bf16" else L.SAT_F32
        key = (N, H, W, dt, self.training, str(images.device), weights_signature(self.resnet), instance, groups)
        prog = self._programs.pop(key, None)
        if prog is not None:
            self._programs[key] = prog                      # most recently used last
        else:
            # room for BOTH modes of one shape with every look-ahead instance (the reference alternates train and eval,
            # train.py:157-159: None + depth instances each), plus a partial last batch; evict the least recently used one
            # program at a time -- a program is ~0.9 GB of activations and its captured graphs at cfg 2
            cap = 2 * (2 * self._n_slots() + 2) + 2
            while len(self._programs) >= cap:
                old = next(iter(self._programs))
                if any(e["prog"] is self._programs[old] for e in self._inflight):
                    break                                   # never evict a program with a batch in flight
                del self._programs[old]
            make = getattr(self.resnet, "program", None)           # a stack with its own op program (Inception-v3)
            # Every program of one (shape, mode, weights) runs its convs on kernel variants of the SAME BatchNorm statistics
            # signature (tile shape / summation order), so a batch gets bit-identical features whichever program runs it.  The
            # first program built tunes freely and leads; with the grouped look-ahead on that should be a grouped one (the
            # tile shapes that win at `lookahead_groups` batches per launch are not the ones that win at one), so build it
            # first when an ungrouped program is asked for
            lead = key[:7]
            grouped_la = dt == L.SAT_BF16 and self.lookahead_depth > 0 and self.lookahead_groups > 1
            if lead not in self._lead_sigs and groups == 1 and grouped_la:
                self._program(images, instance="g0", groups=self.lookahead_groups)
            if make is not None:                         # a stack with its own op program (Inception-v3)
                prog = make(N, H, W, dt, self.training, images.device, groups=groups, signatures=self._lead_sigs.get(lead))
            else:
                prog = ConvStackProgram(self.resnet, N, H, W, dt, self.training, images.device, groups=groups,
                                        signatures=self._lead_sigs.get(lead))
            if lead not in self._lead_sigs:
                self._lead_sigs[lead] = prog.signatures()
            self._programs[key] = prog
            if instance is not None:
                prog.defer_running_stats()
        return prog

    # -- look-ahead: the frozen stack of LATER batches on side streams ---------------------------------------------------
    # stacks in flight.  Measured on MI355X at batch 64, per stack: 5.68 ms alone, 4.40 with two in flight, 4.33 with three (with
    # 8 hardware queues; 4.86 with HIP's default 4, where the third stream shares a queue)
    # whole ResNet-152 step: 5.25 ms at depth 2, 5.10 at depth 3, 5.38 at depth 4; Inception-v3 299x299: 5.68 at 2, 5.98 at 3
    # Inception-v3 (configs[3]): THREE batches per launch, two runs in flight -- its launches are smaller than ResNet-152's (94 convs, many
    # on 17 x 17 and 8 x 8 maps), so they gain more from a third batch per launch, and its step is bound by the decoder (two LSTM layers
    # of hidden 1024), which leaves the Infinity Cache room for six batches of activations (round 5, one box, interleaved,
    # tools/run_gpu_inception_g.sh: G = 2 / depth 4 14152 img/s, conv launches 0.132 of peak; G = 3 / depth 6 14368, 0.143; G = 4 / depth 8
    # 14097, 0.150; G = 4 / depth 4 12622)
    LOOKAHEAD_DEPTH = {"inception_v3": 6}
    LOOKAHEAD_GROUPS = 2
    LOOKAHEAD_GROUPS_BY_ARCH = {"inception_v3": 3}

    # Look-ahead RUN SLOTS: at most `lookahead_depth // lookahead_groups` op-program runs are in flight (3 by default: more than
    # three side streams beside the main one cost a hardware queue), each on its slot's side stream; a slot holds a
    # grouped run (instance "g<k>", `lookahead_groups` batches) or a single one (instance k)
    def _n_slots(self):
        return max(1, self.lookahead_depth // max(1, self.lookahead_groups))

    def _slot_stream(self, device, slot):
        """side stream of run slot `slot`: one per slot, or -- `lookahead_streams` fewer than slots -- round robin in prefetch
        order (a later run then queues behind an earlier one on its hardware queue)"""
        n_slots = self._n_slots()
        n_streams = self.lookahead_streams or n_slots
        idx = slot if (n_streams >= n_slots and slot < n_slots) else self._pf_seq % n_streams
        self._pf_seq += 1
        return lookahead_stream(device, idx)

    def _free_slot(self, extra=False):
        busy = {e["slot"] for e in self._inflight}
        for k in range(self._n_slots() + (1 if extra else 0)):
            if k not in busy:
                return k
        return None

    def _is_in_flight(self, images):
        # (a tensor already consumed from a group that is only partly taken is NOT in flight any more: a staging buffer refilled
        # and handed in again must start a new run instead of silently returning False -- ADVICE r4)
        return any(im is images and not e["taken"][g] for e in self._inflight for g, im in enumerate(e["images"]))

    def _launch(self, ims, slot, groups):
        dev = ims[0].device
        inst = ("g%d" % slot) if groups > 1 else slot
        stream = self._slot_stream(dev, slot)
        stream.wait_stream(torch.cuda.current_stream(dev))             # the images, and this instance's previous consumers
        for im in ims:
            ready = getattr(im, "_sat_ready_event", None)              # a DevicePrefetcher copy still in flight on its own stream
            if ready is not None:
                stream.wait_event(ready)
        with torch.cuda.stream(stream), torch.no_grad():
            prog = self._program(ims[0], instance=inst, groups=groups)
            prog.run(ims if groups > 1 else ims[0])
            for im in ims:
                im.record_stream(stream)                               # the side stream reads the tensor: the allocator must know
            ev = torch.cuda.Event()
            ev.record(stream)
        self._inflight.append(dict(images=list(ims), taken=[False] * len(ims), slot=slot, ev=ev, prog=prog,
                                   sig=weights_signature(self.resnet), vers=[im._version for im in ims]))

    def prefetch(self, images, _extra=False):
        """Start the conv stack (frozen, `no_grad`: models.py:14-15, 25-27) of a LATER batch on a side stream.  Its pooled
        features depend on the images and the frozen weights only, not on the optimizer steps in between, so computing them
        early changes nothing but the schedule: up to three stacks run next to each other (one's HBM-bound
        BatchNorm passes and under-filled launches under the other's convs) and under the current batch's head / decoder /
        backward / optimizer.  Each batch keeps its own BatchNorm batch statistics (separate program instances); the model's
        running statistics are updated when the batch is consumed, i.e. in batch order.  `forward(images)` /
        `pooled_features(images)` / `TrainStep.step(images, ...)` of the SAME tensor object later picks the result up.
        Returns False (and does nothing) when the tensor is already in flight or every run slot is taken."""
        if images is None or images.dim() != 4 or self._is_in_flight(images):
            return False
        slot = self._free_slot(extra=_extra)
        if slot is None:
            return False
        L.require_gpu(images, "images")
        self._launch([images], slot, 1)
        return True

    def prefetch_many(self, images_list, last=None, own_stack=False):
        """`prefetch` for the next few batches IN ORDER.  With `lookahead_groups` = G > 1 (bf16) G batches that are not in flight
        yet start together as ONE grouped program (every launch of the stack covers G batches; each batch's statistics and
        features are bit for bit those of its own ungrouped run); a batch left over is started alone when it is the very next
        one or at the END OF THE DATA (no partner will come).  `last`: True / False says explicitly whether the list reaches the
        end of the data (`DevicePrefetcher.upcoming_images()` sets it on the list it returns); None infers it from a list shorter
        than the look-ahead window -- right for callers that always hand in `lookahead_depth` batches when they have them
        (`bench.py`), wrong for a prefetcher of smaller depth, which would start a single per step and never a group.
        `own_stack`: the caller runs the CURRENT batch's stack itself right after this call (`TrainStep` when that batch was not
        prefetched: the first step of a loop).  Returns the number of batches started."""
        if last is None:
            last = getattr(images_list, "last", None)
        ims = [im for im in images_list if im is not None and im.dim() == 4]
        G = self.lookahead_groups if self.compute_dtype == "bf16" else 1
        started = 0
        new = [im for im in ims if not self._is_in_flight(im)]
        # COLD START (nothing in flight, and the caller is about to run the current batch's own stack beside what starts here): that
        # stack takes one of the pipeline's places, so one grouped run fewer starts now -- the next call starts it, behind the first
        # hand-over.  With all `n_slots` runs AND the own stack started together, four stacks share the chip, all finish at the same
        # moment (21 ms into a region, profiles/r05_step_timeline.txt) and the refills then trickle in one decoder step apart: 18.45-18.53
        # -> 18.72-18.80 k img/s at the contract's 20-step regions (interleaved on one box; one run fewer still: no better than before)
        cap = max(1, self._n_slots() - 1) if (own_stack and not self._inflight) else None
        if G > 1:
            while len(new) >= G:
                if cap is not None and started >= cap * G:
                    return started                                      # (the rest starts with the next call)
                grp = new[:G]
                if len({tuple(im.shape) for im in grp}) != 1 or len({id(im) for im in grp}) != G:
                    break                                               # ragged last batch / the same tensor twice: singles below
                slot = self._free_slot()
                if slot is None:
                    break
                for im in grp:
                    L.require_gpu(im, "images")
                self._launch(grp, slot, G)
                new = new[G:]
                started += G
            # a batch left without a partner starts alone when it is the very next one (it must not wait: one slot beyond the
            # regular ones is its), or when the caller's list is shorter than the look-ahead window -- the end of the data: no
            # partner will come, and started now its stack runs beside the last groups instead of alone behind them
            tail = bool(last) if last is not None else len(ims) < self.lookahead_depth
            for im in new:
                if im is ims[0]:
                    started += 1 if self.prefetch(im, _extra=True) else 0
                elif tail:
                    started += 1 if self.prefetch(im) else 0
            return started
        for im in new:
            started += 1 if self.prefetch(im) else 0
        return started

    def build_lookahead(self, images):
        """Build (autotune, capture the hipGraphs of) every op program the look-ahead of batches shaped like `images` will use,
        now instead of inside the first steps: each look-ahead instance runs four times on `images` (both statistics parities,
        eager then captured).  Touches no model state: look-ahead instances keep their running-statistics updates deferred, and
        nothing here applies them."""
        L.require_gpu(images, "images")
        G = self.lookahead_groups if self.compute_dtype == "bf16" else 1
        progs = []
        with torch.no_grad():
            if G > 1:
                progs += [(self._program(images, instance="g%d" % k, groups=G), [images] * G) for k in range(self._n_slots())]
                progs += [(self._program(images, instance=0), images)]      # the single a left-over batch runs on
            else:
                progs += [(self._program(images, instance=k), images) for k in range(self._n_slots())]
            for prog, arg in progs:
                for _ in range(4):
                    prog.run(arg)
        torch.cuda.current_stream(images.device).synchronize()

    def _take_prefetched(self, images):
        """(program instance, group index) of a prefetched `images` whose run has finished (the current stream now waits for
        it), or None.  The caller reads `prog.pooled_of(g)` and then calls `prog.apply_running_stats(g)` -- both on the current
        stream."""
        for k, e in enumerate(self._inflight):
            for g, im in enumerate(e["images"]):
                if im is images and not e["taken"][g]:
                    e["taken"][g] = True
                    if all(e["taken"]):
                        del self._inflight[k]
                    torch.cuda.current_stream(images.device).wait_event(e["ev"])
                    # conv weights rewritten since (version counters): the stack in flight used the old ones -> recompute;
                    # the same for the IMAGES: a staging buffer refilled in place (copy_, normal_, ...) between prefetch and
                    # forward is the same tensor object with other contents (its version counter moved)
                    ok = e["sig"] == weights_signature(self.resnet) and e["vers"][g] == images._version
                    return (e["prog"], g) if ok else None
        return None

    def drop_lookahead(self):
        """Forget batches in flight (their results are discarded; the model's running statistics never see them)."""
        for e in self._inflight:
            e["ev"].synchronize()
        self._inflight = []

    def refresh_weights(self):
        """Drop the cached op programs (and their kernel-layout weight copies); needed only after writing conv weights
        through `.data`, which no version counter sees."""
        self._invalidate()

    def _pooled_raw(self, images):
        """The program-owned pooled buffer (overwritten by the next forward of the same shape): internal use within
        one step only (`TrainStep`)."""
        L.require_gpu(images, "images")
        with torch.no_grad():
            return self._program(images).run(images)

    def pooled_features(self, images):
        """conv stack + global average pool: f32 [B, 2048] (no autograd: the stack is frozen, models.py:14-15).
        Returns a tensor the caller owns (a copy of the program's output buffer, B x 2048 f32)."""
        hit = self._take_prefetched(images)
        if hit is not None:
            prog, g = hit
            out = prog.pooled_of(g).clone()
            prog.apply_running_stats(g)             # batch order = consumption order
            return out
        return self._pooled_raw(images).clone()

    def forward(self, images):
        """Extract the image feature vectors (models.py:25-29)."""
        # the head's backward needs `pooled`: it must not alias the program's buffer, which a second forward (two
        # micro-batches before one backward, or model(images) followed by model.sample(images)) would overwrite
        pooled = self.pooled_features(images) if (torch.is_grad_enabled() or self._inflight) else self._pooled_raw(images)
        out = _HeadFn.apply(pooled, self.resnet.fc.weight, self.resnet.fc.bias, self.bn.weight, self.bn.bias,
                            self.bn.running_mean, self.bn.running_var, self.training)
        if self.training:
            L.counter_add(self.bn.num_batches_tracked)
        return out


# ------------------------------------------------------------------------------------------------------
# decoder
class _LSTMParams(nn.Module):
    """Parameter holder with nn.LSTM's names and default init U(-1/sqrt(H), 1/sqrt(H)) (models.py:36)."""

    def __init__(self, input_size, hidden_size, num_layers):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        k = 1.0 / (hidden_size ** 0.5)
        for l in range(num_layers):
            in_sz = input_size if l == 0 else hidden_size
            for name, shape in (("weight_ih", (4 * hidden_size, in_sz)), ("weight_hh", (4 * hidden_size, hidden_size)),
                                ("bias_ih", (4 * hidden_size,)), ("bias_hh", (4 * hidden_size,))):
                setattr(self, "%s_l%d" % (name, l), nn.Parameter(torch.empty(*shape).uniform_(-k, k)))

    def layer(self, l):
        return tuple(getattr(self, "%s_l%d" % (n, l)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


class _Weight(nn.Module):
    def __init__(self, *shape, bias=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*shape))
        if bias is not None:
            self.bias = nn.Parameter(torch.zeros(bias))


def draw_ss_seed():
    """The 63-bit seed of one scheduled-sampling forward, from torch's CPU default generator (`torch.manual_seed` reproduces a run)"""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())


def _as_f32(value):
    """value as the float32 the kernel receives (None when it is no number)"""
    try:
        return float(torch.tensor(float(value), dtype=torch.float32))
    except (TypeError, ValueError, OverflowError):
        return None


def check_sample_args(temperature, top_k, top_p, num_samples, seed):
    """The arguments of `sample_stochastic` as (temperature, top_k, top_p, num_samples, seed or None); a ValueError names the bad
    one.  Host arithmetic only: runs before the library is loaded."""
    import math
    tau, p = _as_f32(temperature), _as_f32(top_p)
    if isinstance(temperature, bool) or tau is None or not math.isfinite(tau) or tau <= 0:
        raise ValueError("temperature must be a finite number > 0 (as float32), got %r" % (temperature,))
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0 or top_k > 2 ** 31 - 1:
        raise ValueError("top_k must be an int >= 0 (0: no top-k filter), got %r" % (top_k,))
    if isinstance(top_p, bool) or p is None or not 0 < p <= 1 or not 0 < float(top_p) <= 1:
        raise ValueError("top_p must be in (0, 1] (1: no nucleus filter), got %r" % (top_p,))
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
        raise ValueError("num_samples must be an int >= 1, got %r" % (num_samples,))
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or seed < 0 or seed >= 2 ** 64):
        raise ValueError("seed must be None or an int in [0, 2^64), got %r" % (seed,))
    return tau, top_k, p, num_samples, seed


class BeamConstraints:
    """The checked constraints of one `sample_beam` call (`check_beam_constraints`).  `active`: something differs from the defaults,
    so the `_ex` entry points run; `struct(device)` is the `sat_beam_constraints` the library reads -- this object keeps the
    `suppress_ids` device tensor it points to alive."""

    def __init__(self, suppress_ids, min_length, no_repeat_ngram_size, block_repeat, length_penalty):
        self.suppress_ids, self.min_length, self.no_repeat_ngram_size = suppress_ids, min_length, no_repeat_ngram_size
        self.block_repeat, self.length_penalty = block_repeat, length_penalty
        self.active = bool(suppress_ids or min_length or no_repeat_ngram_size or block_repeat or length_penalty > 0)
        self._tensor = self._struct = None

    def struct(self, device):
        if self._struct is None or self._tensor is not None and self._tensor.device != torch.device(device):
            self._tensor = torch.tensor(self.suppress_ids, dtype=torch.int64, device=device) if self.suppress_ids else None
            self._struct = L.SatBeamConstraints(self._tensor.data_ptr() if self.suppress_ids else None, len(self.suppress_ids),
                                                self.min_length, self.no_repeat_ngram_size, int(self.block_repeat), self.length_penalty)
        return self._struct


BEAM_MAX_SUPPRESS, BEAM_MAX_STEPS, BEAM_MAX_VOCAB = 256, 64, 65536         # include/sat_hip.h, sat_beam_step_ex
_NO_CONSTRAINTS = BeamConstraints([], 0, 0, False, 0.0)


def check_beam_constraints(suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0,
                           end_id=None, vocab_size=None, steps=None):
    """The constraint arguments of the `sample_beam` methods as a `BeamConstraints`; a ValueError names the bad one -- everything
    the library refuses, and an `end_id` among `suppress_ids` (no hypothesis could ever finish).  Host arithmetic only: runs
    before the library is loaded."""
    import math
    if suppress_ids is None and block_repeat is False and type(min_length) is int and type(no_repeat_ngram_size) is int and \
            type(length_penalty) in (int, float) and min_length == 0 and no_repeat_ngram_size == 0 and length_penalty == 0 and \
            (end_id is None or type(end_id) is int):
        return _NO_CONSTRAINTS                              # the defaults: nothing to check, nothing to build

    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)

    if suppress_ids is None:
        ids = []
    else:
        try:
            ids = suppress_ids.tolist() if hasattr(suppress_ids, "tolist") else list(suppress_ids)
        except TypeError:
            raise ValueError("suppress_ids must be None or a sequence of token ids, got %r" % (suppress_ids,))
    if any(not is_int(v) or v < 0 or (vocab_size is not None and v >= vocab_size) for v in ids):
        raise ValueError("suppress_ids must be ints in [0, vocab_size), got %r" % (ids,))
    if len(ids) > BEAM_MAX_SUPPRESS:
        raise ValueError("at most %d suppress_ids, got %d" % (BEAM_MAX_SUPPRESS, len(ids)))
    if end_id is not None and not is_int(end_id):
        raise ValueError("end_id must be None or an int, got %r" % (end_id,))
    eid = -1 if end_id is None else end_id
    if eid >= 0 and eid in ids:
        raise ValueError("end_id %d is among suppress_ids: no hypothesis could finish" % eid)
    if not is_int(min_length) or min_length < 0:
        raise ValueError("min_length must be an int >= 0, got %r" % (min_length,))
    if min_length > 0 and eid < 0:
        raise ValueError("min_length > 0 needs an end_id >= 0 (the token it holds back)")
    if not is_int(no_repeat_ngram_size) or no_repeat_ngram_size < 0:
        raise ValueError("no_repeat_ngram_size must be an int >= 0 (0: off), got %r" % (no_repeat_ngram_size,))
    if not isinstance(block_repeat, (bool, int)) or block_repeat not in (0, 1):
        raise ValueError("block_repeat must be a bool, got %r" % (block_repeat,))
    alpha = _as_f32(length_penalty)
    if isinstance(length_penalty, bool) or alpha is None or not math.isfinite(alpha) or alpha < 0:
        raise ValueError("length_penalty must be a finite number >= 0 (as float32; 0: off), got %r" % (length_penalty,))
    c = BeamConstraints(ids, min_length, no_repeat_ngram_size, bool(block_repeat), alpha)
    if ids or min_length or no_repeat_ngram_size or block_repeat:
        if steps is not None and steps > BEAM_MAX_STEPS:
            raise ValueError("a constrained beam search runs at most %d steps, got %d" % (BEAM_MAX_STEPS, steps))
        if vocab_size is not None and vocab_size > BEAM_MAX_VOCAB:
            raise ValueError("a constrained beam search serves a vocabulary of at most %d, got %d" % (BEAM_MAX_VOCAB, vocab_size))
    return c


class SampleConstraints:
    """The checked constraints of one `sample_stochastic` call (`check_sample_constraints`).  `active`: something differs from the
    defaults, so the `_ex` entry points run; `struct(device)` is the `sat_sample_constraints` the library reads -- this object
    keeps the `suppress_ids` device tensor it points to alive."""

    def __init__(self, suppress_ids, min_length, no_repeat_ngram_size, block_repeat, repetition_penalty, end_id):
        self.suppress_ids, self.min_length, self.no_repeat_ngram_size = suppress_ids, min_length, no_repeat_ngram_size
        self.block_repeat, self.repetition_penalty, self.end_id = block_repeat, repetition_penalty, end_id
        self.active = bool(suppress_ids or min_length or no_repeat_ngram_size or block_repeat or repetition_penalty != 1.0)
        self._tensor = self._struct = None

    def struct(self, device):
        if self._struct is None or self._tensor is not None and self._tensor.device != torch.device(device):
            self._tensor = torch.tensor(self.suppress_ids, dtype=torch.int64, device=device) if self.suppress_ids else None
            self._struct = L.SatSampleConstraints(self._tensor.data_ptr() if self.suppress_ids else None, len(self.suppress_ids),
                                                  self.min_length, self.no_repeat_ngram_size, int(self.block_repeat),
                                                  self.repetition_penalty, self.end_id)
        return self._struct


SAMPLE_MAX_STEPS = 64                                                       # include/sat_hip.h, sat_sample_filtered_ex
_NO_SAMPLE_CONSTRAINTS = SampleConstraints([], 0, 0, False, 1.0, -1)


def check_sample_constraints(suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False, repetition_penalty=1.0,
                             end_id=None, vocab_size=None, steps=None):
    """The constraint arguments of the `sample_stochastic` methods as a `SampleConstraints`; a ValueError names the bad one --
    everything the library refuses, and an `end_id` among `suppress_ids`.  The ids, `min_length`, `no_repeat_ngram_size` and
    `block_repeat` are checked by `check_beam_constraints`, whose rules they are.  Host arithmetic only: runs before the library is
    loaded."""
    import math
    if suppress_ids is None and block_repeat is False and type(min_length) is int and type(no_repeat_ngram_size) is int and \
            type(repetition_penalty) in (int, float) and min_length == 0 and no_repeat_ngram_size == 0 and repetition_penalty == 1 and \
            (end_id is None or type(end_id) is int):
        return _NO_SAMPLE_CONSTRAINTS                       # the defaults: nothing to check, nothing to build
    b = check_beam_constraints(suppress_ids, min_length, no_repeat_ngram_size, block_repeat, 0.0, end_id, vocab_size)
    theta = _as_f32(repetition_penalty)
    if isinstance(repetition_penalty, bool) or theta is None or not math.isfinite(theta) or theta <= 0:
        raise ValueError("repetition_penalty must be a finite number > 0 (as float32; 1: off), got %r" % (repetition_penalty,))
    c = SampleConstraints(b.suppress_ids, b.min_length, b.no_repeat_ngram_size, b.block_repeat, theta, -1 if end_id is None else end_id)
    if c.active and steps is not None and steps > SAMPLE_MAX_STEPS:
        raise ValueError("a constrained stochastic decode runs at most %d steps, got %d" % (SAMPLE_MAX_STEPS, steps))
    return c


def check_beam_groups(beam_size, num_beam_groups=1, diversity_penalty=0.0):
    """The group arguments of the `sample_beam` methods (include/sat_hip.h, sat_beam_step_groups) -> (G, penalty as float32); a
    ValueError names the bad one.  Host arithmetic only: runs before the library is loaded."""
    import math
    if num_beam_groups == 1 and type(num_beam_groups) is int and type(diversity_penalty) in (int, float) and diversity_penalty == 0:
        return 1, 0.0                                       # the defaults: nothing to check
    G = num_beam_groups
    if not isinstance(G, int) or isinstance(G, bool) or G < 1:
        raise ValueError("num_beam_groups must be an int >= 1, got %r" % (G,))
    if int(beam_size) % G != 0:
        raise ValueError("beam_size %d is not divisible by num_beam_groups %d" % (int(beam_size), G))
    lam = _as_f32(diversity_penalty)
    if isinstance(diversity_penalty, bool) or lam is None or not math.isfinite(lam) or lam < 0:
        raise ValueError("diversity_penalty must be a finite number >= 0 (as float32), got %r" % (diversity_penalty,))
    if lam > 0 and G == 1:
        raise ValueError("diversity_penalty %r needs num_beam_groups > 1: one group has nothing to differ from" % (diversity_penalty,))
    return G, lam


def stochastic_result(ids, logprobs, logits, alphas=None):
    """What a `sample_stochastic` returns: ids, then -- in this order, each only where asked for (not None) -- the dict(logp, kept),
    the logits and the attention maps; one value alone, else a tuple"""
    out = [ids] + [x for x in (logprobs, logits, alphas) if x is not None]
    return out[0] if len(out) == 1 else tuple(out)


def check_dropout_p(value, name):
    """A dropout probability as the float32 the kernel receives; a ValueError names the attribute `name` unless it is a finite
    number in [0, 1).  Host arithmetic only: runs before the library is loaded."""
    import math
    p = _as_f32(value)
    if isinstance(value, bool) or p is None or not math.isfinite(p) or not 0 <= p < 1:
        raise ValueError("%s must be a finite number in [0, 1) (as float32), got %r" % (name, value))
    return p


def refuse_dropout_with(active, what):
    """Dropout inside the step loops that project within one library call (scheduled sampling, the rollouts) is not built:
    `active` names the dropout attributes that are on, `what` the caller's side of the combination"""
    if active:
        raise NotImplementedError("%s with %s: the dropout mask is applied between library calls, and this loop projects inside "
                                  "one (set %s to 0 for it)" % (" / ".join(active), what, " / ".join(active)))


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, captions, pi, ss, dropout, names, *tensors):
        params = dict(zip(names, tensors))
        sampling = None if ss is None else (ss["prob"], ss["seed"], ss["rank"])
        logits, tapes = decoder_forward(L.load(), features, params, captions, pi, ss=sampling, dropout=dropout)
        if ss is not None:              # scheduled sampling: ss = dict(prob, seed, rank) receives "used", the tokens fed
            ss["used"] = tapes["captions"]
        ctx.tapes, ctx.pi, ctx.names, ctx.params = tapes, pi, names, params
        V = params["linear.weight"].shape[0]
        return logits if logits.shape[1] == V else logits[:, :V]

    @staticmethod
    def backward(ctx, dlogits):
        g = _decoder_grads(ctx, dlogits)
        return (g["features"], None, None, None, None, None, *(g[n] for n in ctx.names))


def _decoder_grads(ctx, dlogits):
    """`decoder_backward` on the tapes a decoder Function's forward left in ctx: gradients by parameter name, plus "features" """
    g = {n: torch.empty_like(p) for n, p in ctx.params.items()}
    g["features"] = torch.empty(ctx.pi.B, ctx.params["embed.weight"].shape[1], device=dlogits.device)
    decoder_backward(L.load(), L.pad_rows4(dlogits), ctx.tapes, ctx.params, ctx.pi, g, None)
    return g


class _RolloutFn(torch.autograd.Function):
    """The sampled rollout of self-critical training; its backward is the teacher-forced backward on the tokens drawn"""

    @staticmethod
    def forward(ctx, features, steps, seed, rank, out, names, *tensors):
        params = dict(zip(names, tensors))
        out["ids"], logits, tapes, pi = rollout_forward(L.load(), features, params, steps, seed, rank)
        ctx.tapes, ctx.pi, ctx.names, ctx.params = tapes, pi, names, params
        V = params["linear.weight"].shape[0]
        return logits if logits.shape[1] == V else logits[:, :V]

    @staticmethod
    def backward(ctx, dlogits):
        g = _decoder_grads(ctx, dlogits)
        return (g["features"], None, None, None, None, None, *(g[n] for n in ctx.names))


class DecoderRNN(nn.Module):
    """models.py:31-67."""

    last_beam_norm_scores = last_beam_order = None     # set by a constrained `sample_beam` (None after a plain one)
    last_beam_groups = None                            # set by a grouped `sample_beam`: [B,K] i32, the group of the hypothesis at r

    def __init__(self, embed_size, hidden_size, vocab_size, num_layers):
        super().__init__()
        self.embed = _Weight(vocab_size, embed_size)                     # nn.Embedding (models.py:35)
        self.lstm = _LSTMParams(embed_size, hidden_size, num_layers)     # nn.LSTM(batch_first) (models.py:36)
        self.linear = _Weight(vocab_size, hidden_size, bias=vocab_size)  # nn.Linear (models.py:37)
        self.embed_size, self.hidden_size, self.vocab_size, self.num_layers = embed_size, hidden_size, vocab_size, num_layers
        self.ss_prob = 0                  # scheduled sampling (models.py:38; schedule: trainer.ss_prob_for_epoch), training mode only
        self.ss_rank = 0                  # data-parallel rank: a stream of draws of its own per rank
        self.last_ss_inputs = self.last_ss_seed = None   # tokens fed [B, T-1] and seed of the last sampled forward
        self.last_rollout_seed = None     # seed of the last `rollout`
        self.last_sample_seed = None      # seed of the last `sample_stochastic`
        # dropout, training mode only (masks: include/sat_hip.h `sat_dropout_f32`; rank `ss_rank`): `dropout_p` on the top layer's
        # output in front of `linear` (site num_layers), `lstm_dropout_p` on the output of every layer but the last as
        # nn.LSTM(dropout=) does (layer l: site l + 1; nothing to act on with one layer)
        self.dropout_p = self.lstm_dropout_p = 0.0
        self.last_dropout_seed = None     # seed of the last forward that dropped anything
        self._id_guard = None
        self.init_weights()

    def id_guard(self):
        dev = self.embed.weight.device
        if self._id_guard is None or self._id_guard.status.device != dev:
            self._id_guard = IdGuard(dev)
        return self._id_guard

    def init_weights(self):
        """models.py:41-45."""
        self.embed.weight.data.uniform_(-0.1, 0.1)
        self.linear.weight.data.uniform_(-0.1, 0.1)
        self.linear.bias.data.fill_(0)

    def forward(self, features, captions, lengths):
        """Decode image feature vectors and generate caption logits (models.py:47-54): f32 [sum(lengths), V],
        rows in time-major packed order.  In training mode with ss_prob > 0 the input of step t >= 2 is, with probability
        ss_prob, a token drawn from softmax(logits of step t-1) (scheduled sampling; seed drawn from torch's CPU generator);
        the tokens fed and the seed are kept as `last_ss_inputs` / `last_ss_seed`.  In training mode `dropout_p` / `lstm_dropout_p`
        drop activations (see `__init__`); the masks' seed, one `draw_ss_seed()` per forward that drops, stays on
        `last_dropout_seed`.  Dropout together with ss_prob > 0 raises NotImplementedError."""
        dropout = self.dropout_plan(sampling=self.training and self.ss_prob > 0)
        features = _f32c(features, "features")
        L.require_gpu(captions, "captions")
        if len(lengths) != features.shape[0]:
            raise ValueError("len(lengths) != batch size")
        pi = PackInfo.get(lengths, features.device)
        if pi.T > captions.shape[1] + 1:
            raise ValueError("a length exceeds captions.shape[1] + 1")
        if captions.dtype != torch.int64 or captions.stride(1) != 1:
            captions = captions.long().contiguous()
        if pi.T > 1:
            self.id_guard().submit(captions, pi.T - 1, self.vocab_size, "captions")
        ss = None
        if self.training and self.ss_prob > 0:
            ss = dict(prob=float(self.ss_prob), seed=draw_ss_seed(), rank=int(self.ss_rank))
        if dropout is not None:
            dropout = self.draw_dropout(dropout)
        names, tensors = zip(*self.named_parameters())
        out = _DecoderFn.apply(features, captions, pi, ss, dropout, names, *tensors)
        if ss is not None:
            self.last_ss_inputs, self.last_ss_seed = ss["used"], ss["seed"]
        return out

    def dropout_plan(self, sampling=False, what="ss_prob > 0 (scheduled sampling)"):
        """(p_out, p_lstm) of a training forward, or None when nothing is dropped (eval mode, both probabilities 0, or only
        `lstm_dropout_p` on a one-layer LSTM).  Host checks only, nothing drawn: ValueError for a probability outside [0, 1),
        NotImplementedError when masks are active and `sampling` says the forward is one of the step loops (`what`)."""
        p_out, p_lstm = check_dropout_p(self.dropout_p, "dropout_p"), check_dropout_p(self.lstm_dropout_p, "lstm_dropout_p")
        if not self.training:
            return None
        active = [n for n, p in (("dropout_p", p_out), ("lstm_dropout_p", p_lstm if self.num_layers > 1 else 0.0)) if p > 0]
        if sampling:
            refuse_dropout_with(active, what)
        return (p_out, p_lstm if self.num_layers > 1 else 0.0) if active else None

    def draw_dropout(self, plan):
        """`decoder_forward`'s dropout argument (p_out, p_lstm, seed, rank) for an active `dropout_plan`: draws the forward's seed"""
        self.last_dropout_seed = draw_ss_seed()
        return plan + (self.last_dropout_seed, int(self.ss_rank))

    def rollout(self, features, steps=20, num_samples=1):
        """`sample` with a DRAW from softmax(logits) where `sample` takes the arg-max, in training form (self-critical sequence
        training, Rennie et al. 2017): (ids i64 [B, steps], logits f32 [steps * B, V]), logits row t * B + b those of step t of row
        b.  The logits carry autograd: their backward is the teacher-forced backward on ids[:, :steps-1].  Training mode only.  The
        seed comes from torch's CPU generator (`draw_ss_seed`) and is kept as `last_rollout_seed`; the draws are `ss_rank`'s stream.
        Rows keep running behind their <end>: `scst_loss` masks them.
        num_samples = S > 1: S captions per image.  Every image's features are repeated to R = B * S rows (row r = b * S + s, as
        in `sample_stochastic`) and the same call runs on R rows with draw row r: ids [B, S, steps], logits [steps * R, V] with row
        t * R + r -- bit for bit the rollout of `features.repeat_interleave(S, 0)` from the same seed.  The R-row gradient of the features comes
        back summed per image (`sat_group_sum_rows`)."""
        from .scst import check_group, repeat_rows
        S = check_group(num_samples)[0]
        if not self.training:
            raise RuntimeError("DecoderRNN.rollout is a training forward (decoder.train()); eval mode decodes with sample()")
        self.dropout_plan(sampling=True, what="a rollout")
        features = repeat_rows(_f32c(features, "features"), S)
        seed = draw_ss_seed()
        names, tensors = zip(*self.named_parameters())
        out = {}
        logits = _RolloutFn.apply(features, int(steps), seed, int(self.ss_rank), out, names, *tensors)
        self.last_rollout_seed = seed
        ids = out["ids"]
        return (ids if S == 1 else ids.view(-1, S, ids.shape[1])), logits

    def score_captions(self, features, captions, lengths, *, cross=False, normalize="none", return_tokens=False):
        """The log-probability of GIVEN captions under this decoder (`score.CaptionScores`): with captions [C, T] i64 as the
        data loader gives them (`<start>` ... `<end>`) and `lengths` a Python list in ANY order, step t predicts captions[c][t]
        for t < lengths[c] -- the rows `forward` is trained on against pack_padded_sequence(captions, lengths) (models.py:47-53).
        Paired (features [C, E]): logp f64 [C].  cross=True (features [B_img, E]): logp f64 [B_img, C], every caption under
        every image, chunked over images so that one library call's workspace stays under `score.WORKSPACE_BUDGET`.
        length i32 [C]; token_logp f32 [..., T] with return_tokens (+0.0 beyond a caption's length); score = logp
        (normalize="none") or logp / length ("length").  Results come back in the caller's order.  One `sat_score_captions` call
        per chunk: the [N, V] logits never exist.  Eval or train mode (no dropout, no sampling: the model's own distribution);
        nothing is taped.  Caption ids are range-checked on the device (`id_guard`)."""
        from .score import decoder_score_captions
        return decoder_score_captions(self, features, captions, lengths, cross=cross, normalize=normalize,
                                      return_tokens=return_tokens)

    @torch.no_grad()
    def sample(self, features, states=None):
        """Greedy search, 20 steps (models.py:56-67; torch-0.1 keepdim semantics): i64 [B,20].
        `states`: None (zeros), (h0, c0) each [num_layers, B, H], or eval.py:82-89's stacked [2, B, H] tensor
        (`_initial_states`); the result is squeezed like models.py:67 ([20] at batch 1)."""
        lib = L.load()
        features, h, c, h_tmp, xe = self._decode_state(features, states, 1)
        dev, B = features.device, features.shape[0]
        H, V, E = self.hidden_size, self.vocab_size, self.embed_size
        st = L.stream()
        ids = torch.empty(B, 20, dtype=torch.int64, device=dev)
        wsb = lib.sat_vocab_argmax_ws_bytes(B, V)
        ws = torch.empty(max(wsb // 4, 4), device=dev)
        # the 20 steps (LSTM step, vocab projection + arg-max, embedding row) are enqueued by ONE library call: the loop was
        # host-bound when every launch came through ctypes (round 4: 0.72 ms per 20 steps at batch 64)
        L.check(lib.sat_greedy_decode(L.ptr(features), L.ptr(self.embed.weight), self._lstm_ptrs(), self.num_layers,
                                      L.ptr(self.linear.weight), L.ptr(self.linear.bias), B, E, H, V, 20, L.ptr(h), L.ptr(c),
                                      L.ptr(h_tmp), L.ptr(xe), ids.data_ptr(), ids.stride(0), L.ptr(ws), wsb, st), "sat_greedy_decode")
        return ids.squeeze()                # models.py:67: [20] at batch 1

    @torch.no_grad()
    def sample_stochastic(self, features, states=None, temperature=1.0, top_k=0, top_p=1.0, num_samples=1, seed=None,
                          return_logprobs=False, return_logits=False, *, suppress_ids=None, min_length=0, no_repeat_ngram_size=0,
                          block_repeat=False, repetition_penalty=1.0, end_id=None):
        """`sample` with a DRAW where it takes the arg-max: every step's token comes from softmax(logits / temperature) restricted
        to the top_k most likely tokens (0: all) and then to the nucleus, the shortest most-likely-first prefix that holds top_p of
        the remaining mass (1: all).  20 steps as ONE `sat_sample_decode` call, no tapes, eval or train mode; rows keep running
        behind their <end> (`kept_tokens` truncates).

        Returns ids i64 [B, 20]; with num_samples = S > 1 ids [B, S, 20] -- features and `states` (as for `sample`) are repeated
        per image and the draw row is b * S + s, so the S captions of an image differ.  (No squeeze: [1, 20] at batch 1.)
        return_logprobs: also a dict(logp=f32 [.., 20], the log-probability of every drawn token under the filtered distribution,
        kept=i32 [.., 20], the number of tokens the filters left).  return_logits: also the exact-f32 logits [20, B*S, V] of
        every step (last).  seed: None draws one from torch's CPU generator (`draw_ss_seed`: `torch.manual_seed` reproduces it);
        the seed used stays on `last_sample_seed`.  The draws are `ss_rank`'s stream and follow sat_vocab_sample's convention: with
        (temperature, top_k, top_p) = (1, 0, 1) the tokens are those `rollout` draws from the same seed; top_k=1 takes every step's
        arg-max (`sample`, up to ties between logits: its projection is another kernel with another summation order).

        Constraints (all off by default: the call is then the `sat_sample_decode` above; otherwise ONE `sat_sample_decode_ex`).
        They act on every step's row of logits BEFORE the top-k and nucleus cuts, so logp and kept are those of the constrained
        distribution; `return_logits` still hands back the raw logits.  The prefix of a row is what this decode drew for it so far.
        suppress_ids: up to 256 ids that are never drawn (<unk>, <pad>, <start>).  min_length: `end_id` is not drawn before that
        step (needs end_id).  no_repeat_ngram_size = n: no n-gram twice (n = 1: no token twice).  block_repeat: never the previous
        token again.  repetition_penalty = theta: the logit of every token already drawn is divided by theta when positive,
        multiplied when not (1: off; a ban wins).  The rules hold at every step of every row, also behind its <end>.  Rollouts,
        SCST and scheduled sampling (`sat_vocab_sample`: a banned policy would change the gradient's meaning), `Ensemble` and
        `validation_step` do not take them; there are no frequency / presence penalties and no length penalty (a sample has no
        ranking to re-order)."""
        tau, top_k, top_p, S, seed = check_sample_args(temperature, top_k, top_p, num_samples, seed)
        cons = check_sample_constraints(suppress_ids, min_length, no_repeat_ngram_size, block_repeat, repetition_penalty, end_id,
                                        self.vocab_size, 20)
        lib = L.load()
        features, h, c, h_tmp, xe = self._decode_state(features, states, S)
        dev, R = features.device, features.shape[0]
        H, V, E, steps = self.hidden_size, self.vocab_size, self.embed_size, 20
        if seed is None:
            seed = draw_ss_seed()
        ids = torch.empty(R, steps, dtype=torch.int64, device=dev)
        logp = torch.empty(R, steps, device=dev) if return_logprobs else None
        kept = torch.empty(R, steps, dtype=torch.int32, device=dev) if return_logprobs else None
        ldl = L.pad4(V)
        logits = torch.zeros(steps * R, ldl, device=dev) if return_logits else None
        wsb = lib.sat_sample_decode_ws_bytes(R, E, H, V, self.num_layers)
        ws, ws_ptr = L.workspace256(wsb, dev)
        head = (L.ptr(features), L.ptr(self.embed.weight), self._lstm_ptrs(), self.num_layers, L.ptr(self.linear.weight),
                L.ptr(self.linear.bias), R, E, H, V, steps, tau, top_k, top_p, seed, int(self.ss_rank), L.ptr(h), L.ptr(c), L.ptr(h_tmp),
                L.ptr(xe), ids.data_ptr(), ids.stride(0), L.ptr(logp), L.ptr(kept), L.ptr(logits), ldl)
        if cons.active:
            L.check(lib.sat_sample_decode_ex(*head, cons.struct(dev), ws_ptr, wsb, L.stream()), "sat_sample_decode_ex")
        else:
            L.check(lib.sat_sample_decode(*head, ws_ptr, wsb, L.stream()), "sat_sample_decode")
        self.last_sample_seed = seed
        shape = (R // S, S, steps) if S > 1 else (R, steps)
        return stochastic_result(ids.view(shape), dict(logp=logp.view(shape), kept=kept.view(shape)) if return_logprobs else None,
                                 logits.view(steps, R, ldl)[:, :, :V] if return_logits else None)

    def _decode_state(self, features, states, rows):
        """What `sample` / `sample_stochastic` hand the decode call for `rows` rows per image (row b * rows + r): the features f32
        [R, E], the state h, c [num_layers, R, H] as PRIVATE contiguous copies of `states` (`_initial_states`; state in, state out:
        the caller's tensors are never written), the scratch h_tmp of h's size and the embedding rows xe [R, E]"""
        features = _f32c(features, "features")
        h, c = self._initial_states(states, features.shape[0], features.device)
        if rows > 1:
            features = features.repeat_interleave(rows, 0).contiguous()
            h, c = h.repeat_interleave(rows, 1), c.repeat_interleave(rows, 1)
        h, c = h.clone().contiguous(), c.clone().contiguous()
        return features, h, c, torch.empty_like(h), torch.empty(features.shape[0], self.embed_size, device=features.device)

    def _lstm_ptrs(self):
        """HOST array of the LSTM's device pointers, (w_ih, w_hh, b_ih, b_hh) per layer: the `lstm_w` argument of the decode calls"""
        import ctypes as _C
        ptrs = []
        for l in range(self.num_layers):
            ptrs += [t.data_ptr() for t in self.lstm.layer(l)]
        return (_C.c_void_p * len(ptrs))(*ptrs)

    def _initial_states(self, states, B, dev):
        """The LSTM state `sample` starts from (models.py:56,61 hands `states` to nn.LSTM) as two f32 [num_layers, B, H]
        tensors.  Accepted: None (zeros); `(h0, c0)` each [num_layers, B, H] (nn.LSTM's own form) or, for one layer, [B, H];
        eval.py:82-89's stacked tensor [2, B, H] (= (h0, c0) of a one-layer LSTM) or [2, num_layers, B, H].  Anything else
        raises -- nothing is silently replaced by zeros."""
        Lh, H = self.num_layers, self.hidden_size
        if states is None:
            z = torch.zeros(2, Lh, B, H, device=dev)
            return z[0], z[1]
        if torch.is_tensor(states):
            if states.dim() not in (3, 4) or states.shape[0] != 2:
                raise ValueError("states tensor must be stacked (h0, c0): [2, B, H] or [2, num_layers, B, H], got %s"
                                 % (tuple(states.shape),))
            states = (states[0], states[1])
        if not isinstance(states, (tuple, list)) or len(states) != 2 or not all(torch.is_tensor(s) for s in states):
            raise TypeError("states must be None, a (h0, c0) pair of tensors or their stacked tensor")
        out = []
        for name, s in zip(("h0", "c0"), states):
            if s.dim() == 2 and Lh == 1:
                s = s.unsqueeze(0)
            if tuple(s.shape) != (Lh, B, H):
                raise ValueError("%s must be [num_layers=%d, B=%d, H=%d]%s, got %s"
                                 % (name, Lh, B, H, " (or [B, H])" if Lh == 1 else "", tuple(s.shape)))
            L.require_gpu(s, name)
            out.append(s.to(dtype=torch.float32).contiguous())
        return out[0], out[1]

    @torch.no_grad()
    def sample_beam(self, features, beam_size=5, end_id=None, steps=20, return_all=False, *, suppress_ids=None, min_length=0,
                    no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0, num_beam_groups=1, diversity_penalty=0.0):
        """Beam search over the same 20-step loop (`model2.py:113-114` is a stub in the reference).
        Returns the best hypothesis per image, i64 [B,steps]; with return_all also (ids [B,K,steps] best-first,
        scores [B,K] = sum of token log-probabilities).  beam_size=1, end_id=None is exactly `sample`.
        end_id (eval.py's `<end>`, id 2): a finished hypothesis only repeats end_id at no cost.
        Constraints (include/sat_hip.h, sat_beam_step_ex; all off by default, and then the call is the one it always was):
        suppress_ids are never emitted; end_id not in front of position min_length; no_repeat_ngram_size=n: no n-gram twice;
        block_repeat: no token twice in a row; length_penalty=alpha re-orders the K results by score / length^alpha once the
        search is over.  Scores are never renormalised: `scores` stays the raw sums, in the returned order; the normalised ones
        are kept as `last_beam_norm_scores` [B,K] and the permutation as `last_beam_order` [B,K] (the search rank of the hypothesis
        now at r) -- both None after an unconstrained call.  beam_size=1 with constraints is the constrained greedy decode.
        Diverse beam search (sat_beam_decode_groups; arXiv:1610.02424): num_beam_groups=G splits the K slots into G groups of K / G
        that search in order; a group's candidates lose diversity_penalty per slot of the groups in front that chose the same token
        at the same step.  The penalty steers the selection only: `scores` stay the raw sums.  The K results come back ordered by
        (normalised score, search slot) through the same rerank, with `last_beam_norm_scores` and `last_beam_order` set as for a
        constrained call and `last_beam_groups` [B,K] i32 = last_beam_order // (K / G), the group of the hypothesis now at r (None
        after an ungrouped call).  Constraints compose: bans are per row, applied before the selection."""
        cons = check_beam_constraints(suppress_ids, min_length, no_repeat_ngram_size, block_repeat, length_penalty, end_id,
                                      self.vocab_size, steps)
        G, lam = check_beam_groups(beam_size, num_beam_groups, diversity_penalty)
        lib = L.load()
        features = _f32c(features, "features")
        dev = features.device
        B, K = features.shape[0], int(beam_size)
        if K < 1 or K > 8:
            raise ValueError("beam_size must be in 1..8")
        H, V, E = self.hidden_size, self.vocab_size, self.embed_size
        st = L.stream()
        eid = -1 if end_id is None else int(end_id)
        ids = torch.empty(B, K, steps, dtype=torch.int64, device=dev)
        scores = torch.empty(B, K, device=dev)
        if self.last_beam_order is not None:
            self.last_beam_norm_scores = self.last_beam_order = self.last_beam_groups = None
        # every step (LSTM step, exact-f32 vocab projection, per-row log-softmax + top-K, per-image merge that also gathers the next
        # input's embedding rows, one (h, c) re-ordering launch) is enqueued by ONE library call (sat_beam_decode)
        if G > 1:
            wsb = lib.sat_beam_decode_groups_ws_bytes(B, K, E, H, V, self.num_layers, steps)
            ws, ws_ptr = L.workspace256(wsb, dev)
            norm, order = torch.empty(B, K, device=dev), torch.empty(B, K, dtype=torch.int32, device=dev)
            L.check(lib.sat_beam_decode_groups(L.ptr(features), L.ptr(self.embed.weight), self._lstm_ptrs(), self.num_layers,
                                               L.ptr(self.linear.weight), L.ptr(self.linear.bias), B, K, E, H, V, int(steps), eid,
                                               cons.struct(dev) if cons.active else None, G, lam, ids.data_ptr(), L.ptr(scores),
                                               L.ptr(norm), L.ptr(order), ws_ptr, wsb, st), "sat_beam_decode_groups")
            self.last_beam_norm_scores, self.last_beam_order, self.last_beam_groups = norm, order, order // (K // G)
        elif cons.active:
            wsb = lib.sat_beam_decode_ex_ws_bytes(B, K, E, H, V, self.num_layers, steps)
            ws, ws_ptr = L.workspace256(wsb, dev)
            norm, order = torch.empty(B, K, device=dev), torch.empty(B, K, dtype=torch.int32, device=dev)
            L.check(lib.sat_beam_decode_ex(L.ptr(features), L.ptr(self.embed.weight), self._lstm_ptrs(), self.num_layers,
                                           L.ptr(self.linear.weight), L.ptr(self.linear.bias), B, K, E, H, V, int(steps), eid,
                                           cons.struct(dev), ids.data_ptr(), L.ptr(scores), L.ptr(norm), L.ptr(order), ws_ptr, wsb, st),
                    "sat_beam_decode_ex")
            self.last_beam_norm_scores, self.last_beam_order = norm, order
        else:
            wsb = lib.sat_beam_decode_ws_bytes(B, K, E, H, V, self.num_layers, steps)
            ws, ws_ptr = L.workspace256(wsb, dev)
            L.check(lib.sat_beam_decode(L.ptr(features), L.ptr(self.embed.weight), self._lstm_ptrs(), self.num_layers,
                                        L.ptr(self.linear.weight), L.ptr(self.linear.bias), B, K, E, H, V, int(steps), eid,
                                        ids.data_ptr(), L.ptr(scores), ws_ptr, wsb, st), "sat_beam_decode")
        if return_all:
            return ids, scores
        return ids[:, 0].contiguous()


class ShowAndTell(nn.Module):
    """Encoder + decoder behind the reference trainer's single-module call contract (train.py:37,139;
    eval.py:93,99): `model(images, captions, lengths)` and `model.sample(images, state)`.
    state_dict keys: `encoder.*`, `decoder.*`."""

    last_beam_norm_scores = last_beam_order = None     # set by a constrained `sample_beam` (None after a plain one)
    last_beam_groups = None                            # set by a grouped `sample_beam`: [B,K] i32, the group of the hypothesis at r

    def __init__(self, embed_size, hidden_size, vocab_size, num_layers=1, arch=RESNET152, compute_dtype="bf16"):
        super().__init__()
        self.encoder = EncoderCNN(embed_size, arch, compute_dtype)
        self.decoder = DecoderRNN(embed_size, hidden_size, vocab_size, num_layers)

    @classmethod
    def from_trainer_args(cls, hidden_size, context_size, vocab_size, embed_size, opt=None, **kw):
        """The argument order of the model the reference trainer constructs, train.py:37
        `ShowAttendTellModel(opt.hidden_size, opt.embed_size, len(vocab), opt.embed_size, opt)`: hidden FIRST, then a
        context size this architecture has no use for, vocab, embed, and the options namespace (its `num_layers`,
        config.py:30, is honoured).  Dropping `ShowAndTell.from_trainer_args` in at that call site keeps every
        dimension where the trainer put it."""
        num_layers = int(getattr(opt, "num_layers", 1)) if opt is not None else 1
        return cls(embed_size, hidden_size, vocab_size, num_layers, **kw)

    def prefetch(self, images):
        """Start the frozen conv stack of a LATER batch on a side stream (`EncoderCNN.prefetch`)."""
        return self.encoder.prefetch(images)

    def prefetch_many(self, images_list):
        """... of the next few batches, in order (`EncoderCNN.prefetch_many`: two batches per program run)."""
        return self.encoder.prefetch_many(images_list)

    def forward(self, images, captions, lengths):
        return self.decoder(self.encoder(images), captions, lengths)

    def scst_forward(self, images, image_index, scorer, end_id=2, num_samples=1, baseline="greedy"):
        """The self-critical loss of one batch (`scst.SelfCritical`) behind the encoder's forward, so that `loss.backward()` also
        trains fc / bn.  image_index: the corpus image of every row, as for `CiderScorer.score`.  The `SelfCritical` object (its
        last_reward, last_baseline, last_ids) is kept as `last_scst`.  num_samples, baseline: `SelfCritical`'s -- S captions per
        image from ONE encoder pass, baseline "greedy" or "sample_mean" (leave-one-out; no greedy decode)."""
        from .scst import SelfCritical
        self.decoder.dropout_plan(sampling=True, what="a rollout (scst_forward)")            # before the encoder runs
        self.last_scst = SelfCritical(scorer, end_id, num_samples=num_samples, baseline=baseline)
        return self.last_scst(self.decoder, self.encoder(images), image_index)

    @torch.no_grad()
    def score_captions(self, images, captions, lengths, **kw):
        """`DecoderRNN.score_captions` (cross, normalize, return_tokens as there) behind the encoder in its current mode."""
        return self.decoder.score_captions(self.encoder(images), captions, lengths, **kw)

    @torch.no_grad()
    def sample(self, images, state=None):
        """eval.py:93,99 `model.sample(images, state)`: the state is handed to the decoder's LSTM (models.py:56,61)."""
        return self.decoder.sample(self.encoder(images), state)

    @torch.no_grad()
    def sample_beam(self, images, beam_size=5, end_id=None, return_all=False, *, suppress_ids=None, min_length=0,
                    no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0, num_beam_groups=1, diversity_penalty=0.0):
        """`DecoderRNN.sample_beam` behind the encoder, its constraints and beam groups included (checked before the encoder runs);
        `last_beam_norm_scores`, `last_beam_order` and `last_beam_groups` are the decoder's."""
        cons = dict(suppress_ids=suppress_ids, min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size,
                    block_repeat=block_repeat, length_penalty=length_penalty)
        check_beam_constraints(end_id=end_id, vocab_size=self.decoder.vocab_size, **cons)
        if check_beam_groups(beam_size, num_beam_groups, diversity_penalty)[0] > 1:
            cons.update(num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty)
        ids = self.decoder.sample_beam(self.encoder(images), beam_size, end_id, return_all=return_all, **cons)
        if self.decoder.last_beam_order is not None or self.last_beam_order is not None:
            self.last_beam_norm_scores, self.last_beam_order = self.decoder.last_beam_norm_scores, self.decoder.last_beam_order
            self.last_beam_groups = self.decoder.last_beam_groups
        return ids

    @torch.no_grad()
    def sample_stochastic(self, images, state=None, *, suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False,
                          repetition_penalty=1.0, end_id=None, **kw):
        """`DecoderRNN.sample_stochastic` behind the encoder: temperature, top_k, top_p, num_samples, seed, return_logprobs,
        return_logits and the constraints as there (checked before the encoder runs)."""
        check_sample_args(kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0), kw.get("num_samples", 1), kw.get("seed"))
        cons = dict(suppress_ids=suppress_ids, min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size,
                    block_repeat=block_repeat, repetition_penalty=repetition_penalty, end_id=end_id)
        if check_sample_constraints(vocab_size=self.decoder.vocab_size, steps=20, **cons).active:
            kw.update(cons)
        return self.decoder.sample_stochastic(self.encoder(images), state, **kw)


Encoder = EncoderCNN      # names BASELINE.json uses
Decoder = DecoderRNN
CaptionModel = ShowAndTell
