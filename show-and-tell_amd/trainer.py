"""Fused training step: the body of the reference's hot loop (`/root/reference/train.py:126-146`) for the
Show-and-Tell model, with every tensor op a libsat_hip.so kernel and no autograd:

    lengths-1, targets = pack(captions[:,1:])            train.py:134-135   sat_pack_targets
    outputs = model(images, captions[:,:-1], lengths)     train.py:139       sat_run_ops / sat_fc_bn1d_fwd /
                                                                             sat_embed_concat_fwd / sat_lstm_fwd / sat_vocab_logits_fwd
    loss = CrossEntropyLoss()(outputs, targets)           train.py:143       sat_ce_rows (gradient written in place)
    loss.backward()                                       train.py:144       sat_vocab_ce_bwd / sat_lstm_bwd / sat_embed_concat_bwd / sat_fc_bn1d_bwd
    clip_gradient (elementwise clamp) + Adam step         train.py:145-146   sat_clamp_adam_step (one launch)

MI355X-first layout: all trainable parameters live in ONE flat f32 buffer (module parameters are views of it),
with matching flat grad / Adam-m / Adam-v buffers.  The optimizer is one HBM-bound launch over 28 B/param and
the data-parallel gradient exchange is a handful of large RCCL all-reduces over contiguous buckets, launched
as each bucket's gradients become final and overlapped with the rest of the backward (`DataParallelStep`).
"""
import torch

from . import _lib as L
from .criterion import MAX_UL_STEPS, _check_smoothing, _check_unlikelihood
from .decoder import LSTMWorkspaces, VocabCE, decoder_backward, decoder_forward, rollout_forward
from .models import ShowAndTell, draw_ss_seed, fc_bn1d_backward, fc_bn1d_forward
from .optim import AVERAGED_NOTE, FlatAdam, check_accumulate_weight, check_max_norm, delegated, grad_accumulate, is_number
from .pack import PackInfo
from .scst import SelfCritical, ce_rows_weighted, check_group, group_sum_rows, scst_weights, scst_weights_group
from .watch import ResidencyWatch, StatusRing


import os as _os

# bf16 throughput mode (compute_dtype="bf16", BASELINE configs[1]): the vocab projection and its two gradient GEMMs run on the
# bf16 matrix pipe from per-step bf16 operand copies (sat_gemm_bf16.hip; f32 accumulate, f32 logits / CE / outputs / master
# weights).  SAT_DECODER_BF16=0 keeps them exact-f32 as in the parity mode (round 2's behaviour: 0.39 ms/step instead of ~0.1).
_DECODER_BF16 = _os.environ.get("SAT_DECODER_BF16", "1") != "0"


def lr_for_epoch(epoch, learning_rate=1e-3, decay_start=1, decay_every=3, decay_rate=0.8):
    """Epoch step decay of the reference trainer (train.py:101-107; defaults config.py:38-46)."""
    if epoch > decay_start and decay_start >= 1:
        return learning_rate * decay_rate ** ((epoch - decay_start) // decay_every)
    return learning_rate


def ss_prob_for_epoch(epoch, start=-1, increase_every=5, increase_prob=0.05, max_prob=0.25):
    """Scheduled-sampling probability of an epoch: the reference trainer's commented-out schedule (train.py:109-113; defaults
    config.py:50-57).  Before `start` (and with start < 0, the default: off) the probability is the initial 0."""
    if epoch > start and start >= 0:
        return min(increase_prob * ((epoch - start) // increase_every), max_prob)
    return 0.0


class FlatParams(FlatAdam):
    """The `FlatAdam` of a ShowAndTell model: the trainable parameters re-homed into its flat buffer in gradient-completion order
    (bucket 0 = vocab projection, bucket 1 = LSTM (top layer first), bucket 2 = encoder head + embedding), `slices` by name, the
    loss / fault slots behind the gradients, and `acc`, the accumulated twin of `grads`.  `names` / `layout` / `tensors` are in the
    order train.py:55 hands the parameters to optim.Adam (model.parameters() with requires_grad): the order of a state dict."""

    WORDS = ("max_grad_norm", "model has %d trainable", "load_optimizer_state_dict()")

    def __init__(self, model):
        dec, enc = model.decoder, model.encoder
        groups = [[("decoder.linear.weight", dec.linear.weight), ("decoder.linear.bias", dec.linear.bias)], [], []]
        for l in reversed(range(dec.num_layers)):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                groups[1].append(("decoder.lstm.%s_l%d" % (n, l), getattr(dec.lstm, "%s_l%d" % (n, l))))
        groups[2] = [("encoder.resnet.fc.weight", enc.resnet.fc.weight), ("encoder.resnet.fc.bias", enc.resnet.fc.bias),
                     ("encoder.bn.weight", enc.bn.weight), ("encoder.bn.bias", enc.bn.bias),
                     ("decoder.embed.weight", dec.embed.weight)]
        self.slices, self.buckets = {}, []
        off = 0
        for g in groups:
            start = off
            for name, p in g:
                self.slices[name] = (off, p.numel(), tuple(p.shape))
                off += L.pad4(p.numel())
            self.buckets.append((start, off))
        # 4 trailing floats: slot 0 carries this rank's loss term through the last bucket's all-reduce, slot 1 the step's fault
        # flag (TrainStep._fault_flag: non-zero on EVERY rank after the reduction when any rank's persistent LSTM launch gave up)
        self.loss_slot = off
        self.buckets[-1] = (self.buckets[-1][0], off + 4)
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        assert {n for n, _ in named} == set(self.slices), "the trainable parameters are those of the three buckets"
        super().__init__([self.slices[n] for n, _ in named], dec.linear.weight.device, tail=4)
        self.names = [n for n, _ in named]
        self.acc = None          # the accumulated gradient, a twin of `grads` (4 B/param): made by the first TrainStep.accumulate()
        self.rehome([p for _, p in named])

    def grad(self, name):
        o, n, shape = self.slices[name]
        return self.grads[o:o + n].view(shape)


class TrainStep:
    """One object = model + flat optimizer state; `step()` = one train.py:126-146 iteration on this GPU.
    label_smoothing (keyword, and a settable attribute; 0 <= value < 1): the teacher-forced step's criterion becomes
    nn.CrossEntropyLoss(label_smoothing=) -- `sat_ce_rows_ls` in place on the step's logits in the f32 mode, `sat_vocab_ce_fwd_bf16_ls`
    in the bf16 mode; with 0 both modes make exactly the calls they make without it.  Scheduled sampling and dropout compose: only
    the CE call changes.  The loss slot then holds the SMOOTHED loss; `last_nll` (1-element device tensor) holds THIS RANK's
    inv_denom * sum of the rows' plain NLL, for a perplexity -- it is not all-reduced: in a data-parallel step inv_denom is the
    global token count, so the ranks' values add up to the global NLL.  With label_smoothing == 0 the loss is the NLL and `last_nll`
    is the loss slot itself (which a data-parallel step does all-reduce).  `scst_step` and `validation_step` ignore the attribute:
    SCST weights its own rows, validation reports the plain CE of eval.py:95.
    unlikelihood (a settable, checked attribute like max_grad_norm, not a constructor argument; a finite value >= 0, default 0): token-level unlikelihood training (criterion.py's module
    docstring; arithmetic at `sat_ce_rows_ul` in include/sat_hip.h) -- every target row also pays that weight times
    sum_c -log(1 - p_c) over the distinct ground-truth tokens c of the earlier steps of its own caption.  The candidates are always
    the ground-truth targets, whatever scheduled sampling feeds.  `sat_ce_rows_ul` in place in the f32 mode,
    `sat_vocab_ce_fwd_bf16_ul` in the bf16 mode; with 0 both modes make exactly the calls they make without it.  Captions of more
    than 65 tokens (64 target steps) are a ValueError.  `last_ul` (1-element device tensor, None with 0) holds THIS RANK's inv_denom *
    sum of the rows' unweighted terms, rank-local like `last_nll`, which is then the plain NLL as with label smoothing.  `scst_step`
    and `validation_step` ignore it too."""

    def __init__(self, model, lr=1e-3, grad_clip=0.1, betas=(0.9, 0.999), eps=1e-8, label_smoothing=0.0):
        if not isinstance(model, ShowAndTell):
            raise TypeError("TrainStep drives a ShowAndTell model")
        L.require_gpu(model.decoder.linear.weight, "model")
        lib = L.load()                       # (before the parameters are re-homed: a missing library leaves the model as it was)
        self.model = model
        self.flat = FlatParams(model)
        self.lib = lib
        self.lr, self.grad_clip, self.betas, self.eps = lr, grad_clip, betas, eps
        self.label_smoothing = label_smoothing
        self.last_nll = self.last_ul = None
        self.buckets = self.flat.buckets
        self.flat_grad = self.flat.grads
        self._bufs = {}
        # "bf16": vocab projection + its gradient GEMMs on the bf16 matrix pipe (the throughput mode); "f32": exact-f32 MFMA
        self.decoder_gemm_dtype = "bf16" if (_DECODER_BF16 and model.encoder.compute_dtype == "bf16") else "f32"
        # sticky device-side fault word of this engine (sat_step_fault_flag): set by a step whose persistent LSTM recurrence gave
        # up, cleared by the host once it has raised for it; while it is set every clamp + Adam launch drops its update
        self._fault_sticky = torch.zeros(1, device=self.flat.params.device)
        self.fault_slot = self.flat.grads[self.flat.loss_slot + 1:self.flat.loss_slot + 2]
        # the LSTM workspaces this engine owns for good (their status words are folded into the step's fault flag)
        self.lstm_ws = LSTMWorkspaces(self.flat.params.device, watch=False)
        self._lag_ring = StatusRing(8)       # data-parallel steps: reduced fault flags in flight (_watch_fixed_lag)

    @property
    def label_smoothing(self):
        return self._label_smoothing

    @label_smoothing.setter
    def label_smoothing(self, value):
        self._label_smoothing = _check_smoothing(value)

    _unlikelihood = 0.0

    @property
    def unlikelihood(self):
        return self._unlikelihood

    @unlikelihood.setter
    def unlikelihood(self, value):
        self._unlikelihood = _check_unlikelihood(value)

    # -- the optimizer: `flat` (a `FlatAdam`: its docstring has the launch sequence and the drop rules) holds the state and these -----
    # settings, attributes here, not constructor arguments.  What is TrainStep's own:
    # max_grad_norm: `flat.max_norm` with 0.0 for "off"; taken over the whole flat gradient after the bucket all-reduces of a
    #   data-parallel step.  no_decay: NAMES from `flat.slices` that do not decay (`no_decay_names(model)`: biases, BatchNorm weight /
    #   bias); None decays every parameter, which is what torch does with one param group.
    # The skip word of every update is the step's fault word, so a faulted step moves neither parameters nor moments nor the
    #   average; its step_count is rolled back (`_on_fault`), and the EMA warm-up schedule follows the rollback.  `scst_step` and
    #   `DataParallelStep` come through `optimizer_step`; every rank computes the same bits from the same parameters, so the
    #   average is not exchanged.
    lib, lr, betas, eps, grad_clip = (delegated(k, "flat") for k in ("lib", "lr", "betas", "eps", "clip"))
    step_count, last_grad_norm, weight_decay = (delegated(k, "flat") for k in ("step_count", "last_grad_norm", "weight_decay"))
    ema_decay, ema_warmup, _averaged = (delegated(k, "flat") for k in ("ema_decay", "ema_warmup", "averaged"))
    _exempt, _params_list = delegated("exempt", "flat"), delegated("tensors", "flat")
    _no_decay = None

    @property
    def max_grad_norm(self):
        return self.flat.max_norm or 0.0

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        self.flat.max_norm = None if (is_number(value) and value == 0) else check_max_norm(value, "max_grad_norm")

    @property
    def no_decay(self):
        return self._no_decay

    @no_decay.setter
    def no_decay(self, names):
        if names is not None:
            if isinstance(names, (str, bytes)) or not hasattr(names, "__iter__"):
                raise ValueError("no_decay takes parameter NAMES (an iterable of str), or None")
            names = tuple(names)
            if not all(isinstance(n, str) for n in names):
                raise ValueError("no_decay takes parameter NAMES (an iterable of str), or None")
        slices = self.flat.slices
        unknown = [n for n in names or () if n not in slices]
        if unknown:
            raise ValueError("no_decay: %s are not parameters of the flat buffer (%s)" % (unknown, sorted(slices)))
        self.flat.set_exempt([slices[n] for n in set(names or ())])
        self._no_decay = names

    def reset_ema(self):
        """the average starts again from the parameters as they are now"""
        self.flat.reset_ema()

    def averaged_weights(self):
        """`with step.averaged_weights():` -- `flat.params` and `flat.ema` change places (sat_swap_f32, in place, no third buffer)
        and the parameters' version counters are bumped, so the weight caches keyed on `_version` see it: the model's parameters
        are views of the flat buffer, hence every decode, `validation_step` and `score_captions` inside the block runs on the
        averaged weights.  On the way out (also by an exception) they change places again.  Inside the block `optimizer_step`,
        `step`, `scst_step`, `forward_backward` and a nested entry raise RuntimeError; so does the entry when no average is kept.
        BatchNorm running statistics and the frozen stack are the live model's: they are not averaged."""
        return self.flat.averaged_weights(self)

    def averaged_state_dict(self):
        """`model.state_dict()` with the trainable entries taken from the average and everything else -- the frozen conv weights,
        every BatchNorm buffer, num_batches_tracked -- cloned from the live model: what to save as `model-best.pth`.  It loads into
        a fresh ShowAndTell, and so into a member of `sat.Ensemble`."""
        averages = self.flat.views(self.flat.averages("averaged_state_dict()"))
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        sd.update((name, t.clone()) for name, t in zip(self.flat.names, averages))
        return sd

    # -- gradient accumulation: K backwards, ONE update ------------------------------------------------------------------------
    # `flat.acc` (None until the first `accumulate()`, then a twin of `flat.grads`: the n gradients, the loss slot, the fault word;
    # 4 B per trainable parameter).  `accumulate(weight)` folds the backward that `forward_backward` / `scst_forward_backward` has
    # just left in `flat.grads` into it with one sat_grad_accumulate launch on the step's stream: acc = weight * g on the first fold
    # after an update (or after `discard_accumulated()`), acc = fma(weight, g, acc) on the later ones, and the fault words OR-ed.
    # `optimizer_step` with `accumulated > 0` then runs its usual sequence on `flat.acc` and its fault word and closes the
    # accumulation: step_count, the bias correction, the EMA and `last_grad_norm` advance once per UPDATE, and a fault or a
    # non-finite value in any micro-batch drops the one update.  With `accumulated == 0` it makes exactly the calls it makes without.
    # BatchNorm (the head's BatchNorm1d, the frozen stack's train-mode statistics) sees each micro-batch on its own, as in torch
    # gradient accumulation: accumulated micro-batches equal the big batch only where no BatchNorm lies in the path (cached 2-D
    # features).  Scheduled sampling and dropout draw per call.
    _accumulated = 0

    @property
    def accumulated(self):
        """micro-batches folded into `flat.acc` since the last update (or `discard_accumulated()`)"""
        return self._accumulated

    def accumulate(self, weight=1.0):
        """Fold the finished backward in `flat.grads` (gradients, loss slot, fault word) into `flat.acc`, times `weight` (a finite
        float, ValueError otherwise).  Nothing is read on the host.  Returns the accumulated loss slot (1-element device view)."""
        if self._averaged:
            raise RuntimeError(AVERAGED_NOTE % "accumulate()")
        weight = check_accumulate_weight(weight)
        f = self.flat
        if f.acc is None:
            f.acc = torch.zeros_like(f.grads)
        grad_accumulate(self.lib, f.acc, f.grads, f.n, weight, first=self._accumulated == 0)
        self._accumulated += 1
        return f.acc[f.loss_slot:f.loss_slot + 1]

    def discard_accumulated(self):
        """close an open accumulation without an update: the next `accumulate()` starts afresh and does not read what was folded"""
        self._accumulated = 0

    @property
    def acc_grad(self):
        """`flat.acc` (None before the first fold): what a data-parallel step all-reduces bucket by bucket"""
        return self.flat.acc

    # -- encoder look-ahead ---------------------------------------------------------------------------
    def prefetch_encoder(self, images):
        """Start the frozen conv stack of a LATER batch on a side stream (`EncoderCNN.prefetch`: up to three batches' stacks in
        flight next to each other and under this batch's decoder work; bitwise identical results)."""
        return self.model.encoder.prefetch(images)

    def _encoder_pooled(self, images, out, next_images=None):
        """pooled features [B, F] of `images` into `out` (a buffer this step owns): from the look-ahead if this tensor was
        prefetched, computed now otherwise.  `next_images`: the following batches -- their stacks are started on side streams
        (`EncoderCNN.prefetch_many`): BEFORE this batch's own stack when that still has to run (the first step of a loop: the
        look-ahead then fills the chip next to it instead of waiting for it), behind the hand-over otherwise (the instance this
        batch frees is available to them)."""
        enc = self.model.encoder
        nxt = None
        last = getattr(next_images, "last", None)      # (DevicePrefetcher.upcoming_images() says whether the data ends inside the list)
        if next_images is not None:
            nxt = list(next_images) if isinstance(next_images, (list, tuple)) else [next_images]
        hit = enc._take_prefetched(images)
        if hit is not None:
            prog, g = hit
            out.copy_(prog.pooled_of(g))
            prog.apply_running_stats(g)         # batch order = consumption order
            if nxt:
                enc.prefetch_many(nxt, last=last)
            return out
        if nxt:
            enc.prefetch_many(nxt, last=last, own_stack=True)
        out.copy_(enc._pooled_raw(images))
        return out

    def drop_lookahead(self):
        self.model.encoder.drop_lookahead()

    # -- engine interface used by DataParallelStep ----------------------------------------------------
    def forward_backward(self, batch, inv_denom, on_bucket_ready=None, next_images=None):
        """batch = (images f32[B,3,H,W], captions i64[B,T], lengths list[int] desc).  Fills the flat grad buffer
        (gradients of sum-CE * inv_denom) and the loss slot; returns the loss slot tensor (device, 1 elem).
        next_images: the FOLLOWING batch's images, or a list of the next few in order; their conv stacks are started on side
        streams under this batch's decoder work (prefetch_encoder)."""
        images, captions, lengths = batch
        lib, model, flat = self.lib, self.model, self.flat
        dec = model.decoder
        if self._averaged:
            raise RuntimeError(AVERAGED_NOTE % "a training step")
        if not model.training:
            raise RuntimeError("TrainStep needs model.train() (batch-statistics BatchNorm, train.py never calls eval())")
        dropout = dec.dropout_plan(sampling=dec.ss_prob > 0)         # host checks, before anything is launched or drawn
        L.require_gpu(captions, "captions")
        dev = images.device
        st = L.stream()
        B = images.shape[0]
        if captions.dtype != torch.int64 or captions.stride(1) != 1:
            captions = captions.long().contiguous()
        lengths = [int(l) for l in lengths]
        # sat_pack_targets reads captions[b][t+1] up to column lengths[0]-1 and the embedding gather captions[b][t-1]:
        # every caption must hold at least <start> + one target, and no length may exceed the matrix width
        if len(lengths) != B or captions.dim() != 2 or captions.shape[0] != B:
            raise ValueError("captions must be [B, T] with one length per image")
        if lengths[-1] < 2 or lengths[0] > captions.shape[1]:
            raise ValueError("need 2 <= every length <= captions.shape[1] (got min %d, max %d, width %d)"
                             % (lengths[-1], lengths[0], captions.shape[1]))
        dec.id_guard().submit(captions, lengths[0], dec.vocab_size, "captions")   # raises for a bad EARLIER batch at the latest here
        l1 = [l - 1 for l in lengths]                                        # train.py:134
        pi = PackInfo.get(l1, dev)
        N, V, E = pi.N, dec.vocab_size, dec.embed_size
        bufs = self._step_bufs(B, N, dev)
        # targets = pack(captions[:,1:], lengths-1)                           train.py:135
        L.check(lib.sat_pack_targets(captions.data_ptr(), captions.stride(0), L.ptr(pi.prefix_dev), pi.T, N,
                                     L.ptr(bufs["targets"]), st), "sat_pack_targets")
        # ---- forward (train.py:139) ----
        feats_in, pooled = self._head_forward(images, bufs, next_images)
        params = dict(dec.named_parameters())
        loss_slot = flat.grads[flat.loss_slot:flat.loss_slot + 1]
        ce = mixed_ws = None
        smoothing, alpha = self._label_smoothing, self._unlikelihood
        if alpha > 0 and pi.T > MAX_UL_STEPS:
            raise ValueError("unlikelihood supports captions of at most %d target steps (got %d)" % (MAX_UL_STEPS, pi.T))
        if (smoothing > 0 or alpha > 0) and "row_nll" not in bufs:
            bufs["row_nll"], bufs["nll"] = torch.empty(N, device=dev), torch.empty(1, device=dev)
        if alpha > 0 and "row_ul" not in bufs:
            bufs["row_ul"], bufs["ul"] = torch.empty(N, device=dev), torch.empty(1, device=dev)
        self.last_nll = bufs["nll"] if (smoothing > 0 or alpha > 0) else loss_slot
        self.last_ul = bufs["ul"] if alpha > 0 else None
        if self.decoder_gemm_dtype == "bf16":
            wsb = lib.sat_vocab_bf16_ws_bytes(N, dec.hidden_size, V)
            if wsb > 0:
                if "vocab_bf16_ws" not in bufs:
                    bufs["vocab_bf16_ws"] = torch.empty(wsb, dtype=torch.uint8, device=dev)
                ce = VocabCE(bufs["targets"], inv_denom, bufs["row_loss"], loss_slot, bufs["vocab_bf16_ws"])
                if smoothing > 0 or alpha > 0:
                    ce = ce._replace(smoothing=smoothing, row_nll=bufs["row_nll"], nll_out=bufs["nll"])
                if alpha > 0:
                    ce = ce._replace(alpha=alpha, row_ul=bufs["row_ul"], ul_out=bufs["ul"])
            # the LSTM layers' batched GEMMs on the bf16 matrix pipe too
            if "lstm_mixed_ws" not in bufs:
                need = max(lib.sat_lstm_mixed_ws_bytes(N, E if l == 0 else dec.hidden_size, dec.hidden_size) for l in range(dec.num_layers))
                bufs["lstm_mixed_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
            mixed_ws = bufs["lstm_mixed_ws"]
        ss = None
        if dec.ss_prob > 0:
            # scheduled sampling (model.training is required above): the step loop with its draws; exact-f32 logits for sat_ce_rows,
            # or in the bf16 mode draws only and the mode's projection + CE over every row (`ce`)
            ss = (dec.ss_prob, draw_ss_seed(), dec.ss_rank)
        if dropout is not None:
            dropout = dec.draw_dropout(dropout)
        logits, tapes = decoder_forward(lib, feats_in, params, captions[:, :-1], pi, self.lstm_ws, logits=bufs["logits"], ce=ce,
                                        mixed_ws=mixed_ws, ss=ss, dropout=dropout)
        # a step that dropped keeps the top layer's dropped tape [N, H] (what `linear` read) until the next step: the tests compare its
        # zero pattern with the mask of `last_dropout_seed`
        self.last_dropped_tape = tapes["X"][-1] if dropout is not None else None
        if ss is not None:
            dec.last_ss_inputs, dec.last_ss_seed = tapes["captions"], ss[1]
        if ce is None and alpha > 0:
            # ---- the same with the unlikelihood term over each row's earlier ground-truth targets, in place ----
            L.check(lib.sat_ce_rows_ul(L.ptr(logits), logits.stride(0), L.ptr(bufs["targets"]), L.ptr(pi.prefix_dev), pi.T, N, V,
                                       float(inv_denom), smoothing, alpha, L.ptr(logits), logits.stride(0), L.ptr(bufs["row_loss"]),
                                       L.ptr(bufs["row_nll"]), L.ptr(bufs["row_ul"]), L.ptr(loss_slot), L.ptr(bufs["nll"]),
                                       L.ptr(bufs["ul"]), st), "sat_ce_rows_ul")
        elif ce is None and smoothing > 0:
            # ---- smoothed loss, plain NLL + d(loss)/d(logits) in place (nn.CrossEntropyLoss(label_smoothing=)) ----
            L.check(lib.sat_ce_rows_ls(L.ptr(logits), logits.stride(0), L.ptr(bufs["targets"]), N, V, float(inv_denom), smoothing,
                                       L.ptr(logits), logits.stride(0), L.ptr(bufs["row_loss"]), L.ptr(bufs["row_nll"]),
                                       L.ptr(loss_slot), L.ptr(bufs["nll"]), st), "sat_ce_rows_ls")
        elif ce is None:
            # ---- loss + d(loss)/d(logits) in place (train.py:143) ----
            L.check(lib.sat_ce_rows(L.ptr(logits), logits.stride(0), L.ptr(bufs["targets"]), N, V, float(inv_denom), 1,
                                    L.ptr(bufs["row_loss"]), L.ptr(loss_slot), st), "sat_ce_rows")
        # ---- backward (train.py:144): gradients land directly in the flat buffer ----
        g = {name: flat.grad("decoder." + name) for name in params}
        g["features"] = bufs["d_feat"]
        decoder_backward(lib, logits, tapes, params, pi, g, self.lstm_ws, on_stage=on_bucket_ready, ce=ce, mixed_ws=mixed_ws)
        self._head_backward(bufs, pooled, feats_in)
        if on_bucket_ready is not None:
            on_bucket_ready(2)   # encoder head + embedding gradients (and the loss slot) are final
        return loss_slot

    def _step_bufs(self, B, N, dev, R=None):
        """the buffers a step of B images, R decoder rows (None: B) and N packed rows owns (one set is kept: another (B, N, R)
        replaces it).  R != B, S sampled captions per image: the set also holds the features repeated to R rows and their
        gradient, feat_rows and d_feat_rows [R, E]"""
        R = B if R is None else R
        bufs = self._bufs.get((B, N, R))
        if bufs is None:
            self._bufs.clear()
            enc, dec = self.model.encoder, self.model.decoder
            E, V, F = dec.embed_size, dec.vocab_size, enc.resnet.feature_dim
            wsb = self.lib.sat_fc_bn1d_ws_bytes(B, F, E)
            bufs = self._bufs[(B, N, R)] = dict(
                targets=torch.empty(N, dtype=torch.int64, device=dev), logits=L.logits_buffer(N, V, dev),
                row_loss=torch.empty(N, device=dev), feats=torch.empty(B, E, device=dev),
                xhat=torch.empty(B, E, device=dev), rstd=torch.empty(E, device=dev),
                head_ws=torch.empty(max(wsb // 4, B * E), device=dev), d_feat=torch.empty(B, E, device=dev),
                pooled=torch.empty(B, F, device=dev))
            if R != B:
                bufs["feat_rows"], bufs["d_feat_rows"] = torch.empty(R, E, device=dev), torch.empty(R, E, device=dev)
        return bufs

    def _head_forward(self, images, bufs, next_images):
        """(features [B, E], pooled): the frozen stack (from the look-ahead when prefetched) and fc + BatchNorm1d; `images` [B, E]
        are precomputed encoder features (decoder-only training): passed through, pooled None"""
        if images.dim() == 2:
            return images.contiguous(), None
        enc = self.model.encoder
        fc, bn = enc.resnet.fc, enc.bn
        pooled = self._encoder_pooled(images, bufs["pooled"], next_images)
        fc_bn1d_forward(self.lib, pooled, fc.weight, fc.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, True,
                        bufs["feats"], bufs["xhat"], bufs["rstd"], bufs["head_ws"])
        L.counter_add(bn.num_batches_tracked)
        return bufs["feats"], pooled

    def _head_backward(self, bufs, pooled, feats_in):
        """the head's backward from bufs["d_feat"] into the flat buffer (not with cached features), then the step's fault flag"""
        lib, flat = self.lib, self.flat
        if pooled is not None:
            fc_bn1d_backward(lib, bufs["d_feat"], pooled, bufs["xhat"], bufs["rstd"], self.model.encoder.bn.weight,
                             flat.grad("encoder.resnet.fc.weight"), flat.grad("encoder.resnet.fc.bias"),
                             flat.grad("encoder.bn.weight"), flat.grad("encoder.bn.bias"), bufs["head_ws"])
        self.last_d_features = bufs["d_feat"]
        # this step's encoder outputs (views of step-owned buffers, overwritten by the next step): the parity tests at the
        # benchmarked configuration read them
        self.last_pooled, self.last_features = pooled, feats_in
        # the step's fault flag (one 1-thread launch): OR of the status words of this step's persistent LSTM launches and of the
        # engine's sticky word, into slot 1 of the trailing floats -- it rides the last bucket's all-reduce, and clamp + Adam
        # read it on the device (optimizer_step): a step that any rank lost never reaches the parameters of any rank
        words, nw = self.lstm_ws.fault_words
        L.check(lib.sat_step_fault_flag(words, nw, L.ptr(self._fault_sticky), L.ptr(self.fault_slot), L.stream()), "sat_step_fault_flag")

    def scst_forward_backward(self, images, image_index, scorer, end_id=2, steps=20, next_images=None, num_samples=1,
                              baseline="greedy"):
        """`forward_backward` for the self-critical loss (`scst.SelfCritical`, Rennie et al. 2017): same look-ahead, cached [B, E]
        features accepted, gradients straight into the flat buffer, loss into the loss slot, fault flag.  The decoder part is the
        sampled rollout (`sat_rollout_decoder_fwd`), the greedy decode as baseline, CIDEr of both on the device, `sat_scst_weights`
        + `sat_ce_rows_weighted` in place on the step's logits, and the teacher-forced backward on the tokens drawn.  The decoder
        arithmetic of this step is EXACT F32 whatever `decoder_gemm_dtype` says: the draws are taken from exact-f32 logits and
        the backward runs on them (the bf16 decoder GEMMs are not wired into this step).  Rewards, baseline and ids of the step
        are kept on `last_scst`.
        num_samples = S > 1, baseline "greedy" / "sample_mean": `SelfCritical`'s.  The head runs on the B images once; its [B, E]
        features are repeated to R = B * S rows, the decoder buffers hold R rows and R * steps packed rows, the weights come from
        `sat_scst_weights_group`, and the decoder's d_feat [R, E] is summed per image (`sat_group_sum_rows`) in front of the head's
        backward.  With the defaults the calls are those made without the keywords."""
        S, baseline = check_group(num_samples, baseline)             # host checks, before anything is launched
        lib, model, flat = self.lib, self.model, self.flat
        dec = model.decoder
        if self._averaged:
            raise RuntimeError(AVERAGED_NOTE % "a training step")
        if not model.training:
            raise RuntimeError("TrainStep needs model.train() (batch-statistics BatchNorm, train.py never calls eval())")
        dec.dropout_plan(sampling=True, what="a rollout (scst_step)")
        dev = images.device
        B, steps = images.shape[0], int(steps)
        R = B * S
        bufs = self._step_bufs(B, R * steps, dev, R)
        feats_in, pooled = self._head_forward(images, bufs, next_images)
        params = dict(dec.named_parameters())
        loss_slot = flat.grads[flat.loss_slot:flat.loss_slot + 1]
        seed = draw_ss_seed()
        rows_in = feats_in
        if S > 1:
            rows_in = bufs["feat_rows"]                              # row b * S + s = the features of image b (data movement)
            rows_in.view(B, S, -1).copy_(feats_in.unsqueeze(1).expand(B, S, -1))
        ids, logits, tapes, pi = rollout_forward(lib, rows_in, params, steps, seed, dec.ss_rank, self.lstm_ws, logits=bufs["logits"])
        dec.last_rollout_seed = seed
        sc = self.last_scst = SelfCritical(scorer, end_id, num_samples=S, baseline=baseline)
        if S == 1:
            sc.last_reward, sc.last_baseline, sc.last_greedy_ids = sc.rewards(dec, feats_in, ids, image_index)
            sc.last_ids = ids
            w, _, _ = scst_weights(ids, sc.last_reward, sc.last_baseline, end_id)
        else:
            sc.last_ids = ids.view(B, S, steps)
            sc.last_reward, base, sc.last_greedy_ids = sc.rewards(dec, feats_in, sc.last_ids, image_index)
            w, _, _, sc._advantage, sc.last_baseline = scst_weights_group(sc.last_ids, sc.last_reward, base, end_id)
        ce_rows_weighted(logits[:, :dec.vocab_size], ids, w, write_grad=True, loss_out=loss_slot)
        g = {name: flat.grad("decoder." + name) for name in params}
        g["features"] = bufs["d_feat"] if S == 1 else bufs["d_feat_rows"]
        decoder_backward(lib, logits, tapes, params, pi, g, self.lstm_ws)
        if S > 1:
            group_sum_rows(bufs["d_feat_rows"], S, out=bufs["d_feat"])
        self._head_backward(bufs, pooled, feats_in)
        return loss_slot

    def check_ids(self):
        """Block until the device-side verdicts of the last submitted batch are known: raises IndexError on a bad caption id,
        RuntimeError when a persistent LSTM recurrence gave up (`watch.ResidencyWatch`; see `optimizer_step`)."""
        self.model.decoder.id_guard().poll(block=True)
        self._retire_fixed_lag(0)          # data-parallel steps: every flag still in flight, oldest first (same order on every rank)
        ResidencyWatch.get(self.model.decoder.linear.weight.device).poll(block=True)

    FAULT_NOTE = ("the parameter update of that step and of every step submitted since was SKIPPED on the device (on every rank in "
                  "data-parallel training, where every rank raises this at the same step): parameters and Adam moments are exactly "
                  "those before the faulted step and the step count has been rolled back; repeat the batches.  What is NOT rolled "
                  "back: the BatchNorm running statistics and num_batches_tracked (the frozen stack's and the head's) have seen the "
                  "dropped batches once already")

    # data-parallel steps look at step k - DP_FAULT_LAG's (all-reduced, hence rank-identical) fault flag right after submitting step
    # k, BLOCKING: every rank then raises at the same step, with the same steps dropped.  A lag of 2 keeps the host up
    # to two steps ahead of the device, which is all the look-ahead needs.
    DP_FAULT_LAG = 2

    def _on_fault(self, step_before):
        """host side of a raised fault: per-step launches from now on, step count back to where the first dropped update found
        it (the updates in between were dropped on the device), sticky word cleared so that updates resume"""
        self.lib.sat_lstm_persist_enable(0)
        self.step_count = step_before
        self._fault_sticky.zero_()

    def _watch_fixed_lag(self, before, lag, fault_slot=None):
        """The host half of the fault path for DATA-PARALLEL steps.  The device half is rank-consistent by construction (the flag
        rides the all-reduce); the host half must be too: with the non-blocking poll of the single-rank path, ranks could see
        the flag one step apart, the early one would clear its sticky word, and the late one's next update -- no longer dropped --
        would mix a retried batch with a later one while both rolled their step counts back.  Here every rank copies
        the step's REDUCED flag to pinned memory and, after submitting step k, waits for the copy of step k - lag: same flag, same
        point in the loop, same decision on every rank.  While the faulted rank's sticky word is set, every rank's reduced flag is
        non-zero, so the steps between the fault and the raise are dropped everywhere; the raise rolls the step count back to the
        faulted step's on every rank and clears the sticky word."""
        self._lag_ring.push((self.fault_slot if fault_slot is None else fault_slot).view(torch.int32), before)
        self._retire_fixed_lag(lag)

    def _retire_fixed_lag(self, keep):
        fault = self._lag_ring.retire(block=True, keep=keep)
        if fault is not None:
            code, before = fault
            torch.cuda.synchronize()
            self._on_fault(before)
            raise RuntimeError("show-and-tell_amd: a persistent LSTM recurrence of a training step timed out waiting for its "
                               "workgroups to be resident together (reduced fault flag 0x%x: on this rank or another); %s.  "
                               "Later calls use the form without a device-wide wait" % (code & 0xffffffff, self.FAULT_NOTE))

    def optimizer_step(self, lr=None, fixed_lag=None):
        """clip_gradient + Adam (train.py:145-146) as one launch over the flat buffers, GUARDED on the device by the step's
        fault flag: when a persistent LSTM launch of this step (any rank's, after the all-reduce) gave up waiting for its
        workgroups, the launch drops the whole update -- the garbage gradients never reach parameters or moments -- and so does
        every later one until the host has seen the flag (sticky), raised RuntimeError (at the latest on the next submit;
        `check_ids()` at once) and rolled the step count back.  fixed_lag (data-parallel steps): look at the flag of the step
        submitted `fixed_lag` steps ago, blocking, instead of polling (`_watch_fixed_lag`)."""
        f = self.flat
        if f.averaged:
            raise RuntimeError(AVERAGED_NOTE % "optimizer_step()")
        before = f.step_count
        # an open accumulation: the same sequence on `flat.acc` and ITS fault word (the OR over the micro-batches), closed here
        grads, fault_slot = f.grads, self.fault_slot
        if self._accumulated > 0:
            grads, fault_slot = f.acc, f.acc[f.loss_slot + 1:f.loss_slot + 2]
            self._accumulated = 0
        f.update(grads, None, fault_slot, lr)       # (no update kernel writes the fault word: it lies past the n elements they cover)
        if fixed_lag is not None:
            self._watch_fixed_lag(before, int(fixed_lag), fault_slot)
            return
        ResidencyWatch.get(f.params.device).submit(fault_slot.view(torch.int32), "a persistent LSTM recurrence of a training step",
                                                   lambda: self._on_fault(before), note=self.FAULT_NOTE)

    # -- optimizer checkpoint interchange (the reference's load_optimizer is an empty stub, ------
    #    train.py:60-64, and only model.state_dict() is saved, train.py:191-193) ---------------------------
    def _trainable(self):
        """(name, param) in the order train.py:55 hands them to optim.Adam: model.parameters() with requires_grad"""
        return list(zip(self.flat.names, self.flat.tensors))

    def optimizer_state_dict(self):
        """The flat Adam state in `torch.optim.Adam.state_dict()` layout (loads into a torch Adam built over
        `filter(requires_grad, model.parameters())` and back), with "param_names" and 0.0 for no "max_grad_norm"."""
        sd = self.flat.state_dict(self.flat.names)
        sd["max_grad_norm"] = self.max_grad_norm
        return sd

    def load_optimizer_state_dict(self, sd):
        self.flat.load_state_dict(sd, self.flat.names)

    # -- single-GPU convenience ----------------------------------------------------------------------
    def step(self, images, captions, lengths, lr=None, next_images=None):
        """One whole iteration; returns the mean-CE loss as a 1-element device tensor (no host sync).  next_images (the
        following batch's images, optional) starts that batch's frozen conv stack under this one's decoder work."""
        n_tokens = sum(int(l) - 1 for l in lengths)
        loss = self.forward_backward((images, captions, lengths), 1.0 / n_tokens, next_images=next_images).clone()
        self.optimizer_step(lr)
        return loss

    def scst_step(self, images, image_index, scorer, lr=None, next_images=None, end_id=2, steps=20, num_samples=1,
                  baseline="greedy"):
        """One whole self-critical iteration (`scst_forward_backward` + `optimizer_step`); returns the loss as a 1-element device
        tensor (no host sync).  The decoder arithmetic of this step is exact f32 whatever `decoder_gemm_dtype` is.  num_samples,
        baseline: S sampled captions per image and the baseline they are judged against (`scst_forward_backward`)."""
        loss = self.scst_forward_backward(images, image_index, scorer, end_id, steps, next_images, num_samples, baseline).clone()
        self.optimizer_step(lr)
        return loss

    def step_accumulated(self, batches, lr=None, next_images=None):
        """One update from K micro-batches: `batches` is a sequence of (images, captions, lengths).  Every micro-batch runs
        `forward_backward` with inv_denom = 1 / (target tokens of ALL micro-batches) and is folded with weight 1, so the update
        is that of the mean CE over the union -- the rule `DataParallelStep` applies across ranks -- with gradients summed in f32
        in call order.  Returns the accumulated loss as a 1-element device tensor (no host sync).  Look-ahead: micro-batch k
        hands micro-batch k + 1's images on as `next_images`, the last one the caller's.  `last_nll` / `last_ul` are the sums of
        the micro-batches' values in fresh 1-element tensors.  BatchNorm sees each micro-batch on its own (see `accumulate`)."""
        batches = list(batches)
        if not batches:
            raise ValueError("step_accumulated needs at least one micro-batch")
        if self._accumulated:
            raise RuntimeError("step_accumulated: an accumulation is open (%d folded): optimizer_step() or discard_accumulated() "
                               "first" % self._accumulated)
        inv_denom = 1.0 / sum(int(l) - 1 for _, _, lengths in batches for l in lengths)
        nll = ul = None
        try:
            for k, batch in enumerate(batches):
                nxt = batches[k + 1][0] if k + 1 < len(batches) else next_images
                self.forward_backward(tuple(batch), inv_denom, next_images=nxt)
                self.accumulate()
                nll = self.last_nll.clone() if nll is None else nll + self.last_nll
                if self.last_ul is not None:
                    ul = self.last_ul.clone() if ul is None else ul + self.last_ul
        except BaseException:
            self.discard_accumulated()
            raise
        self.last_nll, self.last_ul = nll, ul
        loss = self.flat.acc[self.flat.loss_slot:self.flat.loss_slot + 1].clone()
        self.optimizer_step(lr)
        return loss

    def mixed_step(self, images, captions, lengths, image_index, scorer, rl_weight, lr=None, next_images=None, **scst):
        """One update of (1 - rl_weight) * XE + rl_weight * SCST (Paulus et al. 2017): a teacher-forced `forward_backward` folded
        with weight 1 - rl_weight, a `scst_forward_backward` (keywords end_id, steps, num_samples, baseline in `scst`) folded with
        weight rl_weight, one `optimizer_step`: one bias-correction step and one EMA update, where alternating `step` and
        `scst_step` takes two.  rl_weight lies in [0, 1] (ValueError); at exactly 0 or 1 the call IS `step` / `scst_step`: no
        accumulate launch, the same bits.  Returns the mixed loss (1-element device tensor, no host sync); `last_scst` is what
        `scst_step` leaves, `last_nll` / `last_ul` what the XE half leaves (unweighted).  BOTH halves run the encoder head on
        `images`: the frozen stack (unless cached [B, E] features are handed in) runs twice and the BatchNorm running statistics
        are updated once by each half.  `next_images` goes to the second half."""
        if isinstance(rl_weight, bool) or not isinstance(rl_weight, (int, float)) or not 0.0 <= rl_weight <= 1.0:
            raise ValueError("rl_weight must be a number in [0, 1] (got %r)" % (rl_weight,))
        unknown = sorted(set(scst) - {"end_id", "steps", "num_samples", "baseline"})
        if unknown:
            raise TypeError("mixed_step: unexpected keywords %s" % unknown)
        if rl_weight == 0:
            return self.step(images, captions, lengths, lr, next_images)
        if rl_weight == 1:
            return self.scst_step(images, image_index, scorer, lr, next_images, **scst)
        if self._accumulated:
            raise RuntimeError("mixed_step: an accumulation is open (%d folded): optimizer_step() or discard_accumulated() first"
                               % self._accumulated)
        try:
            n_tokens = sum(int(l) - 1 for l in lengths)
            self.forward_backward((images, captions, lengths), 1.0 / n_tokens)
            self.accumulate(1.0 - float(rl_weight))
            nll, ul = self.last_nll.clone(), None if self.last_ul is None else self.last_ul.clone()
            self.scst_forward_backward(images, image_index, scorer, next_images=next_images, **scst)
            self.accumulate(float(rl_weight))
        except BaseException:
            self.discard_accumulated()
            raise
        self.last_nll, self.last_ul = nll, ul
        loss = self.flat.acc[self.flat.loss_slot:self.flat.loss_slot + 1].clone()
        self.optimizer_step(lr)
        return loss


def dp_shard(images, captions, lengths, rank, world):
    """Interleaved shard of a length-sorted global batch: rank r takes rows r, r+world, ...  Every shard stays
    sorted by decreasing length (pack_padded_sequence's requirement) and shards are balanced in tokens.
    Returns (images_r, captions_r, lengths_r, global_tokens) with global_tokens = sum(lengths-1) over ALL rows."""
    idx = list(range(rank, len(lengths), world))
    sel = torch.as_tensor(idx, device=captions.device)
    return (images.index_select(0, sel.to(images.device)), captions.index_select(0, sel), [lengths[i] for i in idx],
            sum(int(l) - 1 for l in lengths))


def decode_shard(n, rank, world):
    """Decode (eval.py:93-99 `model.sample`) shards by image with no exchange step: rank r owns the contiguous rows
    [lo, hi) of an n-image batch (the first n % world ranks take one row more)."""
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def gather_decoded(ids_local, n, process_group=None):
    """Collect every rank's decoded ids (i64 [rows_r, ...]) into the full [n, ...] tensor on every rank -- only the
    result collection for the host-side id->word loop (eval.py:99-118), not part of the decode itself."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(process_group) == 1:
        return ids_local
    world = dist.get_world_size(process_group)
    rows = max(decode_shard(n, r, world)[1] - decode_shard(n, r, world)[0] for r in range(world))
    pad = ids_local.new_zeros((rows,) + tuple(ids_local.shape[1:]))
    pad[:ids_local.shape[0]] = ids_local
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=process_group)
    return torch.cat([parts[r][:decode_shard(n, r, world)[1] - decode_shard(n, r, world)[0]] for r in range(world)], 0)


class DataParallelStep:
    """One process per GPU; replaces `nn.DataParallel` (train.py:43-44).  Semantics:
      * the minibatch is sharded along dim 0, parameters replicated, forward/backward rank-local;
      * gradients are those of the GLOBAL mean CE: every rank scales by 1/(global token count), then one
        all-reduce(sum) per bucket over RCCL/xGMI, launched as soon as the bucket is final and overlapped with
        the remaining backward kernels; the loss rides in the last bucket;
      * clamp + Adam run AFTER the reduction (train.py:144-146 order), identically on every rank;
      * BatchNorm uses per-rank batch statistics (what nn.DataParallel replicas do as well).
    `engine` needs: .flat_grad, .buckets, .forward_backward(batch, inv_denom, on_bucket_ready), .optimizer_step(lr); for
    `step_accumulated` also .accumulate(weight) (folds the finished backward in .flat_grad into .acc_grad), .acc_grad (the
    accumulated twin of .flat_grad, same buckets) and .accumulated (folds since the last update), and an .optimizer_step that
    updates from .acc_grad while an accumulation is open.
    """

    def __init__(self, engine, process_group=None):
        import torch.distributed as dist
        self.dist = dist
        self.engine = engine
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        dec = getattr(getattr(engine, "model", None), "decoder", None)
        if dec is not None and hasattr(dec, "ss_rank"):       # scheduled sampling: every rank draws from a stream of its own
            dec.ss_rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        # The bucket all-reduces overlap the rest of the backward: c10d `async_op=True` as each bucket's gradients become final,
        # `wait()` before clamp + Adam.  (Measured on ONE rank, where RCCL launches no kernel -- bench.py --force-dist, round 3: any
        # DEFERRED wait costs 0.4-0.5 ms of a 4.5 ms step, whatever the form -- a communication stream of our own, one bucket or
        # three -- while waiting at once would expose the whole exchange with N > 1; those variants were removed in round 4.)
        if self.world > 1:
            self.cap_lookahead()

    LOOKAHEAD_STREAMS_DP = 2

    def cap_lookahead(self):
        """With collectives in the step, RCCL's stream is one more concurrently active hardware queue: main + three look-ahead streams +
        RCCL = five, and the fifth costs 0.45-0.55 ms per step (bench.py --force-dist on one rank, end of round 3: 14.0-14.2 k img/s with
        three stacks on three streams against 15.9 k without collectives).  So the data-parallel step spreads the (still three)
        stacks in flight over TWO side streams -- the third queues behind the first on its hardware queue and starts the moment that
        one ends: 15.05-15.1 k img/s (depth 2 on two streams: 14.85 k; tools/run_gpu_dist_ab.sh).  SAT_LOOKAHEAD_STREAMS overrides."""
        enc = getattr(getattr(self.engine, "model", None), "encoder", None)
        if enc is not None and hasattr(enc, "lookahead_depth") and not _os.environ.get("SAT_LOOKAHEAD_STREAMS"):
            enc.lookahead_streams = min(enc.lookahead_depth, self.LOOKAHEAD_STREAMS_DP)

    def step(self, batch, global_tokens, lr=None, next_images=None):
        eng, dist = self.engine, self.dist
        works = []

        def ready(i):
            if self.world > 1:
                s_, e_ = eng.buckets[i]
                works.append(dist.all_reduce(eng.flat_grad[s_:e_], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

        if next_images is not None:
            loss = eng.forward_backward(batch, 1.0 / float(global_tokens), ready, next_images=next_images)
        else:
            loss = eng.forward_backward(batch, 1.0 / float(global_tokens), ready)
        for w in works:
            w.wait()                 # every bucket is reduced before clamp + Adam read the gradients
        loss = loss.clone()          # the slot in the flat gradient buffer is overwritten by the next step
        if self.world > 1 and hasattr(eng, "DP_FAULT_LAG"):
            eng.optimizer_step(lr, fixed_lag=eng.DP_FAULT_LAG)     # rank-consistent fault handling (TrainStep._watch_fixed_lag)
        else:
            eng.optimizer_step(lr)
        return loss

    def step_accumulated(self, batches, global_tokens, lr=None, next_images=None):
        """One update from K micro-batches per rank with ONE gradient exchange (torch DDP's `no_sync` for the first K - 1):
        every micro-batch runs `forward_backward` with 1 / global_tokens -- the target tokens of all micro-batches on ALL ranks --
        without bucket callbacks and is folded into `engine.acc_grad`; after the last fold each bucket of `acc_grad` is
        all-reduced once (async, waited for before the update; loss and fault word ride in the last bucket) and the update runs
        on it.  The exchange starts behind the last fold: it is not overlapped with the last backward.  Returns the global loss."""
        eng, dist = self.engine, self.dist
        batches = list(batches)
        if not batches:
            raise ValueError("step_accumulated needs at least one micro-batch")
        if eng.accumulated:
            raise RuntimeError("step_accumulated: an accumulation is open on the engine (%d folded)" % eng.accumulated)
        inv_denom = 1.0 / float(global_tokens)
        lookahead = hasattr(eng, "prefetch_encoder")       # (an engine without one is not handed the keyword, as in `step`)
        for k, batch in enumerate(batches):
            nxt = next_images if k + 1 == len(batches) else (batches[k + 1][0] if lookahead else None)
            if nxt is not None:
                eng.forward_backward(batch, inv_denom, next_images=nxt)
            else:
                eng.forward_backward(batch, inv_denom)
            eng.accumulate(1.0)
        acc = eng.acc_grad
        works = []
        if self.world > 1:
            for s_, e_ in eng.buckets:
                works.append(dist.all_reduce(acc[s_:e_], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        for w in works:
            w.wait()                 # every bucket is reduced before clamp + Adam read the accumulated gradients
        end = eng.buckets[-1][1]     # the 4 trailing floats of the last bucket: loss, fault word, padding
        loss = acc[end - 4:end - 3].clone()
        if self.world > 1 and hasattr(eng, "DP_FAULT_LAG"):
            eng.optimizer_step(lr, fixed_lag=eng.DP_FAULT_LAG)
        else:
            eng.optimizer_step(lr)
        return loss
