"""What every conv stack's op program shares: the builder state and the op emitters a stack's topology is written with, and
running, hipGraph replay, kernel selection and the deferred running statistics of the finished `sat_op` array.

A stack subclasses `OpProgram`, emits its layers into `self.ops` (image prep first: `run` points ops[0 .. groups) at the
caller's images) and calls `_finish`.  BatchNorm statistics go through ONE emitter, `bn_stats`, which picks their form and
returns a `BnSource` that the consuming op attaches as its BatchNorm operand."""
import ctypes as C
import os

import torch

from . import _lib as L
from . import tune as T

BN_MOMENTUM = 0.1

# BatchNorm statistics as integer atomics straight from the conv epilogue up to this many 128-row tiles; beyond (the stem,
# layer 1) the conv writes per-tile slabs and a wide reducer launch folds them into the same accumulators
ATOMIC_MAX_TILES = 128      # (measured again with the round-4 kernels: 400 / 1600 slow the convs by 2 / 6 % for the 21 / 37 reducer launches they save)

_PROGRAM_PICKS = {}      # tune key -> variant chosen in a program of this process (OpProgram._pick_in_program)


def tdtype(dtype):
    return torch.bfloat16 if dtype == L.SAT_BF16 else torch.float32


def conv_op(dtype, x, w, out, n, hin, win, cin, hout, wout, cout, kh, kw, stride, pad, **fields):
    """implicit-GEMM conv over a dense NHWC input [n][hin][win][cin] (`sN` / `sH` / `sW` in `fields` override its strides)"""
    f = dict(sN=hin * win * cin, sH=win * cin, sW=cin)
    f.update(fields)
    return L.op(L.OP_CONV, dtype, in0=x, w=w, out=out, N=n, Hin=hin, Win=win, Cin=cin, Hout=hout, Wout=wout, Cout=cout,
                KH=kh, KW=kw, stride=stride, pad=pad, **f)


def act_op(kind, dtype, x, out, n, h, w, c, **fields):
    """an elementwise normalise (+ add) + ReLU pass over [n][h][w][c]; its BatchNorm operands come from `BnSource.attach`"""
    return L.op(kind, dtype, in0=x, out=out, N=n, Hout=h, Wout=w, Cout=c, **fields)


def image_prep(dtype, img, n, h, w, pad, groups=1, cout=0):
    """one image-prep op per batch of n f32 NCHW images [n,3,h,w], each into its slice of the zero-bordered NHWC buffer `img`"""
    return [L.op(L.OP_IMAGE_PREP, dtype, out=img[g * n:], N=n, Hin=h, Win=w, Hout=img.shape[1], Wout=img.shape[2], pad=pad,
                 Cout=cout) for g in range(groups)]


def avgpool(dtype, x, pooled, h, w):
    """global average pool of NHWC [images][h][w][C] into f32 pooled [images][C]"""
    return L.op(L.OP_AVGPOOL, dtype, in0=x, out=pooled, N=pooled.shape[0], Hin=h, Win=w, Cout=pooled.shape[1])


class BnSource:
    """Where a consumer finds one BatchNorm: a (scale, shift) table (`scale`, `shift` pointers), or the integer batch sums of
    the producing conv (`acc`: stat_acc[group][parity][2][C]), from which the consumer derives (scale, shift) itself -- no
    finalize launch; the parity alternates per run so workgroup 0 of the consumer can clear the other half for the next step."""

    def __init__(self, bn, count, eps, acc=None, scale=None, shift=None):
        self.bn, self.count, self.eps, self.acc, self.scale, self.shift = bn, count, eps, acc, scale, shift

    def attach(self, o, slot=0):
        """make this BatchNorm operand `slot` (0 or 1) of a BN_RELU / BN_ADD_RELU / BN_RELU_MAXPOOL op"""
        if self.acc is None:
            setattr(o, "scale%d" % slot, self.scale)
            setattr(o, "shift%d" % slot, self.shift)
            return o
        sfx = "1" if slot else ""
        bn = self.bn
        for name, v in (("stat_acc", self.acc), ("gamma", bn.weight), ("beta", bn.bias), ("running_mean", bn.running_mean),
                        ("running_var", bn.running_var)):
            setattr(o, name + sfx, v if name == "stat_acc" else v.data_ptr())
        o.count, o.momentum, o.eps = self.count, BN_MOMENTUM, self.eps
        return o

    def conv_input(self, cv):
        """the conv reads the RAW output of this BatchNorm's producer and applies BatchNorm + ReLU to its staged operand: a
        table is its operand-0 affine, integer sums take the second statistics slot (the first holds the conv's own)"""
        return self.attach(cv, 1 if self.acc is not None else 0)


class OpProgram:
    """Device buffers + sat_op array of one conv stack for one (batch, H, W, dtype, training) configuration.

    groups = G > 1 (bf16, training): the program runs G independent batches in every launch (`sat_op.groups`, grid.y =
    group): activations are [G][N]..., every BatchNorm keeps per-group batch statistics, weights are shared.  Each group is,
    instruction for instruction, the ungrouped program on its batch as long as both run kernel variants of the same statistics
    signature: the first program built for a model state tunes freely, every other one gets its `signatures()` as a constraint
    (`signatures=`; `EncoderCNN._program` builds the grouped one first), so a batch's pooled features and BatchNorm statistics
    are bit-identical whichever program runs it.  Grouped programs always run with deferred running statistics
    (`defer_running_stats`), one update per consumed batch.  groups > 1 in eval mode: BatchNorm is a fixed affine there, so the
    batches of a group simply concatenate into one program over groups * N images (no `sat_op.groups`): `self.n` images per
    launch and group, `self.G` groups per launch.  Subclasses set BN_EPS and emit the stack's topology."""

    def __init__(self, stack, N, H, W, dtype, training, device, groups=1, signatures=None):
        self.stack, self.N, self.H, self.W, self.dtype, self.training, self.groups = stack, N, H, W, dtype, training, int(groups)
        if self.groups > 1 and dtype != L.SAT_BF16:
            raise ValueError("grouped programs are for the bf16 stack")
        self.n, self.G = (self.groups * N, 1) if (self.groups > 1 and not training) else (N, self.groups)
        self.device, self.td, self.lib = device, tdtype(dtype), L.load()
        # statistics signatures (sat_conv_variant_signature) per conv geometry that the tuner has to stay within: those of the
        # FIRST program built for this model state (`signatures()`), so that every program gives a batch the same bits
        self._want_sigs = dict(signatures or {})
        self.keep = []            # tensors the op array points into
        self.ops = []             # the program, a list until `_finish`
        self.stat_accs = []       # integer BatchNorm sums, [G][2 parities][2][C] each
        self._n_prep = self.groups
        self._slab_users, self._slab_floats, self.partial = [], 0, None
        # one flat int64 counter tensor behind every bn.num_batches_tracked: one increment per forward
        bns = list(stack.bns())
        flat = getattr(stack, "_nbt_flat", None)
        if flat is None or flat.device != torch.device(device) or \
                any(bn.num_batches_tracked.data_ptr() != flat[i].data_ptr() for i, bn in enumerate(bns)):
            flat = torch.stack([bn.num_batches_tracked.detach().to(device) for bn in bns])
            for i, bn in enumerate(bns):
                bn.num_batches_tracked = flat[i]
            object.__setattr__(stack, "_nbt_flat", flat)

    def alloc(self, shape, dt=None, zero=False):
        t = (torch.zeros if zero else torch.empty)(shape, dtype=self.td if dt is None else dt, device=self.device)
        self.keep.append(t)
        return t

    # ---- BatchNorm statistics ----
    def _slabs(self, o, tiles, c):
        """`o` writes / reads per-tile column-sum slabs of `tiles` row tiles x C in the shared partial buffer"""
        o.tiles_m = tiles
        self._slab_users.append(o)
        self._slab_floats = max(self._slab_floats, self.G * tiles * 2 * c)

    def _bn_table(self, c):
        """storage of one BatchNorm's (scale, shift) table"""
        return self.alloc((c,), torch.float32), self.alloc((c,), torch.float32)

    def _eval_bn(self, bn, c, count):
        """eval mode: the BatchNorm as a fixed affine from its running statistics (the stacks differ here)"""
        raise NotImplementedError

    def _bn_finalize(self, bn, c, count, tiles, training):
        """OP_BN_FINALIZE into a fresh (scale, shift) table: from the slabs of the conv in front (training) or from the running
        statistics (training=0)"""
        s, t = self._bn_table(c)
        f = L.op(L.OP_BN_FINALIZE, self.dtype, gamma=bn.weight, beta=bn.bias, running_mean=bn.running_mean,
                 running_var=bn.running_var, scale_out=s, shift_out=t, Cout=c, count=count, tiles_m=tiles, training=training,
                 momentum=BN_MOMENTUM, eps=self.BN_EPS)
        self.ops.append(f)
        return f, BnSource(bn, count, self.BN_EPS, scale=s.data_ptr(), shift=t.data_ptr())

    def bn_stats(self, cv, bn):
        """The statistics of BatchNorm `bn` over the output of conv op `cv` (the last op emitted), in the form this program runs;
        returns the `BnSource` its consumers attach.
          * bf16 training, <= ATOMIC_MAX_TILES row tiles: fixed-point integer atomics straight from the conv epilogue;
          * bf16 training, more tiles: the conv keeps writing per-tile slabs (no contended atomics) and a wide reducer launch
            folds them into the same integer accumulators;
          * f32 training: per-tile slabs + a finalize launch (f64) into a (scale, shift) table;
          * eval: the stack's fixed affine (`_eval_bn`).
        All forms are bitwise reproducible."""
        c, count = cv.Cout, cv.N * cv.Hout * cv.Wout
        tiles = self.lib.sat_conv_tiles_m(count)
        if not self.training:
            return self._eval_bn(bn, c, count)
        if self.dtype != L.SAT_BF16:
            f, src = self._bn_finalize(bn, c, count, tiles, 1)
            self._slabs(cv, tiles, c)
            self._slabs(f, tiles, c)
            return src
        acc = self.alloc((self.G, 2, 2, c), torch.int64, zero=True)
        self.stat_accs.append(acc)
        if tiles <= ATOMIC_MAX_TILES:
            cv.stat_acc = acc.data_ptr()
        else:
            f = L.op(L.OP_BN_FINALIZE, self.dtype, groups=self.G, stat_acc=acc, Cout=c, training=1)
            self._slabs(cv, tiles, c)
            self._slabs(f, tiles, c)
            self.ops.append(f)
        return BnSource(bn, count, self.BN_EPS, acc=acc.data_ptr())

    def _finish(self, tune_buffers=()):
        """the op array, the shared slab buffer, replay / deferral state and the kernel selection of a built program"""
        if self._slab_users:
            # every per-batch buffer of a grouped program is G consecutive copies of the ungrouped one
            self.partial = self.alloc((self._slab_floats,), torch.float32)
            for o in self._slab_users:
                o.stat_partial = self.partial.data_ptr()
        self.ops = (L.SatOp * len(self.ops))(*self.ops)
        self.n_ops = len(self.ops)
        # replay as a hipGraph (SAT_GRAPH=0: eager launches).  Per step parity: first run eager, then captured.
        self._parity = 0
        self._use_graph = os.environ.get("SAT_GRAPH", "1") != "0" and torch.device(self.device).type == "cuda"
        self._runs, self._graphs = [0, 0], [None, None]
        self._running_items = None              # defer_running_stats(): number of redirected BatchNorms
        if self.groups > 1 and self.training:
            self.defer_running_stats()
        self._autotune(tune_buffers)

    # ---- kernel selection ----
    def _autotune(self, buffers):
        """Kernel selection per conv geometry (bf16).  Default: the COMMITTED table (`tune.py`, `tune/gfx950.json`: the BASELINE
        geometries, measured once) and, for a geometry it does not name, the library's geometry-only default -- no stopwatch, so
        every process, rank and box runs the same kernels and the same seed gives the same bits (round 4: a timing-based choice
        moved the first-forward CE by 1.2e-3 between two processes).  SAT_AUTOTUNE=1 times the geometries the table does not name
        on this program's own buffers (`buffers` are re-randomised first; the tuner's three fastest per geometry, the final choice
        IN the program); SAT_TUNE_FILE=<json> saves / reloads those."""
        if self.dtype != L.SAT_BF16 or torch.device(self.device).type != "cuda":
            return
        want_of = lambda o: self._want_sigs.get(T.layer_key(o))
        missing = T.assign(self.ops, self.n_ops, want_of)
        if not missing:
            return
        if T.mode() not in ("time", "force"):
            T.defaults(self.ops, missing, want_of)
            return
        chosen = {i: int(self.ops[i].variant) for i in range(self.n_ops) if self.ops[i].kind == L.OP_CONV}
        for t in buffers:
            t.normal_()
        scratch = self.alloc((4096,), torch.float32)           # the tuner's neutral BatchNorm table lives in OUR memory
        topk = max(1, int(os.environ.get("SAT_TUNE_TOPK", "3")))
        cand = (C.c_int32 * (self.n_ops * topk))()
        L.check(self.lib.sat_conv_autotune_topk(self.ops, self.n_ops, 5, scratch.data_ptr(), scratch.numel() * 4,
                                                L.stream(), topk, cand), "sat_conv_autotune")
        torch.cuda.synchronize()
        for i, v in chosen.items():
            if v > 0:
                self.ops[i].variant = v                   # (entries the table already had stay as loaded)
        if topk > 1:
            self._pick_in_program(cand, topk, {i for i, v in chosen.items() if v > 0})
        T.save(self.ops, self.n_ops, want_of)

    def _pick_in_program(self, cand, topk, fixed):
        """The final choice among the tuner's `topk` fastest variants per conv geometry, made IN the program: a replayed launch finds
        its operand warm, the same launch in the program finds what the previous kernel just wrote (a layer-3 1x1 conv: 13 us
        replayed, 18 in the program), and the two rankings differ by a few microseconds either way.  Pass k runs the whole program
        with every geometry on its k-th candidate and takes each conv launch's own duration (`sat_run_ops_timed`); a geometry keeps
        the candidate with the smallest summed duration.  Leaves no trace: statistics accumulators, parity, running statistics are
        put back."""
        lib = self.lib
        classes = {}
        for i in range(self.n_ops):
            o = self.ops[i]
            if o.kind == L.OP_CONV and i not in fixed and cand[i * topk]:
                key = T.tune_key(o, self._want_sigs.get(T.layer_key(o)))
                if key in _PROGRAM_PICKS:             # decided earlier in this process: the same choice for every model (like the
                    o.variant = _PROGRAM_PICKS[key]   # library's own per-geometry cache), so two models of one shape agree bit for bit
                else:
                    classes.setdefault(key, []).append(i)
        lists = {key: [int(cand[ix[0] * topk + k]) for k in range(topk) if cand[ix[0] * topk + k]] for key, ix in classes.items()}
        depth = max([len(v) for v in lists.values()] or [1])
        if depth < 2:
            return
        ims = [torch.randn(self.N, 3, self.H, self.W, device=self.device) for _ in range(self.groups)]
        bns = list(self.stack.bns()) if self.training else []
        saved = [(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns]
        for g, im in enumerate(ims):
            self.ops[g].in0 = im.data_ptr()
        us = (C.c_float * self.n_ops)()
        total = {key: [0.0] * len(v) for key, v in lists.items()}
        try:
            for k in range(depth):
                for key, ix in classes.items():
                    v = lists[key][min(k, len(lists[key]) - 1)]
                    for i in ix:
                        self.ops[i].variant = v
                for rep in range(6):                          # parity pairs; the first pair warms up
                    L.check(lib.sat_run_ops_timed(self.ops, self.n_ops, rep & 1, L.stream(), us), "sat_run_ops_timed")
                    if rep >= 2:
                        for key, ix in classes.items():
                            if k < len(lists[key]):
                                total[key][k] += sum(us[i] for i in ix)
        finally:
            # the passes ran with real momentum on the model's running statistics (ungrouped programs defer theirs only after the
            # build): put them back whatever happened, before anybody else can read them
            torch.cuda.synchronize()
            for acc in self.stat_accs:
                acc.zero_()
            for bn, (m, v) in zip(bns, saved):
                bn.running_mean.copy_(m)
                bn.running_var.copy_(v)
            self._parity, self._runs = 0, [0, 0]
        verbose = os.environ.get("SAT_TUNE_VERBOSE") is not None
        for key, ix in classes.items():
            best = min(range(len(lists[key])), key=lambda k: total[key][k])
            if verbose:
                import sys
                print("tune in program %s: %s -> v%d" % (key, ", ".join("v%d %.1f us" % (lists[key][k], total[key][k] / 4 / len(ix))
                                                                            for k in range(len(lists[key]))), lists[key][best]), file=sys.stderr)
            for i in ix:
                self.ops[i].variant = lists[key][best]
            _PROGRAM_PICKS[key] = lists[key][best]

    def signatures(self):
        """{conv layer: signature of the variant this program runs}: the BatchNorm statistics signature (training: tile shape and
        summation order fix the bits of the statistics) or the output family (inference: only the K order matters).  Hand it to the
        other programs of the same model state (`signatures=`) and a batch gets bit-identical features from all of them."""
        out = {}
        if self.dtype != L.SAT_BF16:
            return out
        for i in range(self.n_ops):
            o = self.ops[i]
            if o.kind == L.OP_CONV and int(o.variant) > 0:
                if o.stat_partial or o.stat_acc:
                    out[T.layer_key(o)] = int(self.lib.sat_conv_variant_signature(int(o.variant)))
                else:
                    out[T.layer_key(o)] = int(self.lib.sat_conv_variant_family(int(o.variant)))
        return out

    def __del__(self):
        for g in getattr(self, "_graphs", ()):
            if g is not None:
                try:
                    L.load().sat_graph_destroy(g)
                except Exception:
                    pass

    # ---- running statistics ----
    def defer_running_stats(self):
        """Aim every running-statistics update of this (train-mode) program at private zeroed buffers with momentum 1, so that a
        run leaves each layer's batch (mean, unbiased var) there and touches NO model state; `apply_running_stats()` then does
        the real momentum update in one launch.  Lets several batches' frozen stacks be in flight at once while the model's
        running statistics still advance in batch order (TrainStep.prefetch_encoder).  Call before the first run.
        Grouped programs: the log of a BatchNorm is [G][2][C] (what sat_op.groups expects) and every group has its own table."""
        if not self.training or self._running_items is not None:
            return
        if self._runs != [0, 0]:
            raise RuntimeError("defer_running_stats must precede the first run (the hipGraph captures the pointers)")
        dev = self.pooled.device
        G = self.groups
        by_ptr = {bn.running_mean.data_ptr(): bn for bn in self.stack.bns()}
        items, seen = [[] for _ in range(G)], set()
        for i in range(self.n_ops):
            o = self.ops[i]
            hit = False
            for fm, fv in (("running_mean", "running_var"), ("running_mean1", "running_var1")):
                ptr = getattr(o, fm)
                if not ptr:
                    continue
                bn = by_ptr.get(ptr)
                if bn is None or ptr in seen:
                    raise RuntimeError("op %d updates running statistics this program cannot attribute to one BatchNorm" % i)
                seen.add(ptr)
                c = bn.running_mean.numel()
                log = torch.zeros(G, 2, c, dtype=torch.float32, device=dev)
                self.keep.append(log)
                setattr(o, fm, log[0, 0].data_ptr())
                setattr(o, fv, log[0, 1].data_ptr())
                for g in range(G):
                    it = L.SatBnRunningItem()
                    it.running_mean, it.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                    it.batch_mean, it.batch_var, it.C = log[g, 0].data_ptr(), log[g, 1].data_ptr(), c
                    items[g].append(it)
                hit = True
            if hit:
                o.momentum = 1.0           # running' = 0 * running + 1 * f32(batch statistic): the log holds the statistic itself
        self._running_tables = []
        for g in range(G):
            arr = (L.SatBnRunningItem * max(len(items[g]), 1))(*items[g])
            self._running_tables.append(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev))
        self._running_items = len(items[0])

    def apply_running_stats(self, group=0):
        """Momentum update of the model's running statistics from the last run's batch statistics of `group` (deferred programs
        only), on the current stream; the caller has ordered that stream behind the run."""
        if self._running_items:
            L.check(L.load().sat_bn_running_apply(self._running_tables[group].data_ptr(), self._running_items, BN_MOMENTUM, L.stream()),
                    "sat_bn_running_apply")
            L.counter_add(self.stack._nbt_flat)

    # ---- running ----
    def pooled_of(self, group=0):
        """pooled features f32 [N, feature_dim] of one group's batch (a view of the program's output buffer)"""
        return self.pooled[group * self.N:(group + 1) * self.N]

    def _images_list(self, images):
        ims = list(images) if isinstance(images, (list, tuple)) else [images]
        if len(ims) != self.groups:
            raise ValueError("this program runs %d image batch(es) per launch, got %d" % (self.groups, len(ims)))
        out = []
        for im in ims:
            L.require_gpu(im, "images")
            if im.dtype != torch.float32 or tuple(im.shape) != (self.N, 3, self.H, self.W):
                raise ValueError("images must be float32 [%d,3,%d,%d]" % (self.N, self.H, self.W))
            out.append(im.contiguous())
        return out

    def run(self, images):
        """images f32 [N,3,H,W] NCHW on the device (grouped program: a list of `groups` such batches) -> pooled f32
        [groups * N, feature_dim] (owned by the program; `pooled_of(g)` = one batch's rows)."""
        ims = self._images_list(images)
        lib, p, npre = L.load(), self._parity, self._n_prep
        for g, im in enumerate(ims):
            self.ops[g].in0 = im.data_ptr()
        if not self._use_graph or self._runs[p] == 0:
            L.check(lib.sat_run_ops_parity(self.ops, self.n_ops, p, L.stream()), "sat_run_ops")
        else:
            # image prep reads the caller's tensors (new pointers every batch) -> eager; everything after it only
            # touches the program's own buffers -> one hipGraph per step parity, captured on this parity's 2nd run
            if self._graphs[p] is None:
                tail = (L.SatOp * (self.n_ops - npre))(*list(self.ops)[npre:])
                g = C.c_void_p()
                L.check(lib.sat_graph_create(tail, self.n_ops - npre, p, C.byref(g)), "sat_graph_create")
                self._graphs[p] = g
            L.check(lib.sat_run_ops_parity(self.ops, npre, p, L.stream()), "sat_run_ops")
            L.check(lib.sat_graph_launch(self._graphs[p], L.stream()), "sat_graph_launch")
        self._runs[p] += 1
        self._parity ^= 1
        if self.training and self._running_items is None:
            L.counter_add(self.stack._nbt_flat)
        return self.pooled

    def run_timed(self, images):
        """Diagnostics (bench.py's roofline figure): one eager, in-order run of the whole program -- same kernels, same
        statistics / parity bookkeeping as `run` -- that also returns every conv launch's own duration in microseconds
        (dispatch timestamps via `sat_run_ops_timed`).  Synchronises the stream."""
        ims = self._images_list(images)
        lib, p = L.load(), self._parity
        for g, im in enumerate(ims):
            self.ops[g].in0 = im.data_ptr()
        us = (C.c_float * self.n_ops)()
        L.check(lib.sat_run_ops_timed(self.ops, self.n_ops, p, L.stream(), us), "sat_run_ops_timed")
        self._runs[p] += 1
        self._parity ^= 1
        if self.training and self._running_items is None:
            L.counter_add(self.stack._nbt_flat)
        return self.pooled, [float(us[i]) for i in range(self.n_ops) if self.ops[i].kind == L.OP_CONV]
