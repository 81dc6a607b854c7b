"""The criterion of a teacher-forced loop, `nn.CrossEntropyLoss(label_smoothing=)` of train.py:53,143, on the device:

    crit = sat.CrossEntropy(label_smoothing=0.1)
    outputs = decoder(features, captions, lengths)          # or ShowAttendTellModel.forward: f32 [N, V]
    loss = crit(outputs, targets) + model.last_attention_penalty
    loss.backward()
    ppl = crit.last_nll.exp()                               # the smoothed loss is not the negative log-likelihood

One `sat_ce_rows_ls` launch (arithmetic at its declaration in include/sat_hip.h) gives the mean smoothed loss over the N rows, the
plain mean NLL and d(loss)/d(outputs); the gradient is written out of place, so the caller's `outputs` stay what they are, and the
backward multiplies it by the incoming scalar.  Nothing is read back to the host.  There is no CPU path.

Targets outside [0, V) are CLAMPED by the kernel, for memory safety only: torch raises on them.  The module range-checks every
batch of targets on the device as `watch.IdGuard` does for captions -- the IndexError comes at the next call at the latest, or at
once from `crit.check_ids()`.  The function form checks only when it is handed a `guard`.

Token-level unlikelihood training (Welleck et al. 2019, arXiv:1908.04319) against the repetitive captions of maximum-likelihood
training: every row also pays `unlikelihood * sum_c -log(1 - p_c)` over the distinct tokens c already emitted in its own caption
(the ground-truth targets of the earlier steps, the row's own target excluded):

    crit = sat.CrossEntropy(label_smoothing=0.1, unlikelihood=1.0)
    targets = pack_padded_sequence(captions[:, 1:], lengths, batch_first=True)[0]
    loss = crit(outputs, targets, lengths) + model.last_attention_penalty     # the SAME lengths: they say which rows are one caption
    crit.last_ul                                                              # mean of the rows' unweighted terms, f32 [1]

It is one `sat_ce_rows_ul` launch instead; with `unlikelihood == 0` the call is exactly the `sat_ce_rows_ls` call above."""
import math

import torch

from . import _lib as L
from .pack import PackInfo
from .watch import IdGuard

MAX_UL_STEPS = 64          # sat_ce_rows_ul: one wave holds a row's candidates


def _check_smoothing(label_smoothing):
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:                      # (a NaN fails both comparisons)
        raise ValueError("label_smoothing must be in [0, 1) (got %r)" % (label_smoothing,))
    return eps


def _check_unlikelihood(unlikelihood):
    alpha = float(unlikelihood)
    if not (alpha >= 0.0 and math.isfinite(alpha)):          # (a NaN fails the first)
        raise ValueError("unlikelihood must be a finite weight >= 0 (got %r)" % (unlikelihood,))
    return alpha


def _check_ul_lengths(lengths, N):
    """The pack layout of N target rows for the unlikelihood term: `lengths` as given to pack_padded_sequence"""
    if lengths is None:
        raise ValueError("unlikelihood > 0 needs the `lengths` the targets were packed with: they say which rows are one caption")
    lengths = [int(l) for l in lengths]
    if sum(lengths) != N:
        raise ValueError("lengths sum to %d, but there are %d target rows" % (sum(lengths), N))
    if lengths and max(lengths) > MAX_UL_STEPS:
        raise ValueError("unlikelihood supports captions of at most %d steps (got %d)" % (MAX_UL_STEPS, max(lengths)))
    return lengths


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, eps, out, alpha, pi):
        N, V = logits.shape
        dev = logits.device
        grad = L.logits_buffer(N, V, dev)          # the caller's logits stay what they are: the gradient gets a buffer
        row_loss, row_nll = torch.empty(N, device=dev), torch.empty(N, device=dev)
        loss, nll = torch.empty(1, device=dev), torch.empty(1, device=dev)
        if alpha > 0:
            row_ul, ul = torch.empty(N, device=dev), torch.empty(1, device=dev)
            L.check(L.load().sat_ce_rows_ul(logits.data_ptr(), logits.stride(0), targets.data_ptr(), L.ptr(pi.prefix_dev), pi.T, N, V,
                                            1.0 / N, eps, alpha, L.ptr(grad), grad.stride(0), L.ptr(row_loss), L.ptr(row_nll),
                                            L.ptr(row_ul), L.ptr(loss), L.ptr(nll), L.ptr(ul), L.stream()), "sat_ce_rows_ul")
        else:
            row_ul, ul = torch.zeros(N, device=dev), torch.zeros(1, device=dev)
            L.check(L.load().sat_ce_rows_ls(logits.data_ptr(), logits.stride(0), targets.data_ptr(), N, V, 1.0 / N, eps, L.ptr(grad),
                                            grad.stride(0), L.ptr(row_loss), L.ptr(row_nll), L.ptr(loss), L.ptr(nll), L.stream()),
                    "sat_ce_rows_ls")
        out["last_nll"], out["last_row_nll"] = nll, row_nll
        out["last_ul"], out["last_row_ul"] = ul, row_ul
        ctx.grad, ctx.V = grad, V
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        return (ctx.grad * g)[:, :ctx.V], None, None, None, None, None


def cross_entropy(outputs, targets, label_smoothing=0.0, out=None, guard=None, unlikelihood=0.0, lengths=None):
    """Mean over the N rows of the label-smoothed cross entropy of `outputs` (f32 [N, V], contiguous rows, on the device) against
    `targets` (int64 [N]): a 0-dim f32 device tensor with a backward.  `out`: a dict that receives "last_nll" (f32 [1], the plain
    mean NLL) and "last_row_nll" (f32 [N]).  `guard`: a `watch.IdGuard` that range-checks the targets (module
    docstring); without one, targets outside [0, V) are clamped silently.  `unlikelihood` > 0 adds that weight times the
    token-level unlikelihood term and needs `lengths`, the ones `targets` were packed with (non-increasing, sum N, at most 64
    steps); `out` then also receives "last_ul" (f32 [1], the mean unweighted term) and "last_row_ul" (f32 [N]) -- zeros without."""
    eps = _check_smoothing(label_smoothing)
    alpha = _check_unlikelihood(unlikelihood)
    if outputs.dim() != 2 or outputs.dtype != torch.float32 or outputs.stride(1) != 1:
        raise TypeError("outputs must be a float32 matrix with contiguous rows")
    if targets.dim() != 1 or targets.dtype != torch.int64 or targets.numel() != outputs.shape[0]:
        raise TypeError("targets must be an int64 vector with one id per row of outputs (%d)" % outputs.shape[0])
    if outputs.shape[0] < 1 or outputs.shape[1] < 1:
        raise ValueError("outputs must have at least one row and one column")
    if alpha > 0:
        lengths = _check_ul_lengths(lengths, outputs.shape[0])
    L.require_gpu(outputs, "outputs")
    L.require_gpu(targets, "targets")
    pi = PackInfo.get(lengths, outputs.device) if alpha > 0 else None
    targets = targets.contiguous()
    if guard is not None:
        guard.submit(targets.view(1, -1), targets.numel(), outputs.shape[1], "targets")
    return _CrossEntropyFn.apply(outputs, targets, eps, {} if out is None else out, alpha, pi)


class CrossEntropy(torch.nn.Module):
    """`nn.CrossEntropyLoss(label_smoothing=)` for the drop-in loop (module docstring).  After a call: `last_nll` (f32 [1] device
    tensor, the plain mean NLL of the batch: exp() of it is the perplexity) and `last_row_nll` (f32 [N]); `last_ul` (f32 [1], the
    mean over the rows of the unweighted unlikelihood term) and `last_row_ul` (f32 [N]).  `unlikelihood` > 0: call it as
    `crit(outputs, targets, lengths)` (module docstring)."""

    def __init__(self, label_smoothing=0.0, unlikelihood=0.0):
        super().__init__()
        self.label_smoothing = _check_smoothing(label_smoothing)
        self.unlikelihood = _check_unlikelihood(unlikelihood)
        self.last_nll = self.last_row_nll = self.last_ul = self.last_row_ul = None
        self._id_guard = None

    def id_guard(self, device):
        if self._id_guard is None or self._id_guard.status.device != device:
            self._id_guard = IdGuard(device)
        return self._id_guard

    def check_ids(self):
        """Block until the verdict on the last targets is known: IndexError for an id outside [0, V)"""
        if self._id_guard is not None:
            self._id_guard.poll(block=True)

    def forward(self, outputs, targets, lengths=None):
        out = {}
        guard = self.id_guard(targets.device) if targets.is_cuda else None
        loss = cross_entropy(outputs, targets, self.label_smoothing, out=out, guard=guard, unlikelihood=self.unlikelihood,
                             lengths=lengths)
        self.last_nll, self.last_row_nll = out["last_nll"], out["last_row_nll"]
        self.last_ul, self.last_row_ul = out["last_ul"], out["last_row_ul"]
        return loss
