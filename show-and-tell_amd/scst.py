"""Self-critical sequence training (Rennie et al. 2017) on the device: a caption SAMPLED from the model is trained with its cross
entropy weighted by CIDEr(sampled) - CIDEr(greedy), the number `train.py:169-177` keeps `model-best.pth` by.

    sc = sat.SelfCritical(scorer)                       # scorer: a `CiderScorer` over the training references
    loss = sc(model.decoder, features, image_index)     # rollout, greedy baseline, two CIDEr calls, weighted CE: no host read
    loss.backward()

With `len[b]` the sampled tokens of row b up to and including its first <end> and M = sum(len) (or `denom`):

    loss = sum over b, t < len[b] of (reward[b] - baseline[b]) / M * -log softmax(logits[t * B + b])[ids[b][t]]

`sat_scst_weights` makes the per-row weights, `sat_ce_rows_weighted` the loss and d(loss)/d(logits); the arithmetic is stated at
both in include/sat_hip.h.  `TrainStep.scst_step` is the fused form.  There is no CPU path.

For the attention model (`ShowAttendTellModel`, the model `train.py:37` builds):

    loss = sc.attend(model, features, fmean, image_index)    # `model.rollout` sampled, and with greedy=True as the baseline
    loss = model.scst_forward(images, image_index, scorer)   # the same behind the conv stack"""
import torch

from . import _lib as L
from .evaluate import kept_tokens


def _ids_matrix(ids, name="ids"):
    L.require_gpu(ids, name)
    if ids.dim() != 2 or ids.dtype != torch.int64 or ids.stride(1) != 1:
        raise TypeError("%s must be an int64 matrix with contiguous rows" % name)
    return ids


def _f64_vector(t, n, name):
    L.require_gpu(t, name)
    if t.dtype not in (torch.float32, torch.float64) or t.numel() != n:
        raise TypeError("%s must be a float32 or float64 tensor of %d elements" % (name, n))
    return t.reshape(n).to(torch.float64).contiguous()          # (f32 -> f64 is exact)


def scst_weights(ids, reward, baseline=None, end_id=2, denom=None):
    """`sat_scst_weights`: (w f32 [T * B] in the rollout's packed order t * B + b, len i32 [B], M f64 [1]).  reward / baseline:
    device f32 or f64 [B] (baseline None: 0); denom: None or a 1-element device tensor that replaces M = sum(len) -- the global
    token count of a data-parallel step."""
    ids = _ids_matrix(ids)
    B, T = ids.shape
    dev = ids.device
    reward = _f64_vector(reward, B, "reward")
    baseline = None if baseline is None else _f64_vector(baseline, B, "baseline")
    denom = None if denom is None else _f64_vector(denom, 1, "denom")
    w = torch.empty(T * B, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    M = torch.empty(1, dtype=torch.float64, device=dev)
    L.check(L.load().sat_scst_weights(ids.data_ptr(), ids.stride(0), B, T, int(end_id), L.ptr(reward), L.ptr(baseline), L.ptr(denom),
                                      L.ptr(w), L.ptr(length), L.ptr(M), L.stream()), "sat_scst_weights")
    return w, length, M


def ce_rows_weighted(logits, ids, w, write_grad=True, loss_out=None):
    """`sat_ce_rows_weighted` over the rollout's logits [T * B, V] (row stride >= V) and ids [B, T]: returns (row_loss f32 [N],
    loss f32 [1] = sum w * row_loss).  write_grad: `logits` is overwritten IN PLACE with w[n] * (softmax - onehot)."""
    L.require_gpu(logits, "logits")
    ids = _ids_matrix(ids)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("logits must be a float32 matrix with contiguous rows")
    N, V = logits.shape
    B, T = ids.shape
    if N != B * T or w.numel() != N or w.dtype != torch.float32 or not w.is_contiguous():
        raise ValueError("logits has %d rows and w %d weights for ids %s" % (N, w.numel(), tuple(ids.shape)))
    L.require_gpu(w, "w")
    row_loss = torch.empty(N, device=logits.device)
    loss = torch.empty(1, device=logits.device) if loss_out is None else loss_out
    L.check(L.load().sat_ce_rows_weighted(logits.data_ptr(), logits.stride(0), ids.data_ptr(), ids.stride(0), B, N, V, L.ptr(w),
                                          1 if write_grad else 0, L.ptr(row_loss), L.ptr(loss), L.stream()), "sat_ce_rows_weighted")
    return row_loss, loss


class _ScstLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, ids, reward, baseline, end_id, denom):
        N, V = logits.shape
        grad = L.logits_buffer(N, V, logits.device)         # the caller's logits stay what they are: the gradient gets a buffer
        grad[:, :V].copy_(logits)
        w, _, _ = scst_weights(ids, reward, baseline, end_id, denom)
        _, loss = ce_rows_weighted(grad[:, :V], ids, w, write_grad=True)
        ctx.grad, ctx.V = grad, V
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        return (ctx.grad * g)[:, :ctx.V], None, None, None, None, None


def scst_loss(logits, ids, reward, baseline=None, end_id=2, denom=None):
    """The self-critical loss (module docstring) of a rollout's (logits, ids) as a 0-dim f32 device tensor.  reward, baseline:
    device f32 or f64 [B], constants of the loss (no gradient flows into them); denom: see `scst_weights`.  Backward hands
    w[n] * (softmax - onehot), computed in the forward, to the rollout's backward."""
    L.require_gpu(logits, "logits")
    return _ScstLossFn.apply(logits, ids, reward, baseline, int(end_id), denom)


class SelfCritical:
    """`sc(decoder, features, image_index)`: `decoder.rollout`, `decoder.sample` (greedy, from the same features) as the baseline,
    `kept_tokens` and `scorer.score` of both id sets, `scst_loss`.  Leaves last_reward / last_baseline (device f64 [B]), last_ids
    (the sampled ids) and last_greedy_ids.  Nothing is read back to the host."""

    def __init__(self, scorer, end_id=2):
        self.scorer, self.end_id = scorer, int(end_id)
        self.last_reward = self.last_baseline = self.last_ids = self.last_greedy_ids = None

    def _score(self, ids, greedy_ids, image_index):
        """(reward, baseline): the scorer's per-row score of the sampled rows and of the greedy rows, each up to its <end>"""
        kept_s, kept_g = kept_tokens(ids, self.end_id), kept_tokens(greedy_ids, self.end_id)
        _, reward = self.scorer.score(ids, image_index, end_id=self.end_id, kept=kept_s)
        _, baseline = self.scorer.score(greedy_ids, image_index, end_id=self.end_id, kept=kept_g)
        return reward, baseline

    def _finish(self, logits, ids, greedy_ids, reward, baseline):
        loss = scst_loss(logits, ids, reward, baseline, self.end_id)
        self.last_reward, self.last_baseline, self.last_ids, self.last_greedy_ids = reward, baseline, ids, greedy_ids
        return loss

    def rewards(self, decoder, features, ids, image_index):
        """(reward, baseline, greedy ids) for sampled `ids`: CIDEr of the sampled rows and of the greedy decode"""
        greedy = decoder.sample(features)
        if greedy.dim() == 1:                                # squeezed at batch 1 (models.py:67)
            greedy = greedy.view(1, -1)
        return self._score(ids, greedy, image_index) + (greedy,)

    def __call__(self, decoder, features, image_index, steps=20):
        ids, logits = decoder.rollout(features, steps)
        reward, baseline, greedy = self.rewards(decoder, features, ids, image_index)
        return self._finish(logits, ids, greedy, reward, baseline)

    def attend(self, model, features, fmean, image_index, steps=20):
        """The same for the attention model (`ShowAttendTellModel`): `model.rollout(features, fmean, steps)` sampled, and
        `model.rollout(..., greedy=True)` -- the arg-max decode of the same policy, which consumes no seed -- as the baseline.
        Leaves the same last_* fields as `__call__`."""
        ids, logits = model.rollout(features, fmean, steps)
        fed, alphas = model.last_rollout_inputs, model.last_alphas        # the sampled rollout's: what the backward belongs to
        greedy, _ = model.rollout(features, fmean, steps, greedy=True)
        model.last_rollout_inputs, model.last_alphas = fed, alphas
        reward, baseline = self._score(ids, greedy, image_index)
        return self._finish(logits, ids, greedy, reward, baseline)
