"""Self-critical sequence training (Rennie et al. 2017) on the device: a caption SAMPLED from the model is trained with its cross
entropy weighted by CIDEr(sampled) - CIDEr(greedy), the number `train.py:169-177` keeps `model-best.pth` by.

    sc = sat.SelfCritical(scorer)                       # scorer: a `CiderScorer` over the training references
    loss = sc(model.decoder, features, image_index)     # rollout, greedy baseline, two CIDEr calls, weighted CE: no host read
    loss.backward()

With `len[b]` the sampled tokens of row b up to and including its first <end> and M = sum(len) (or `denom`):

    loss = sum over b, t < len[b] of (reward[b] - baseline[b]) / M * -log softmax(logits[t * B + b])[ids[b][t]]

`sat_scst_weights` makes the per-row weights, `sat_ce_rows_weighted` the loss and d(loss)/d(logits); the arithmetic is stated at
both in include/sat_hip.h.  `TrainStep.scst_step` is the fused form.  There is no CPU path.

S captions per image (Luo 2020, arXiv:2003.09971): `sat.SelfCritical(scorer, num_samples=5, baseline="sample_mean")` draws R = B * S
rows (row b * S + s) from one set of features and judges each against the mean reward of the image's other S - 1 rows, with no
greedy decode; `baseline="greedy"` keeps one arg-max decode per image.  `sat_scst_weights_group` makes the weights (the
leave-one-out advantage is a sum of differences: S equal rewards give exactly 0), `sat_group_sum_rows` sums the R-row gradient of
the repeated inputs per image.  The defaults, one sample and the greedy baseline, are the calls above.

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


BASELINES = ("greedy", "sample_mean")


def check_group(num_samples, baseline="greedy"):
    """(S, baseline name) of a self-critical call, checked on the host before anything is launched: S an int >= 1; baseline
    "greedy" (CIDEr of the arg-max decode, one per image) or "sample_mean" (leave-one-out over the S >= 2 samples of an image)"""
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
        raise ValueError("num_samples must be an int >= 1, got %r" % (num_samples,))
    if not isinstance(baseline, str) or baseline not in BASELINES:
        raise ValueError("baseline must be one of %s, got %r" % (BASELINES, baseline))
    if baseline == "sample_mean" and num_samples < 2:
        raise ValueError("baseline='sample_mean' is the mean reward of the OTHER samples of an image: num_samples must be >= 2")
    return num_samples, baseline


def _ids_groups(ids, S=None):
    """ids as [B, S, T]: given so, or [B * S, T] rows in image-major order with S named"""
    if ids.dim() == 2 and S is not None:
        if ids.shape[0] % S:
            raise ValueError("ids has %d rows, no multiple of num_samples = %d" % (ids.shape[0], S))
        _ids_matrix(ids)
        if ids.shape[0] > 1 and ids.stride(0) != ids.shape[1]:
            ids = ids.contiguous()
        return ids.view(ids.shape[0] // S, S, ids.shape[1])
    L.require_gpu(ids, "ids")
    if ids.dim() != 3 or ids.dtype != torch.int64 or (S is not None and ids.shape[1] != S):
        raise TypeError("ids must be an int64 [B, S, T] tensor%s" % ("" if S is None else " with S = %d" % S))
    return ids.contiguous()


def scst_weights_group(ids, reward, baseline=None, end_id=2, denom=None):
    """`sat_scst_weights_group` for ids [B, S, T], S sampled captions per image (row r = b * S + s): returns (w f32 [T * R] in
    the rollout's packed order t * R + r, len i32 [R], M f64 [1], advantage f64 [R], baseline_rows f64 [R]), R = B * S.
    reward: device f32 or f64 [R].  baseline: None (0) or a device tensor [B], one value per image (mode 0), or "sample_mean":
    the leave-one-out mean of the other S - 1 samples' rewards (mode 1, S >= 2; Luo 2020) -- the arithmetic is stated at the
    entry point in include/sat_hip.h.  denom as for `scst_weights`."""
    if isinstance(baseline, str) and baseline != "sample_mean":
        raise ValueError("baseline must be None, a [B] tensor or 'sample_mean', got %r" % (baseline,))
    ids = _ids_groups(ids)
    B, S, T = ids.shape
    mode = 1 if isinstance(baseline, str) else 0
    if mode == 1 and S < 2:
        raise ValueError("baseline='sample_mean' needs at least 2 samples per image, ids has S = %d" % S)
    R, dev = B * S, ids.device
    reward = _f64_vector(reward, R, "reward")
    base = None if mode == 1 or baseline is None else _f64_vector(baseline, B, "baseline")
    denom = None if denom is None else _f64_vector(denom, 1, "denom")
    w = torch.empty(T * R, device=dev)
    length = torch.empty(R, dtype=torch.int32, device=dev)
    M = torch.empty(1, dtype=torch.float64, device=dev)
    adv, rows = torch.empty(R, dtype=torch.float64, device=dev), torch.empty(R, dtype=torch.float64, device=dev)
    L.check(L.load().sat_scst_weights_group(ids.data_ptr(), T, B, S, T, int(end_id), L.ptr(reward), L.ptr(base), mode, L.ptr(denom),
                                            L.ptr(w), L.ptr(length), L.ptr(M), L.ptr(adv), L.ptr(rows), L.stream()),
            "sat_scst_weights_group")
    return w, length, M, adv, rows


def group_sum_rows(x, S, out=None):
    """`sat_group_sum_rows`: x f32 [B * S, ...] (dense) -> [B, ...], out[b] = ((x[b*S] + x[b*S+1]) + ...) in f32, ascending s --
    the backward of repeating every image's row S times.  out: None, or the dense f32 [B, ...] tensor on x's device to write"""
    S = check_group(S)[0]
    L.require_gpu(x, "x")
    if x.dtype != torch.float32 or x.dim() < 1 or x.shape[0] % S:
        raise TypeError("x must be float32 with a multiple of %d rows" % S)
    x = x.contiguous()
    B, W = x.shape[0] // S, x[0].numel()
    shape = (B,) + tuple(x.shape[1:])
    if out is None:
        out = torch.empty(shape, device=x.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != x.device or tuple(out.shape) != shape
          or not out.is_contiguous()):
        raise TypeError("out must be a dense float32 tensor of shape %s on %s" % (shape, x.device))
    L.check(L.load().sat_group_sum_rows(L.ptr(x), W, B, S, W, L.ptr(out), W, L.stream()), "sat_group_sum_rows")
    return out


class _RepeatRowsFn(torch.autograd.Function):
    """x [B, ...] -> [B * S, ...], every image's row S times in a row (data movement); backward `sat_group_sum_rows`"""

    @staticmethod
    def forward(ctx, x, S):
        ctx.S = S
        return x.repeat_interleave(S, 0)

    @staticmethod
    def backward(ctx, g):
        return group_sum_rows(g, ctx.S), None


def repeat_rows(x, S):
    """x with every row S times in a row (row b * S + s = x[b]); the gradient comes back through `sat_group_sum_rows`"""
    return _RepeatRowsFn.apply(x, S) if S > 1 else x


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
    def forward(ctx, logits, ids, reward, baseline, end_id, denom, out=None):
        """ids [B, T] (one caption per image: `sat_scst_weights`) or [B, S, T] (`sat_scst_weights_group`; out, a dict, then
        receives "advantage" and "baseline", f64 [B * S])"""
        N, V = logits.shape
        grad = L.logits_buffer(N, V, logits.device)         # the caller's logits stay what they are: the gradient gets a buffer
        grad[:, :V].copy_(logits)
        if ids.dim() == 2:
            w, _, _ = scst_weights(ids, reward, baseline, end_id, denom)
        else:
            w, _, _, adv, rows = scst_weights_group(ids, reward, baseline, end_id, denom)
            ids = ids.view(-1, ids.shape[2])
            if out is not None:
                out["advantage"], out["baseline"] = adv, rows
        _, loss = ce_rows_weighted(grad[:, :V], ids, w, write_grad=True)
        ctx.grad, ctx.V = grad, V
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        return (ctx.grad * g)[:, :ctx.V], None, None, None, None, None, None


def scst_loss(logits, ids, reward, baseline=None, end_id=2, denom=None, num_samples=1):
    """The self-critical loss (module docstring) of a rollout's (logits, ids) as a 0-dim f32 device tensor.  reward, baseline:
    device f32 or f64 [B], constants of the loss (no gradient flows into them); denom: see `scst_weights`.  Backward hands
    w[n] * (softmax - onehot), computed in the forward, to the rollout's backward.

    num_samples = S > 1 (or ids given as [B, S, T], which names S by itself: a num_samples > 1 beside it must agree): S captions
    per image, ids [B, S, T] or its [B * S, T] rows, logits [T * B * S, V], reward [B * S]; baseline None, a [B] tensor (one value
    per image) or "sample_mean", the leave-one-out mean of the image's other samples (`scst_weights_group`).  With S = 1 and a
    [B] or None baseline the call is `sat_scst_weights`, exactly as without the keyword."""
    return _scst_loss(logits, ids, reward, baseline, end_id, denom, num_samples, None)


def _scst_loss(logits, ids, reward, baseline, end_id, denom, num_samples, out):
    """`scst_loss`; out: None or a dict that receives "advantage" and "baseline", f64 [B * S], of a call with S rows per image"""
    S = check_group(num_samples)[0]
    if ids.dim() == 3:                                      # host checks first: they are the same without a GPU
        if S > 1 and ids.shape[1] != S:
            raise ValueError("ids %s holds %d samples per image, num_samples says %d" % (tuple(ids.shape), ids.shape[1], S))
        S = int(ids.shape[1])
    if isinstance(baseline, str):
        check_group(S, baseline)
        if baseline != "sample_mean":
            raise ValueError("baseline must be None, a [B] tensor or 'sample_mean', got %r" % (baseline,))
    L.require_gpu(logits, "logits")
    if ids.dim() == 2 and S == 1:
        return _ScstLossFn.apply(logits, ids, reward, baseline, int(end_id), denom, None)
    return _ScstLossFn.apply(logits, _ids_groups(ids, S), reward, baseline, int(end_id), denom, out)


def _repeat_index(image_index, S):
    """image_index with every entry S times in a row: the corpus image of row b * S + s"""
    if torch.is_tensor(image_index):
        return image_index.repeat_interleave(S)
    return [i for i in image_index for _ in range(S)]


class SelfCritical:
    """`sc(decoder, features, image_index)`: `decoder.rollout`, `decoder.sample` (greedy, from the same features) as the baseline,
    `kept_tokens` and `scorer.score` of both id sets, `scst_loss`.  Leaves last_reward / last_baseline (device f64 [B]), last_ids
    (the sampled ids) and last_greedy_ids.  Nothing is read back to the host.

    num_samples = S > 1: the rollout draws S captions per image (R = B * S rows, row b * S + s; `rollout(num_samples=S)`), the
    scorer sees `image_index` repeated to R rows, and last_ids is [B, S, T], last_reward / last_baseline / last_advantage f64 [R].
    baseline="greedy": one arg-max decode per image, its score the baseline of the image's S rows.  baseline="sample_mean" (Luo
    2020, arXiv:2003.09971; S >= 2): every row's baseline is the mean reward of the image's other S - 1 rows -- no greedy decode is
    launched and last_greedy_ids stays None.  The defaults make exactly the calls made without the keywords."""

    def __init__(self, scorer, end_id=2, *, num_samples=1, baseline="greedy"):
        self.num_samples, self.baseline = check_group(num_samples, baseline)
        self.scorer, self.end_id = scorer, int(end_id)
        self.last_reward = self.last_baseline = self.last_ids = self.last_greedy_ids = self._advantage = None

    @property
    def last_advantage(self):
        """f64 [R]: what weighted the rows of the last loss (with one sample per image: last_reward - last_baseline, made on demand)"""
        if self._advantage is None and self.last_reward is not None:
            return self.last_reward - self.last_baseline
        return self._advantage

    def _score(self, ids, greedy_ids, image_index):
        """(reward, baseline): the scorer's per-row score of the sampled rows and of the greedy rows, each up to its <end>"""
        kept_s, kept_g = kept_tokens(ids, self.end_id), kept_tokens(greedy_ids, self.end_id)
        _, reward = self.scorer.score(ids, image_index, end_id=self.end_id, kept=kept_s)
        _, baseline = self.scorer.score(greedy_ids, image_index, end_id=self.end_id, kept=kept_g)
        return reward, baseline

    def _score_group(self, ids, greedy_ids, image_index):
        """(reward f64 [R], baseline): ids [B, S, T] scored as R rows against `image_index` repeated; the baseline is the greedy
        rows' score f64 [B], or "sample_mean" when there are none"""
        rows = ids.view(-1, ids.shape[2])
        _, reward = self.scorer.score(rows, _repeat_index(image_index, ids.shape[1]), end_id=self.end_id,
                                      kept=kept_tokens(rows, self.end_id))
        if greedy_ids is None:
            return reward, "sample_mean"
        _, baseline = self.scorer.score(greedy_ids, image_index, end_id=self.end_id, kept=kept_tokens(greedy_ids, self.end_id))
        return reward, baseline

    def _finish(self, logits, ids, greedy_ids, reward, baseline):
        if ids.dim() == 3:
            out = {}
            loss = _scst_loss(logits, ids, reward, baseline, self.end_id, None, ids.shape[1], out)
            baseline, self._advantage = out["baseline"], out["advantage"]
        else:
            loss = scst_loss(logits, ids, reward, baseline, self.end_id)
        self.last_reward, self.last_baseline, self.last_ids, self.last_greedy_ids = reward, baseline, ids, greedy_ids
        return loss

    def _greedy(self, decoder, features):
        greedy = decoder.sample(features)
        if greedy.dim() == 1:                                # squeezed at batch 1 (models.py:67)
            greedy = greedy.view(1, -1)
        return greedy

    def rewards(self, decoder, features, ids, image_index):
        """(reward, baseline, greedy ids) for sampled `ids`: CIDEr of the sampled rows and of the greedy decode.  ids [B, S, T]:
        reward f64 [B * S]; baseline f64 [B] of the greedy rows, or with baseline="sample_mean" the string itself and no decode"""
        if ids.dim() == 3:
            greedy = self._greedy(decoder, features) if self.baseline == "greedy" else None
            return self._score_group(ids, greedy, image_index) + (greedy,)
        greedy = self._greedy(decoder, features)
        return self._score(ids, greedy, image_index) + (greedy,)

    def __call__(self, decoder, features, image_index, steps=20):
        if self.num_samples == 1:
            ids, logits = decoder.rollout(features, steps)
        else:
            ids, logits = decoder.rollout(features, steps, num_samples=self.num_samples)
        reward, baseline, greedy = self.rewards(decoder, features, ids, image_index)
        return self._finish(logits, ids, greedy, reward, baseline)

    def attend(self, model, features, fmean, image_index, steps=20):
        """The same for the attention model (`ShowAttendTellModel`): `model.rollout(features, fmean, steps)` sampled, and
        `model.rollout(..., greedy=True)` -- the arg-max decode of the same policy, which consumes no seed -- as the baseline.
        Leaves the same last_* fields as `__call__`."""
        if self.num_samples == 1:
            ids, logits = model.rollout(features, fmean, steps)
        else:
            ids, logits = model.rollout(features, fmean, steps, num_samples=self.num_samples)
        greedy = None
        if self.baseline == "greedy":
            fed, alphas = model.last_rollout_inputs, model.last_alphas    # the sampled rollout's: what the backward belongs to
            greedy, _ = model.rollout(features, fmean, steps, greedy=True)
            model.last_rollout_inputs, model.last_alphas = fed, alphas
        if ids.dim() == 3:
            reward, baseline = self._score_group(ids, greedy, image_index)
        else:
            reward, baseline = self._score(ids, greedy, image_index)
        return self._finish(logits, ids, greedy, reward, baseline)
