"""numpy / torch-f64 restatement of the self-critical loss (include/sat_hip.h, `sat_scst_weights` and `sat_ce_rows_weighted`) and
of the sampled rollout's draws (`sat_rollout_decoder_fwd`): what the tests check the library against."""
import numpy as np
import torch

import ss_reference as R


def lengths(ids, end_id):
    """len[b] = min(kept[b] + 1, T), kept[b] the ids in front of the first end_id (T when there is none)"""
    ids = np.asarray(ids)
    B, T = ids.shape
    out = np.empty(B, dtype=np.int32)
    for b in range(B):
        hit = np.flatnonzero(ids[b] == end_id)
        kept = int(hit[0]) if len(hit) else T
        out[b] = min(kept + 1, T)
    return out


def weights(ids, reward, baseline=None, end_id=2, denom=None):
    """(w f32 [T * B] with row t * B + b, len i32 [B], M f64): w = (float)((reward - baseline) / M) for t < len[b], +0 after;
    M = sum(len) or denom; float64 arithmetic, rounded once"""
    ids = np.asarray(ids)
    B, T = ids.shape
    ln = lengths(ids, end_id)
    M = np.float64(ln.astype(np.int64).sum()) if denom is None else np.float64(denom)
    adv = np.asarray(reward, dtype=np.float64) - (0.0 if baseline is None else np.asarray(baseline, dtype=np.float64))
    wb = (adv / M).astype(np.float32)
    w = np.zeros((T, B), dtype=np.float32)
    for b in range(B):
        w[:ln[b], b] = wb[b]
    return w.reshape(-1), ln, M


def targets(ids):
    """the target of packed row t * B + b: ids[b][t]"""
    return torch.as_tensor(np.asarray(ids)).t().reshape(-1)


def loss_and_grad(logits, ids, w):
    """torch f64: (row_loss [N], loss = sum w * row_loss over rows of non-zero weight, grad [N, V] = w * (softmax - onehot), rows of
    weight 0 exactly 0 whatever their logits hold)"""
    x = torch.as_tensor(logits).double()
    w = torch.as_tensor(np.asarray(w)).double()
    tgt = targets(ids)
    live = w != 0
    row_loss = torch.zeros(x.shape[0], dtype=torch.float64)
    grad = torch.zeros_like(x)
    xl = x[live]
    lse = torch.logsumexp(xl, 1)
    row_loss[live] = lse - xl.gather(1, tgt[live].view(-1, 1)).view(-1)
    p = torch.exp(xl - lse.view(-1, 1))
    p[torch.arange(xl.shape[0]), tgt[live]] -= 1.0
    grad[live] = p * w[live].view(-1, 1)
    return row_loss, (w[live] * row_loss[live]).sum(), grad


def replay(logits, B, steps, V, seed, rank):
    """Replay of a rollout's draws from its f32 logits [steps * B, >= V] in float64: (ids [B, steps], margin [B, steps]), margin
    the gap between the best and the second-best perturbed score"""
    lg = np.asarray(logits)[:, :V].astype(np.float64)
    ids = np.empty((B, steps), dtype=np.int64)
    margin = np.empty((B, steps))
    for t in range(steps):
        for b in range(B):
            s = lg[t * B + b] + R.noise(seed, rank, b, t, V)
            top = np.sort(s)[-2:]
            ids[b, t] = int(np.argmax(s))
            margin[b, t] = top[1] - top[0]
    return ids, margin


# (Lh, rank, B, V, torch.manual_seed) of the replay tests: E 32, H 64, 6 steps; V 203 leaves a partial last 16-column group.  The
# host test checks that no draw of these seeds is a near tie (top-two gap < 1e-4) on the oracle's logits.
REPLAY_E, REPLAY_H, REPLAY_STEPS = 32, 64, 6
REPLAY_CASES = [(1, 0, 5, 203, 101), (1, 3, 5, 203, 102), (2, 0, 5, 203, 103), (2, 3, 5, 203, 104), (1, 0, 1, 203, 105),
                (1, 0, 5, 1003, 106)]


def replay_inputs(OD, Lh, B, V):
    """(oracle decoder parameters, features [B, E]) of a replay case"""
    g = torch.Generator().manual_seed(40 + Lh)
    params = OD.init_decoder_params(REPLAY_E, REPLAY_H, V, Lh, generator=g)
    return params, torch.randn(B, REPLAY_E, generator=g)


def oracle_rollout(OD, params, feats, steps, seed, rank, Lh):
    """the rollout on the CPU oracle: step t's logits from the teacher-forced forward on the tokens drawn so far, the draw in
    float64.  Returns (ids [B, steps], margin [B, steps], logits f32 [steps * B, V])"""
    B = feats.shape[0]
    V = params["linear.weight"].shape[0]
    ids = torch.zeros(B, steps, dtype=torch.int64)
    margin = np.empty((B, steps))
    for t in range(steps):
        logits = OD.decoder_forward(params, feats, ids[:, :t], [t + 1] * B, Lh)
        lg = logits.numpy()[t * B:(t + 1) * B].astype(np.float64)
        for b in range(B):
            s = lg[b] + R.noise(seed, rank, b, t, V)
            top = np.sort(s)[-2:]
            ids[b, t] = int(np.argmax(s))
            margin[b, t] = top[1] - top[0]
    return ids, margin, logits
