"""The rollout of the Show-Attend-Tell decoder (`sat_rollout_attend_fwd`) on the CPU oracle: `oracle.attend`'s own layers step by
step, the draw of `ss_reference.noise` in float64 -- the attention model's counterpart of `scst_reference.oracle_rollout` -- and the
shapes, parameters and seeds the rollout tests share."""
import numpy as np
import torch

import ss_reference as R

SMALL = dict(P=16, C=32, E=32, H=64, V=300)          # tests/test_gpu_ss_attend.py's: V is no multiple of 16
STEPS = 6
START, END = 1, 2

# (B, rank, steps, torch.manual_seed) of the replay tests; B 65 crosses the skinny kernel's 64-row chunk.  The host test checks that
# no draw of these seeds is a near tie (top-two gap < 1e-4) on the oracle's logits.
REPLAY_CASES = [(5, 0, STEPS, 201), (5, 3, STEPS, 202), (1, 0, STEPS, 203), (65, 0, 3, 204)]


def params(OA, seed=0, dims=SMALL):
    return OA.init_attend_params(dims["H"], dims["C"], dims["V"], dims["E"], generator=torch.Generator().manual_seed(seed),
                                 feat=dims["C"])


def features(B, seed=1, dims=SMALL):
    """[B, P, C], post-ReLU like the conv stack's"""
    return torch.randn(B, dims["P"], dims["C"], generator=torch.Generator().manual_seed(seed)).clamp(min=0)


def oracle_rollout(OA, p, feats, steps, seed, rank, start_id=START, greedy=False):
    """model2.py:38-85 fed its own tokens: step 0 takes start_id, step t >= 1 the token taken from step t-1's logits -- the float64
    Gumbel-max draw of counter (v >> 2, b, t, 2*rank), or with `greedy` the first maximal column.  Returns (ids [B, steps], margin
    [B, steps] = the gap between the best and second-best (perturbed) score, logits [steps * B, V] in p's dtype, fed [B, steps])."""
    B = feats.shape[0]
    V = p["classifier.weight"].shape[0]
    ids = torch.zeros(B, steps, dtype=torch.int64)
    fed = torch.zeros(B, steps, dtype=torch.int64)
    margin = np.empty((B, steps))
    ctx_enc = feats @ p["image_att_w"]
    h, c = OA.init_lstm(p, feats)
    tok = torch.full((B,), int(start_id), dtype=torch.int64)
    outs = []
    for t in range(steps):
        fed[:, t] = tok
        context, _ = OA.attention_layer(p, feats, ctx_enc, h)
        h, c = OA.lstmcell(p, torch.cat([p["embedding.weight"][tok], context], 1), h, c)
        logits = OA.output_layer(p, context, h)
        outs.append(logits)
        lg = logits.detach().numpy().astype(np.float64)
        for b in range(B):
            s = lg[b] if greedy else lg[b] + R.noise(seed, rank, b, t, V)
            top = np.sort(s)[-2:]
            ids[b, t] = int(np.argmax(s))
            margin[b, t] = top[1] - top[0]
        tok = ids[:, t].clone()
    return ids, margin, torch.cat(outs, 0), fed
