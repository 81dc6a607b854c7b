"""CPU restatement of the Show-Attend-Tell decoder WITH its attention maps and the doubly stochastic penalty (Xu et al. 2015,
section 4.2.1), built from `oracle.attend`'s own functions.  A plain helper module (like ss_reference.py): the forward that returns
the per-step alphas, the penalty, loss and gradients by autograd of CE + penalty, greedy decode with alphas, and the oracle's beam
loop carrying the alphas along with h and c.  Runs in the dtype of its inputs (the tests feed float64)."""
import torch
import torch.nn.functional as F

from oracle import attend as OA

# The penalty weight of the model tests (tests/test_alpha_host.py::test_penalty_moves_the_attention_gradients_far_beyond_the_gpu_tolerance):
# on the G6 configuration alpha_c = 1 moves the gradient of weight_hh.weight by only ~10 x the GPU test's tolerance (weight_att
# ~4700 x, image_att_w ~850 x); 16 moves it ~170 x, so a dropped injection cannot pass.
MODEL_TEST_ALPHA_C = 16.0
GRAD_RTOL, GRAD_ATOL = 2e-3, 2e-7          # the golden test's gradient tolerances (tests/test_gpu_attend.py)


def forward(p, features, captions, lengths):
    """`OA.attend_forward` keeping what `attention_layer` returns: (logits [N, V], [alpha_t [bs_t, P] for every step])."""
    emb = p["embedding.weight"][captions]
    context_encode = features @ p["image_att_w"]
    h, c = OA.init_lstm(p, features)
    outs, alphas = [], []
    for t, bs in enumerate(OA.batch_sizes(lengths)):
        context, alpha = OA.attention_layer(p, features[:bs], context_encode[:bs], h[:bs])
        h, c = OA.lstmcell(p, torch.cat([emb[:bs, t], context], 1), h[:bs], c[:bs])
        outs.append(OA.output_layer(p, context, h))
        alphas.append(alpha)
    return torch.cat(outs, 0), alphas


def coverage(alphas, B):
    """cov[b, p] = sum of alpha_t[b, p] over the steps image b is alive in: [B, P]"""
    return sum(F.pad(a, (0, 0, 0, B - a.shape[0])) for a in alphas)


def penalty(alphas, B, alpha_c=1.0):
    """alpha_c * mean_{b,p} (1 - sum_t alpha[b,t,p])^2"""
    return alpha_c * ((1.0 - coverage(alphas, B)) ** 2).mean()


def loss_and_grads(p, features, captions_in, lengths, targets, alpha_c, feature_grad=False):
    """mean CE of forward(captions_in) against `targets`, plus the penalty; autograd of the sum.
    Returns dict(loss, ce, penalty, grads, d_features, logits, alphas [N, P] packed)."""
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    f = features.clone().requires_grad_(feature_grad)
    logits, alphas = forward(q, f, captions_in, lengths)
    ce = F.cross_entropy(logits, targets)
    pen = penalty(alphas, features.shape[0], alpha_c) if alpha_c else torch.zeros((), dtype=logits.dtype)
    loss = ce + pen
    loss.backward()
    return dict(loss=loss.detach(), ce=ce.detach(), penalty=pen.detach(), grads={k: v.grad for k, v in q.items()},
                d_features=f.grad, logits=logits.detach(), alphas=torch.cat(alphas, 0).detach())


def greedy(p, features, states=None, start_id=1, steps=20):
    """`OA.attend_sample` returning (ids [B, steps], alphas [B, steps, P])"""
    B = features.shape[0]
    H = p["lstmcell.weight_hh"].shape[1]
    emb = p["embedding.weight"][torch.full((B,), start_id, dtype=torch.long)]
    context_encode = features @ p["image_att_w"]
    if states is None:
        h, c = torch.zeros(B, H, dtype=features.dtype), torch.zeros(B, H, dtype=features.dtype)
    else:
        h, c = states
    ids, maps, rnn_input = [], [], None
    for i in range(steps):
        context, alpha = OA.attention_layer(p, features, context_encode, h)
        if i == 0:
            rnn_input = torch.cat([emb, context], 1)
        h, c = OA.lstmcell(p, rnn_input, h, c)
        pred = OA.output_layer(p, context, h).max(1)[1]
        ids.append(pred)
        maps.append(alpha)
        rnn_input = torch.cat([p["embedding.weight"][pred], context], 1)
    return torch.stack(ids, 1), torch.stack(maps, 1)


def beam(p, features, beam_size=5, states=None, start_id=1, steps=20, end_id=None):
    """`OA.attend_beam_search`'s loop with the attention maps carried like h and c: a survivor inherits the maps of its parent
    and appends the map its parent's slot computed this step.  Returns (ids [B,K,steps], scores [B,K], alphas [B,K,steps,P])."""
    B, K = features.shape[0], beam_size
    V = p["classifier.weight"].shape[0]
    H = p["lstmcell.weight_hh"].shape[1]
    P = features.shape[1]
    dt = features.dtype
    rep = lambda t: t.repeat_interleave(K, 0)
    feats = rep(features)
    context_encode = feats @ p["image_att_w"]
    if states is None:
        h, c = torch.zeros(B * K, H, dtype=dt), torch.zeros(B * K, H, dtype=dt)
    else:
        h, c = rep(states[0]), rep(states[1])
    emb = p["embedding.weight"][torch.full((B * K,), start_id, dtype=torch.long)]
    scores = torch.full((B, K), float("-inf"), dtype=dt)
    scores[:, 0] = 0.0
    seqs = torch.zeros(B, K, 0, dtype=torch.int64)
    maps = torch.zeros(B, K, 0, P, dtype=dt)
    last, rnn_input = None, None
    for i in range(steps):
        context, alpha = OA.attention_layer(p, feats, context_encode, h)
        if i == 0:
            rnn_input = torch.cat([emb, context], 1)
        h, c = OA.lstmcell(p, rnn_input, h, c)
        logits = OA.output_layer(p, context, h)
        logp = torch.log_softmax(logits, dim=1).view(B, K, V)
        cand = scores.unsqueeze(2) + logp
        if end_id is not None and last is not None:
            fin = last == end_id
            frozen = torch.full((B, K, V), float("-inf"), dtype=dt)
            frozen[:, :, end_id] = scores
            cand = torch.where(fin.unsqueeze(2), frozen, cand)
        cand = cand.view(B, K * V)
        order = torch.sort(cand, dim=1, descending=True, stable=True)[1][:, :K]
        scores = torch.gather(cand, 1, order)
        parent, token = order // V, order % V
        rows = (torch.arange(B).unsqueeze(1) * K + parent).reshape(-1)
        h, c, context = h[rows], c[rows], context[rows]
        seqs = torch.cat([torch.gather(seqs, 1, parent.unsqueeze(2).expand(B, K, seqs.shape[2])), token.unsqueeze(2)], 2)
        maps = torch.cat([torch.gather(maps, 1, parent.view(B, K, 1, 1).expand(B, K, maps.shape[2], P)),
                          alpha[rows].view(B, K, 1, P)], 2)
        last = token
        rnn_input = torch.cat([p["embedding.weight"][token.reshape(-1)], context], 1)
    return seqs, scores, maps
