"""Plain references of the constrained beam search (sat_beam_step_ex, sat_beam_rerank, sat_beam_decode_ex and the `sample_beam`
keywords): numpy / torch on the CPU, one obvious line per rule, nothing shared with the code under test.

The banned set of a live, unfinished hypothesis whose prefix is y_0..y_{i-1} (include/sat_hip.h):
  1. the suppressed ids, at every step;
  2. end_id while i < min_length;
  3. y_{i-1}, with block_repeat, from step 1 on;
  4. with no_repeat_ngram = n >= 1, from step n on: every token that would complete an n-gram the prefix already holds.
Scores are not renormalised: a candidate keeps base + log_softmax(all V logits)[v]; a banned v is simply no candidate.  Finished
and dead hypotheses are untouched.  The length penalty re-orders the K results once, after the last step."""
import numpy as np
import torch

import beam_reference as R


class Constraints:
    def __init__(self, suppress_ids=(), min_length=0, no_repeat_ngram=0, block_repeat=False, length_penalty=0.0):
        self.suppress_ids, self.min_length, self.no_repeat_ngram = tuple(suppress_ids), min_length, no_repeat_ngram
        self.block_repeat, self.length_penalty = block_repeat, length_penalty


def banned_tokens(prefix, end_id=None, suppress_ids=(), min_length=0, no_repeat_ngram=0, block_repeat=False):
    """the set of tokens a live, unfinished hypothesis with this prefix may not emit at step i = len(prefix)"""
    prefix = [int(t) for t in prefix]
    i, n = len(prefix), no_repeat_ngram
    banned = set(int(v) for v in suppress_ids)                                    # rule 1
    if end_id is not None and end_id >= 0 and i < min_length:                     # rule 2
        banned.add(int(end_id))
    if block_repeat and i >= 1:                                                   # rule 3
        banned.add(prefix[-1])
    if n >= 1 and i >= n:                                                         # rule 4
        tail = prefix[i - n + 1:]                                                 # the n - 1 tokens the next one would follow
        for j in range(0, i - n + 1):
            if prefix[j:j + n - 1] == tail:
                banned.add(prefix[j + n - 1])
    return banned


def banned_of(prefix, end_id, c):
    return banned_tokens(prefix, end_id, c.suppress_ids, c.min_length, c.no_repeat_ngram, c.block_repeat)


def prefixes_ref(parents, tokens, i):
    """parents, tokens [T, B, K] records, rows < i valid -> prefix[b][k]: the i tokens of the hypothesis in slot k before step i"""
    parents, tokens = np.asarray(parents), np.asarray(tokens)
    _, B, K = tokens.shape
    out = [[None] * K for _ in range(B)]
    for b in range(B):
        for k in range(K):
            cur, ys = k, []
            for t in range(i - 1, -1, -1):
                ys.append(int(tokens[t, b, cur]))
                cur = int(parents[t, b, cur])
            out[b][k] = ys[::-1]
    return out


def step_ref(logits, scores_in, last_tokens, end_id, K, prefixes, c):
    """One constrained step in f64: `beam_reference.beam_step_ref` with the banned columns of every live, unfinished row struck
    from the candidates AFTER the log-softmax over all V columns.  Also returns nbans: how many finite candidates were struck."""
    cand = R.beam_candidates_ref(logits, scores_in, last_tokens, end_id, K)
    B = cand.shape[0]
    V = cand.shape[1] // K
    scores = np.asarray(scores_in, dtype=np.float64).reshape(B, K)
    nbans = 0
    for b in range(B):
        for k in range(K):
            dead = np.isneginf(scores[b, k])
            finished = last_tokens is not None and end_id is not None and end_id >= 0 and \
                int(np.asarray(last_tokens).reshape(B, K)[b, k]) == end_id
            if dead or finished:
                continue
            for v in banned_of(prefixes[b][k], end_id, c):
                if 0 <= v < V:
                    nbans += int(np.isfinite(cand[b, k * V + v]))
                    cand[b, k * V + v] = -np.inf
    order = np.argsort(-cand, axis=1, kind="stable")[:, :K]
    out_scores = np.take_along_axis(cand, order, 1)
    live = np.minimum(np.isfinite(cand).sum(1), K)
    return dict(cand=cand, order=order, scores=out_scores, parent=order // V, token=order % V, live=live, nbans=nbans)


def lengths_ref(ids, end_id):
    """L [B, K]: tokens in front of the first end_id, plus 1 for it; T for a row without one"""
    ids = np.asarray(ids)
    B, K, T = ids.shape
    L = np.full((B, K), T, dtype=np.int64)
    for b in range(B):
        for k in range(K):
            hit = np.nonzero(ids[b, k] == end_id)[0]
            if hit.size:
                L[b, k] = hit[0] + 1
    return L


def rerank_ref(ids, scores, end_id, alpha):
    """-> dict(L, norm [B, K] f64 in the NEW order, order [B, K]: previous rank of the hypothesis now at r, ids, scores re-ordered)"""
    ids, scores = np.asarray(ids), np.asarray(scores, dtype=np.float64)
    L = lengths_ref(ids, end_id)
    norm = scores / np.power(L.astype(np.float64), float(alpha)) if alpha > 0 else scores.copy()
    order = np.argsort(-norm, axis=1, kind="stable")                              # equal norms keep their rank; -inf goes last
    return dict(L=L, norm=np.take_along_axis(norm, order, 1), order=order,
                ids=np.take_along_axis(ids, order[:, :, None], 1), scores=np.take_along_axis(scores, order, 1))


def _select(scores, logits, seqs, last, end_id, c, K):
    """one selection of a whole-decode restatement, in the dtype of `logits` (the f32 expression the device rounds: base + logp).
    -> order [B, K] flat, new scores, gap [B]: the smallest distance between consecutive candidates among the best K + 1, nbans"""
    B = scores.shape[0]
    V = logits.shape[1]
    cand = scores.unsqueeze(2) + torch.log_softmax(logits, dim=1).view(B, K, V)
    nbans = 0
    for b in range(B):
        for k in range(K):
            if scores[b, k] == float("-inf"):
                continue
            if end_id is not None and last is not None and int(last[b, k]) == end_id:
                cand[b, k] = float("-inf")
                cand[b, k, end_id] = scores[b, k]
                continue
            for v in banned_of(seqs[b, k].tolist(), end_id, c):
                nbans += 1
                cand[b, k, v] = float("-inf")
    cand = cand.view(B, K * V)
    sv, si = torch.sort(cand, dim=1, descending=True, stable=True)
    top = sv[:, :K + 1].double()
    gap = torch.full((B,), float("inf"), dtype=torch.float64)
    for b in range(B):
        t = top[b][torch.isfinite(top[b])]
        if t.numel() > 1:
            gap[b] = (t[:-1] - t[1:]).min()
    return si[:, :K], sv[:, :K], gap, nbans


def decoder_beam(params, features, K, num_layers, end_id, c, steps=20):
    """`oracle.decoder.beam_search`'s loop with the constrained selection.  -> dict(ids [B,K,steps], scores [B,K], gap [B],
    nbans), before any length penalty (`rerank_ref` applies that)"""
    from oracle import decoder as OD
    B = features.shape[0]
    V = params["linear.weight"].shape[0]
    dt = features.dtype
    hs = [torch.zeros(B * K, params["lstm.weight_hh_l%d" % l].shape[1], dtype=dt) for l in range(num_layers)]
    cs = [torch.zeros_like(h) for h in hs]
    scores = torch.full((B, K), float("-inf"), dtype=dt)
    scores[:, 0] = 0.0
    x = features.repeat_interleave(K, 0)
    seqs = torch.zeros(B, K, 0, dtype=torch.int64)
    last, gap, nbans = None, torch.full((B,), float("inf"), dtype=torch.float64), 0
    for _ in range(steps):
        inp = x
        for l in range(num_layers):
            xg = inp @ params["lstm.weight_ih_l%d" % l].t() + params["lstm.bias_ih_l%d" % l] + params["lstm.bias_hh_l%d" % l]
            hs[l], cs[l], _ = OD.lstm_cell(xg, hs[l], cs[l], params["lstm.weight_hh_l%d" % l])
            inp = hs[l]
        logits = inp @ params["linear.weight"].t() + params["linear.bias"]
        order, scores, g, nb = _select(scores, logits, seqs, last, end_id, c, K)
        gap, nbans = torch.minimum(gap, g), nbans + nb
        parent, token = order // V, order % V
        rows = (torch.arange(B).unsqueeze(1) * K + parent).reshape(-1)
        hs, cs = [h[rows] for h in hs], [cc[rows] for cc in cs]
        seqs = torch.cat([torch.gather(seqs, 1, parent.unsqueeze(2).expand(B, K, seqs.shape[2])), token.unsqueeze(2)], 2)
        last = token
        x = params["embed.weight"][token.reshape(-1)]
    return dict(ids=seqs, scores=scores, gap=gap, nbans=nbans)


def attend_beam(p, features, K, end_id, c, states=None, start_id=1, steps=20):
    """the beam loop over `oracle.attend`'s step (as tests/alpha_reference.py lays it out) with the constrained selection; the
    attention maps are carried with h and c.  -> dict(ids, scores, alphas [B,K,steps,P], gap, nbans)"""
    from oracle import attend as OA
    B, P = features.shape[0], features.shape[1]
    V, H, dt = p["classifier.weight"].shape[0], p["lstmcell.weight_hh"].shape[1], features.dtype
    feats = features.repeat_interleave(K, 0)
    context_encode = feats @ p["image_att_w"]
    if states is None:
        h, cc = torch.zeros(B * K, H, dtype=dt), torch.zeros(B * K, H, dtype=dt)
    else:
        h, cc = states[0].repeat_interleave(K, 0), states[1].repeat_interleave(K, 0)
    emb = p["embedding.weight"][torch.full((B * K,), start_id, dtype=torch.long)]
    scores = torch.full((B, K), float("-inf"), dtype=dt)
    scores[:, 0] = 0.0
    seqs, maps = torch.zeros(B, K, 0, dtype=torch.int64), torch.zeros(B, K, 0, P, dtype=dt)
    last, rnn_input, gap, nbans = None, None, torch.full((B,), float("inf"), dtype=torch.float64), 0
    for i in range(steps):
        context, alpha = OA.attention_layer(p, feats, context_encode, h)
        if i == 0:
            rnn_input = torch.cat([emb, context], 1)
        h, cc = OA.lstmcell(p, rnn_input, h, cc)
        logits = OA.output_layer(p, context, h)
        order, scores, g, nb = _select(scores, logits, seqs, last, end_id, c, K)
        gap, nbans = torch.minimum(gap, g), nbans + nb
        parent, token = order // V, order % V
        rows = (torch.arange(B).unsqueeze(1) * K + parent).reshape(-1)
        h, cc, context = h[rows], cc[rows], context[rows]
        seqs = torch.cat([torch.gather(seqs, 1, parent.unsqueeze(2).expand(B, K, seqs.shape[2])), token.unsqueeze(2)], 2)
        maps = torch.cat([torch.gather(maps, 1, parent.view(B, K, 1, 1).expand(B, K, maps.shape[2], P)),
                          alpha[rows].view(B, K, 1, P)], 2)
        last = token
        rnn_input = torch.cat([p["embedding.weight"][token.reshape(-1)], context], 1)
    return dict(ids=seqs, scores=scores, alphas=maps, gap=gap, nbans=nbans)


def check_properties(ids, end_id, c):
    """every hypothesis, up to and including its first end_id, obeys the constraints; returns the number of rows checked"""
    ids = np.asarray(ids)
    rows = ids.reshape(-1, ids.shape[-1])
    for row in rows:
        row = row.tolist()
        n = row.index(end_id) + 1 if end_id in row else len(row)
        for i in range(n):
            assert row[i] not in banned_of(row[:i], end_id, c), (row, i)
    return len(rows)
