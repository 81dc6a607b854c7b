"""Plain references of the diverse beam search (sat_beam_step_groups, sat_beam_decode_groups and the `num_beam_groups` /
`diversity_penalty` keywords): numpy / torch on the CPU, one obvious line per rule, nothing shared with the code under test.

The K slots of an image are G groups of Kg = K / G; slots g*Kg .. g*Kg + Kg - 1 are group g, and a hypothesis never leaves its
group.  At one step the groups select in order.  Group g's candidates are the (k, v) with k in group g, s(k, v) the raw score of
the plain step (base + log_softmax over all V columns, banned columns struck); its key is s - lambda * n(v), where n(v) is how
many slots of the groups in front chose v AT THIS STEP and count: a live, unfinished winner counts, once per slot; a finished
row's repeated end_id and a surplus slot do not.  A finished row's one candidate is not penalised.  The Kg best keys win under
(key descending, flat index k*V+v ascending); the carried score is the raw s, never the key.  Surplus slots of a group with fewer
than Kg candidates hold -inf, parent g*Kg, token 0.

`step_ref` sorts the full Kg*V keys of every group: no shortcut through per-row lists."""
import numpy as np
import torch

import beam_constraints_reference as BC
import beam_reference as R


def group_start(B, K, G, dtype=torch.float32):
    """the scores a grouped search starts from: the first slot of every group live at 0, the others dead"""
    s = torch.full((B, K), float("-inf"), dtype=dtype)
    s[:, ::K // G] = 0.0
    return s


def select_groups(cand, finished, G, lam):
    """cand [K, V]: the raw candidate scores of ONE image (any float dtype; -inf: no candidate), finished [K] bools.  The keys are
    formed in cand's dtype as one multiply and one subtract.  -> dict(parent, token [K], scores [K] raw, keys: per group the best
    Kg + 1 keys, npen: winners that carried a penalty, counted: the tokens that counted, in slot order)"""
    K, V = cand.shape
    Kg = K // G
    assert Kg * G == K
    lam = np.asarray(lam, dtype=cand.dtype)
    parent, token = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    scores = np.full(K, -np.inf, dtype=cand.dtype)
    counted, keys, npen = [], [], 0
    for g in range(G):
        n = np.zeros(V, dtype=cand.dtype)
        for v in counted:
            n[v] += 1
        rows = slice(g * Kg, (g + 1) * Kg)
        s = cand[rows]
        key = np.where((n[None, :] > 0) & ~np.asarray(finished[rows], dtype=bool)[:, None], s - lam * n[None, :], s).reshape(-1)
        order = np.argsort(-key, kind="stable")
        keys.append(key[order[:Kg + 1]])
        new = []
        for r in range(Kg):
            at, slot = int(order[r]), g * Kg + r
            if not np.isfinite(key[at]):                              # surplus: fewer than Kg candidates in this group
                parent[slot], token[slot] = g * Kg, 0
                continue
            k, v = g * Kg + at // V, at % V
            parent[slot], token[slot], scores[slot] = k, v, s.reshape(-1)[at]
            if not finished[k]:
                new.append(v)
                npen += int(n[v] > 0)
        counted += new                                                # the group's own tokens do not penalise each other
    return dict(parent=parent, token=token, scores=scores, keys=keys, npen=npen, counted=counted)


def key_gap(keys):
    """the smallest distance between consecutive finite keys among each group's best Kg + 1"""
    gap = np.inf
    for k in keys:
        k = np.asarray(k, dtype=np.float64)
        k = k[np.isfinite(k)]
        if k.size > 1:
            gap = min(gap, float((k[:-1] - k[1:]).min()))
    return gap


def step_ref(logits, scores_in, last_tokens, end_id, K, G, lam, prefixes=None, c=None):
    """One grouped step in f64 (lambda as the f32 the device is handed).  logits [B*K, V], scores_in [B, K], last_tokens [B, K] or
    None; with a `Constraints` c the banned columns of every row (prefixes[b][k]) are struck first.
    -> dict(parent, token [B, K], scores [B, K] f64, live [B, G], gap [B], npen, counted [B] lists)"""
    if c is not None:
        cand = BC.step_ref(logits, scores_in, last_tokens, end_id, K, prefixes, c)["cand"]
    else:
        cand = R.beam_candidates_ref(logits, scores_in, last_tokens, end_id, K)
    B = cand.shape[0]
    V = cand.shape[1] // K
    fin = np.zeros((B, K), dtype=bool)
    if last_tokens is not None and end_id is not None and end_id >= 0:
        fin = np.asarray(last_tokens).reshape(B, K) == end_id
    lam = float(np.float32(lam))
    out = [select_groups(cand[b].reshape(K, V), fin[b], G, lam) for b in range(B)]
    Kg = K // G
    scores = np.stack([o["scores"] for o in out])
    return dict(parent=np.stack([o["parent"] for o in out]), token=np.stack([o["token"] for o in out]), scores=scores,
                live=np.isfinite(scores).reshape(B, G, Kg).sum(2), gap=np.array([key_gap(o["keys"]) for o in out]),
                npen=sum(o["npen"] for o in out), counted=[o["counted"] for o in out])


def _grouped(loop, G, lam, *args, **kw):
    """run one of tests/beam_constraints_reference.py's whole-decode loops with the grouped selection in place of its `_select`:
    the candidates in the dtype of the logits (the f32 expression the device rounds), the key as one f32 multiply and subtract"""
    stats = dict(npen=0)

    def select(scores, logits, seqs, last, end_id, c, K_):
        B, V = scores.shape[0], logits.shape[1]
        if seqs.shape[2] == 0:
            scores = group_start(B, K_, G, scores.dtype)
        cand = scores.unsqueeze(2) + torch.log_softmax(logits, dim=1).view(B, K_, V)
        fin = torch.zeros(B, K_, dtype=torch.bool)
        nbans = 0
        for b in range(B):
            for k in range(K_):
                if scores[b, k] == float("-inf"):
                    cand[b, k] = float("-inf")
                    continue
                if end_id is not None and last is not None and int(last[b, k]) == end_id:
                    fin[b, k] = True
                    cand[b, k] = float("-inf")
                    cand[b, k, end_id] = scores[b, k]
                    continue
                for v in BC.banned_of(seqs[b, k].tolist(), end_id, c):
                    nbans += 1
                    cand[b, k, v] = float("-inf")
        order = torch.zeros(B, K_, dtype=torch.int64)
        new = torch.empty(B, K_, dtype=scores.dtype)
        gap = torch.full((B,), float("inf"), dtype=torch.float64)
        for b in range(B):
            o = select_groups(cand[b].numpy(), fin[b].numpy(), G, np.float32(lam))
            order[b] = torch.from_numpy(o["parent"] * V + o["token"])
            new[b] = torch.from_numpy(o["scores"])
            gap[b] = key_gap(o["keys"])
            stats["npen"] += o["npen"]
        return order, new, gap, nbans

    old = BC._select
    BC._select = select
    try:
        out = loop(*args, **kw)
    finally:
        BC._select = old
    out["npen"] = stats["npen"]
    return out


def decoder_beam(params, features, K, G, lam, num_layers, end_id, c=None, steps=20):
    """the grouped search over `beam_constraints_reference.decoder_beam`'s loop, in SEARCH order (slot = group * Kg + rank).
    -> dict(ids [B,K,steps], scores [B,K], gap [B], nbans, npen)"""
    return _grouped(BC.decoder_beam, G, lam, params, features, K, num_layers, end_id, c or BC.Constraints(), steps=steps)


def attend_beam(p, features, K, G, lam, end_id, c=None, states=None, start_id=1, steps=20):
    """... over `beam_constraints_reference.attend_beam`'s loop.  -> dict(ids, scores, alphas [B,K,steps,P], gap, nbans, npen)"""
    return _grouped(BC.attend_beam, G, lam, p, features, K, end_id, c or BC.Constraints(), states=states, start_id=start_id,
                    steps=steps)


def distinct_captions(ids, scores, end_id):
    """mean number of distinct captions per image among the live hypotheses, each cut behind its first end_id"""
    ids, scores = np.asarray(ids), np.asarray(scores)
    total = 0
    for b in range(ids.shape[0]):
        seen = set()
        for k in range(ids.shape[1]):
            if np.isfinite(scores[b, k]):
                row = ids[b, k].tolist()
                seen.add(tuple(row[:row.index(end_id) + 1] if end_id in row else row))
        total += len(seen)
    return total / ids.shape[0]
