"""numpy restatement of the dropout masks (include/sat_hip.h, `sat_dropout_f32`), built on `ss_reference.philox4x32_10`, and two CPU
references in float64 torch autograd that take the masks as inputs: the Show-and-Tell decoder as nn.LSTM layers run one at a time
on PackedSequence data (a mask between the layers and in front of the linear layer), and the Show-Attend-Tell decoder as the time
loop of `oracle.attend.attend_forward` with the two lines of `output_layer` written out (the mask in front of the classifier).
A plain helper module (like ss_reference.py); nothing here reads the reference project."""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence

import ss_reference as R
from oracle import attend as OA


def threshold(p):
    """thr = lrint(p * 2^24) of the float32 p the kernel receives (round half to even, like lrint's default mode)"""
    return int(np.rint(np.float64(np.float32(p)) * 16777216.0))


def scale(p):
    """(float)(1.0 / (1.0 - (double)p))"""
    return np.float32(1.0 / (1.0 - np.float64(np.float32(p))))


def keep(seed, rank, site, rows, cols, p):
    """keep(r, j) for r < rows, j < cols: bool [rows, cols].  Element (r, j) reads word j & 3 of counter
    (j >> 2, r, 0x80000000 | site, 2 * rank) under key (seed lo, seed hi) and is kept iff (word >> 8) >= thr."""
    k0, k1 = R.seed_key(seed)
    j = np.arange(cols, dtype=np.uint32)[None, :]
    r = np.arange(rows, dtype=np.uint32)[:, None]
    words = R.philox4x32_10(j >> np.uint32(2), r, np.uint32(0x80000000 | int(site)), np.uint32(2 * int(rank)), k0, k1)
    word = np.choose(np.broadcast_to(j & np.uint32(3), (rows, cols)), words)
    return (word >> np.uint32(8)) >= np.uint32(threshold(p))


def apply(x, p, seed, rank, site):
    """y = keep ? x * scale : 0 on a float32 [rows, cols] array, the product one float32 multiply: the kernel's bits"""
    x = np.asarray(x, dtype=np.float32)
    return np.where(keep(seed, rank, site, x.shape[0], x.shape[1], p), x * scale(p), np.float32(0)).astype(np.float32)


def multiplier(seed, rank, site, rows, cols, p):
    """keep * scale as a float64 torch tensor [rows, cols]: what the references multiply an activation with (all ones for p = 0)"""
    return torch.from_numpy(keep(seed, rank, site, rows, cols, p).astype(np.float64) * np.float64(scale(p)))


# ------------------------------------------------------------------------------------------------------ Show-and-Tell
def decoder_masks(seed, rank, N, H, num_layers, p_out, p_lstm):
    """the multipliers of one `DecoderRNN` forward, by site: l + 1 for the output of layer l (p_lstm; the top layer's: p_out)"""
    return {l + 1: multiplier(seed, rank, l + 1, N, H, p_out if l == num_layers - 1 else p_lstm) for l in range(num_layers)}


def decoder_loss_and_grads(params, features, captions_in, lengths, targets, num_layers, masks):
    """models.py:47-54 + mean CE in float64 autograd: nn.LSTM layers one at a time on the packed rows, the output of layer l
    multiplied by masks[l + 1] [N, H].  captions_in [B, >= T-1] (train.py's captions[:, :-1]), lengths the decoder's (features
    count as step 0).  Returns dict(loss, logits, grads by parameter name, d_features, tapes: the dropped outputs by site)."""
    q = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    f = features.detach().double().clone().requires_grad_(True)
    T = int(lengths[0])
    x = torch.cat((f.unsqueeze(1), q["embed.weight"][captions_in[:, :T - 1]]), 1)
    packed = pack_padded_sequence(x, [int(l) for l in lengths], batch_first=True)
    data, bs = packed.data, packed.batch_sizes
    tapes, mods = {}, []
    for l in range(num_layers):
        H = q["lstm.weight_hh_l%d" % l].shape[1]
        lstm = torch.nn.LSTM(data.shape[1], H, 1).double()
        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            getattr(lstm, n + "_l0").data.copy_(q["lstm.%s_l%d" % (n, l)].data)
        mods.append(lstm)
        out, _ = lstm(PackedSequence(data, bs))
        data = tapes[l + 1] = out.data * masks[l + 1]
    logits = data @ q["linear.weight"].t() + q["linear.bias"]
    loss = F.cross_entropy(logits, targets)
    loss.backward()
    grads = {k: v.grad for k, v in q.items() if not k.startswith("lstm.")}
    for l, lstm in enumerate(mods):
        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            grads["lstm.%s_l%d" % (n, l)] = getattr(lstm, n + "_l0").grad
    return dict(loss=loss.detach(), logits=logits.detach(), grads=grads, d_features=f.grad,
                tapes={k: v.detach() for k, v in tapes.items()})


# ------------------------------------------------------------------------------------------------------ Show-Attend-Tell
def attend_loss_and_grads(params, features, captions_in, lengths, targets, mask, alpha_c=0.0):
    """model2.py:38-65 + mean CE (+ alpha_c * mean_{b,p} (1 - sum_t alpha[b,t,p])^2) in float64 autograd, the output layer's
    z = context2out(ctx) + hidden2tout(h) multiplied by its rows of mask [N, E] in front of the classifier.
    Returns dict(loss, ce, penalty, logits, grads, alphas [N, P])."""
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    features = features.double()
    B = features.shape[0]
    emb = p["embedding.weight"][captions_in]
    context_encode = features @ p["image_att_w"]
    h, c = OA.init_lstm(p, features)
    outs, alphas, r0 = [], [], 0
    for t, bs in enumerate(OA.batch_sizes(lengths)):
        context, alpha = OA.attention_layer(p, features[:bs], context_encode[:bs], h[:bs])
        h, c = OA.lstmcell(p, torch.cat([emb[:bs, t], context], 1), h[:bs], c[:bs])
        z = context @ p["context2out.weight"].t() + p["context2out.bias"] + h @ p["hidden2tout.weight"].t() + p["hidden2tout.bias"]
        z = z * mask[r0:r0 + bs]
        outs.append(z @ p["classifier.weight"].t() + p["classifier.bias"])
        alphas.append(alpha)
        r0 += bs
    logits = torch.cat(outs, 0)
    ce = F.cross_entropy(logits, targets)
    cov = sum(F.pad(a, (0, 0, 0, B - a.shape[0])) for a in alphas)
    pen = alpha_c * ((1.0 - cov) ** 2).mean() if alpha_c else torch.zeros((), dtype=torch.float64)
    loss = ce + pen
    loss.backward()
    return dict(loss=loss.detach(), ce=ce.detach(), penalty=pen.detach(), logits=logits.detach(),
                grads={k: v.grad for k, v in p.items()}, alphas=torch.cat(alphas, 0).detach())
