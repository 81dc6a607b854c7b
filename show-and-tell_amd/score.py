"""Scoring GIVEN captions: the model's log-probability of captions somebody hands it (include/sat_hip.h, "Scoring given captions").

    DecoderRNN.score_captions / ShowAndTell.score_captions      per-caption log p(S | I), paired or the B_img x C cross matrix
    ShowAttendTellModel.score_captions(_features)               paired, from the model's own logits
    retrieval_metrics                                           Recall@K / median rank, image -> sentence and sentence -> image
                                                                (Vinyals et al. 2015, section 4.3.5: ranking by p(S | I))
    rescore                                                     likelihood rerank of K decoded candidates per image

Scored tokens are the rows the training loss averages.  Show-and-Tell (`/root/reference/models.py:47-53`): with the caption as the
data loader gives it (`<start>` ... `<end>`), step t predicts captions[c][t] for t < lengths[c].  Show-Attend-Tell
(`/root/reference/train.py:134-139`): targets captions[:, 1:] with lengths - 1.  Everything stays on the device; nothing is taped."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from .pack import PackInfo, pack_targets

# logp f64 [C] (paired) or [B_img, C] (cross); length i32 [C]; token_logp f32 [..., T] or None (+0.0 beyond a caption's length);
# score = logp ("none") or logp / length ("length")
CaptionScores = namedtuple("CaptionScores", ["logp", "length", "token_logp", "score"])

WORKSPACE_BUDGET = 1 << 30      # bytes one sat_score_captions call may ask for: `cross=True` is chunked over images to stay below


def set_workspace_budget(nbytes):
    """Set the per-call workspace budget of `cross=True` scoring (bytes); returns the previous one.  A budget too small for one
    image still scores one image per call."""
    global WORKSPACE_BUDGET
    nbytes = int(nbytes)
    if nbytes < 1:
        raise ValueError("workspace budget must be positive")
    old, WORKSPACE_BUDGET = WORKSPACE_BUDGET, nbytes
    return old


def _check_normalize(normalize):
    if normalize not in ("none", "length"):
        raise ValueError("normalize must be 'none' or 'length', got %r" % (normalize,))


def _result(logp, length, tokens, normalize):
    score = logp if normalize == "none" else logp / length.to(torch.float64)
    return CaptionScores(logp, length, tokens, score)


def check_captions(captions, lengths, min_length=1):
    """The host checks every scoring entry point starts with (nothing is launched before they pass): captions an i64 matrix on the
    device, one length per row in ANY order, min_length <= length <= captions.shape[1].  Returns (captions, lengths, order):
    `order` lists the rows by length, descending (stable)."""
    L.require_gpu(captions, "captions")
    if captions.dim() != 2:
        raise ValueError("captions must be a matrix [C, T]")
    if captions.dtype != torch.int64 or captions.stride(1) != 1:
        captions = captions.long().contiguous()
    lengths = [int(l) for l in lengths]
    if len(lengths) != captions.shape[0] or not lengths:
        raise ValueError("need one length per caption row")
    if min(lengths) < min_length or max(lengths) > captions.shape[1]:
        raise ValueError("need %d <= every length <= captions.shape[1]" % min_length)
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    return captions, lengths, order


def logits_caption_logp(logits, targets, pi, return_tokens=False):
    """Packed logits f32 [N, V] (time-major, `pi` their PackInfo) and targets i64 [N] -> (logp f64 [B], length i32 [B], token_logp
    f32 [B, T] or None) for the B packed sequences, in the packed (sorted) order: `sat_ce_rows` without a gradient, then
    `sat_caption_logp_sum` (a fixed-order f64 sum per caption).  The logits are left as they are."""
    lib = L.load()
    L.require_gpu(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("logits must be a float32 matrix with contiguous rows")
    N, V = logits.shape
    if N != pi.N or targets.shape[0] != N:
        raise ValueError("logits / targets do not have the packed batch's %d rows" % pi.N)
    dev = logits.device
    row_loss = torch.empty(N, device=dev)
    L.check(lib.sat_ce_rows(logits.data_ptr(), logits.stride(0), targets.data_ptr(), N, V, 1.0, 0, row_loss.data_ptr(), None,
                            L.stream()), "sat_ce_rows")
    nll = torch.empty(pi.B, dtype=torch.float64, device=dev)
    length = torch.empty(pi.B, dtype=torch.int32, device=dev)
    tok = torch.empty(pi.B, pi.T, device=dev) if return_tokens else None
    L.check(lib.sat_caption_logp_sum(row_loss.data_ptr(), pi.prefix_dev.data_ptr(), pi.T, pi.B, nll.data_ptr(), length.data_ptr(),
                                     L.ptr(tok), pi.T if return_tokens else 0, L.stream()), "sat_caption_logp_sum")
    # row_loss = -log p: negation is exact, so -sum(row_loss) is the f64 sum of the log-probabilities in the same order.  The token
    # matrix as 0 - x, not -x: the +0.0 beyond a caption's length stays +0.0
    return -nll, length, (0.0 - tok if return_tokens else None)


def _index_tensor(order, dev):
    return torch.tensor(order, dtype=torch.int64, device=dev)


@torch.no_grad()
def decoder_score_captions(dec, features, captions, lengths, cross=False, normalize="none", return_tokens=False):
    """`DecoderRNN.score_captions` (see there)."""
    from .models import _f32c
    _check_normalize(normalize)
    features = _f32c(features, "features")
    if features.dim() != 2 or features.shape[1] != dec.embed_size:
        raise ValueError("features must be [B_img, embed_size=%d]" % dec.embed_size)
    captions, lengths, order = check_captions(captions, lengths)
    Cn, B_img = len(lengths), features.shape[0]
    if not cross and B_img != Cn:
        raise ValueError("paired scoring needs one feature row per caption (%d rows, %d captions); cross=True scores every pair"
                         % (B_img, Cn))
    lib = L.load()
    dev = features.device
    E, H, V, Lh = dec.embed_size, dec.hidden_size, dec.vocab_size, dec.num_layers
    pi = PackInfo.get([lengths[i] for i in order], dev)              # the captions, longest first
    T = pi.T
    dec.id_guard().submit(captions, T, V, "captions")
    order_dev = _index_tensor(order, dev)
    lstm_w = dec._lstm_ptrs()
    st = L.stream()

    def call(feats, nb, row_image, row_caption, bs_c, prefix_dev, R, N):
        logp = torch.empty(R, dtype=torch.float64, device=dev)
        length = torch.empty(R, dtype=torch.int32, device=dev)
        tok = torch.empty(R, T, device=dev) if return_tokens else None
        need = lib.sat_score_captions_ws_bytes(nb, R, N, E, H, V, Lh)
        if need <= 0:
            raise ValueError("sat_score_captions: unsupported sizes")
        ws, ws_ptr = L.workspace256(need, dev)
        L.check(lib.sat_score_captions(feats.data_ptr(), L.ptr(dec.embed.weight), lstm_w, Lh, L.ptr(dec.linear.weight),
                                       L.ptr(dec.linear.bias), captions.data_ptr(), captions.stride(0), Cn, row_image.data_ptr(),
                                       row_caption.data_ptr(), bs_c, prefix_dev.data_ptr(), T, nb, R, N, E, H, V, logp.data_ptr(),
                                       length.data_ptr(), L.ptr(tok), T if return_tokens else 0, ws_ptr, need, st), "sat_score_captions")
        return logp, length, tok

    order32 = order_dev.to(torch.int32)
    if not cross:
        logp_s, len_s, tok_s = call(features, B_img, order32, order32, pi.bs_c, pi.prefix_dev, Cn, pi.N)
        logp = torch.empty_like(logp_s)
        logp[order_dev] = logp_s
        length = torch.empty_like(len_s)
        length[order_dev] = len_s
        tok = None
        if return_tokens:
            tok = torch.empty_like(tok_s)
            tok[order_dev] = tok_s
        return _result(logp, length, tok, normalize)

    # cross: rows (caption j of the sorted order, image i of the chunk) at r = j * nb + i, so that every step's live rows are a
    # prefix; images per call as many as the workspace budget allows
    nb = B_img
    while nb > 1 and lib.sat_score_captions_ws_bytes(nb, nb * Cn, nb * pi.N, E, H, V, Lh) > WORKSPACE_BUDGET:
        nb -= 1
    logp = torch.empty(B_img, Cn, dtype=torch.float64, device=dev)
    tok = torch.empty(B_img, Cn, T, device=dev) if return_tokens else None
    length = None
    plans = {}
    for b0 in range(0, B_img, nb):
        n = min(nb, B_img - b0)
        plan = plans.get(n)
        if plan is None:
            bs = [n * b for b in pi.batch_sizes]
            prefix = [0]
            for v in bs:
                prefix.append(prefix[-1] + v)
            plan = plans[n] = ((C.c_int32 * T)(*bs), torch.tensor(prefix, dtype=torch.int32, device=dev),
                               torch.arange(n, dtype=torch.int32, device=dev).repeat(Cn),
                               order32.repeat_interleave(n))
        bs_c, prefix_dev, row_image, row_caption = plan
        logp_s, len_s, tok_s = call(features[b0:b0 + n], n, row_image, row_caption, bs_c, prefix_dev, n * Cn, n * pi.N)
        logp[b0:b0 + n, order_dev] = logp_s.view(Cn, n).t()
        if return_tokens:
            tok[b0:b0 + n, order_dev] = tok_s.view(Cn, n, T).transpose(0, 1)
        if length is None:
            length = torch.empty(Cn, dtype=torch.int32, device=dev)
            length[order_dev] = len_s.view(Cn, n)[:, 0]
    return _result(logp, length, tok, normalize)


@torch.no_grad()
def attend_score_captions_features(model, features, fmean, captions, lengths, cross=False, normalize="none", return_tokens=False):
    """`ShowAttendTellModel.score_captions_features` (see there)."""
    _check_normalize(normalize)
    if cross:
        raise NotImplementedError("cross scoring for Show-Attend-Tell: every (image, caption) pair would repeat the attention "
                                  "inputs; score pairs (cross=False)")
    captions, lengths, order = check_captions(captions, lengths, min_length=2)
    if features.shape[0] != len(lengths):
        raise ValueError("paired scoring needs one image per caption")
    dev = captions.device
    order_dev = _index_tensor(order, dev)
    caps_s = captions[order_dev].contiguous()
    sorted_lengths = [lengths[i] for i in order]
    targets, l1 = pack_targets(caps_s, sorted_lengths)
    # like DecoderRNN.score_captions, the score is that of the model's distribution in either mode: dropout and scheduled sampling
    # are training noise and never part of it.  `decode` consults only the model's own flag for both.
    was_training, model.training = model.training, False
    try:
        logits = model.decode(features[order_dev].contiguous(), fmean[order_dev].contiguous(), caps_s, l1)
    finally:
        model.training = was_training
    if not logits.is_contiguous():
        logits = logits.contiguous()
    logp_s, len_s, tok_s = logits_caption_logp(logits, targets, PackInfo.get(l1, dev), return_tokens)
    logp = torch.empty_like(logp_s)
    logp[order_dev] = logp_s
    length = torch.empty_like(len_s)
    length[order_dev] = len_s
    tok = None
    if return_tokens:
        tok = torch.empty_like(tok_s)
        tok[order_dev] = tok_s
    return _result(logp, length, tok, normalize)


def retrieval_metrics(scores, caption_image, ks=(1, 5, 10)):
    """Image-sentence ranking from a score matrix (Vinyals et al. 2015, section 4.3.5).  scores [B_img, C] (larger = better, e.g.
    `score_captions(..., cross=True).score`), caption_image i64 [C]: the image (row) every caption belongs to.
    rank = 1 + (number strictly greater) + (number equal at a smaller index).
      image -> sentence: per image, the rank of its best-ranked own caption among the C captions of its row;
      sentence -> image: per caption, the rank of its image among the B_img images of its column.
    Returns a dict of 0-dim f64 tensors on the scores' device -- "i2s_r@K", "s2i_r@K" for K in ks (fractions in [0, 1]) and
    "i2s_medr", "s2i_medr" (median rank; the mean of the two middle ranks for an even count).  Plain torch ops, no host read.
    Every image needs at least one caption."""
    if scores.dim() != 2 or caption_image.dim() != 1 or caption_image.shape[0] != scores.shape[1]:
        raise ValueError("scores must be [B_img, C] and caption_image [C]")
    B, Cn = scores.shape
    dev = scores.device
    caption_image = caption_image.to(device=dev, dtype=torch.int64)

    def ranks(s, dim):
        order = torch.sort(s, dim=dim, descending=True, stable=True)[1]        # equal scores keep their index order
        shape = [1, 1]
        shape[dim] = s.shape[dim]
        pos = torch.arange(1, s.shape[dim] + 1, device=dev).view(shape).expand_as(s)
        return torch.empty_like(order).scatter_(dim, order, pos)

    own = caption_image.view(1, Cn) == torch.arange(B, device=dev).view(B, 1)
    i2s = torch.where(own, ranks(scores, 1), torch.full((1, 1), Cn + 1, dtype=torch.int64, device=dev)).min(dim=1)[0]
    s2i = ranks(scores, 0).gather(0, caption_image.view(1, Cn)).view(Cn)

    out = {}
    for name, r in (("i2s", i2s), ("s2i", s2i)):
        for k in ks:
            out["%s_r@%d" % (name, k)] = (r <= k).to(torch.float64).mean()
        srt = torch.sort(r)[0].to(torch.float64)
        n = r.shape[0]
        out["%s_medr" % name] = (srt[(n - 1) // 2] + srt[n // 2]) / 2
    return out


def candidate_captions(ids, end_id=2, start_id=1):
    """Decoded candidates ids i64 [R, T] -> (captions i64 [R, T + 1], lengths list) as `score_captions` takes them.
    Convention: a decoded row carries NO `<start>` (`sample`, `sample_beam`, `sample_stochastic` return what follows it), so
    `start_id` is put in front; the row ends with its first `end_id`, which is scored too: length = 1 + min(kept + 1, T) with
    kept = the ids in front of the first `end_id` (`sat_kept_tokens`' rule; T for a row without one).  What follows `<end>` is
    never scored.  The lengths come to the host (one synchronisation): `score_captions` takes them as a Python list."""
    from .evaluate import kept_tokens
    if ids.dim() != 2:
        raise ValueError("ids must be [R, T]")
    ids = ids.long().contiguous()
    R, T = ids.shape
    kept = kept_tokens(ids, end_id)
    lengths = (torch.clamp(kept + 1, max=T) + 1).tolist()
    start = torch.full((R, 1), int(start_id), dtype=torch.int64, device=ids.device)
    return torch.cat([start, ids], dim=1).contiguous(), lengths


@torch.no_grad()
def rescore(model, inputs, ids, end_id=2, normalize="length", start_id=1):
    """Likelihood rerank of K decoded candidates per image: ids i64 [B, K, T] (`sample_beam(return_all=True)`, the beam groups,
    `sample_stochastic(num_samples=K)`), `inputs` what the model's `score_captions` takes first (features for a `DecoderRNN`,
    images otherwise; B rows).  Returns (best i64 [B], score f64 [B, K]): score = the candidate's log-probability under `model`
    ("none") or per token ("length"), best = its arg-max.  The model may be another one than the decoder of the candidates.
    Candidates are turned into captions by `candidate_captions` (`<start>` in front, ended at the first `end_id`).  Only
    `score_captions` computes anything: the B x K pairs are scored as pairs, every input row repeated K times (an image model
    encodes the B images once and scores through its `score_captions_features` / its decoder's `score_captions`)."""
    _check_normalize(normalize)
    if ids.dim() != 3 or ids.shape[0] != inputs.shape[0]:
        raise ValueError("ids must be [B, K, T] with one row of K candidates per input row")
    B, K, T = ids.shape
    caps, lengths = candidate_captions(ids.reshape(B * K, T), end_id, start_id)
    if hasattr(model, "score_captions_features"):                       # Show-Attend-Tell
        feats, fmean = model._encode(inputs)
        res = model.score_captions_features(feats.repeat_interleave(K, 0), fmean.repeat_interleave(K, 0), caps, lengths,
                                            normalize=normalize)
    else:
        dec = getattr(model, "decoder", model)
        feats = model.encoder(inputs) if dec is not model else inputs
        res = dec.score_captions(feats.repeat_interleave(K, 0), caps, lengths, normalize=normalize)
    score = res.score.view(B, K)
    return score.argmax(dim=1), score
