"""The validation half of the reference's `evaluation` (`/root/reference/eval.py:58-122`) for one mini-batch, on the device:

    targets = pack_padded_sequence(captions, lengths)[0]          eval.py:91   sat_pack_tokens (UNSHIFTED captions, FULL lengths)
    outputs = model(images, captions, lengths)                    eval.py:93   the model's own forward (eval mode: running statistics)
    loss = crit(outputs, targets)                                 eval.py:95   sat_ce_rows (no gradient)
    sampled_ids = model.sample(images, state)                     eval.py:99   greedy (or beam) decode
    for word_id in sentence_ids: if word == '<end>': break        eval.py:103-109   sat_kept_tokens: the count per row, on the device

`validation_step` returns device tensors (no host sync); `sentences` is the host-side id -> word join of eval.py:101-110 over
the already truncated rows.

Of `language_eval` (eval.py:15-55) the one number the reference's trainer acts on is here: with a `CiderScorer` (cider.py) and
the batch's `image_index`, `validation_step` also returns CIDEr (`lang_stats['CIDEr']`, train.py:169-177) of the decoded rows,
per caption and as the batch mean, still without a host sync.  With a `BleuScorer` / `RougeLScorer` (langstats.py) it returns
the per-caption Bleu_1..4 (and accumulates the corpus totals) and ROUGE_L the same way.  The reference words must already be
tokenised: the PTB tokenizer, METEOR and SPICE (Java) stay out of scope."""
import torch

from . import _lib as L
from .pack import PackInfo


def pack_validation_targets(captions, lengths):
    """eval.py:91: `pack_padded_sequence(captions, lengths, batch_first=True)[0]` -- captions NOT shifted, lengths NOT
    decremented (unlike train.py:134-135).  Returns (targets i64 [sum(lengths)], PackInfo)."""
    L.require_gpu(captions, "captions")
    if captions.dtype != torch.int64 or captions.stride(1) != 1:
        captions = captions.long().contiguous()
    lengths = [int(l) for l in lengths]
    if len(lengths) != captions.shape[0] or lengths[0] > captions.shape[1] or lengths[-1] < 1:
        raise ValueError("need 1 <= every length <= captions.shape[1], one per row")
    pi = PackInfo.get(lengths, captions.device)
    targets = torch.empty(pi.N, dtype=torch.int64, device=captions.device)
    L.check(L.load().sat_pack_tokens(captions.data_ptr(), captions.stride(0), pi.prefix_dev.data_ptr(), pi.T, pi.N, 0,
                                     targets.data_ptr(), L.stream()), "sat_pack_tokens")
    return targets, pi


def mean_cross_entropy(logits, targets):
    """`nn.CrossEntropyLoss()(outputs, targets)` (eval.py:95) without a gradient: 1-element f32 device tensor."""
    L.require_gpu(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("logits must be a float32 matrix with contiguous rows")
    N, V = logits.shape
    if targets.shape[0] != N:
        raise ValueError("targets has %d rows, logits %d" % (targets.shape[0], N))
    row_loss = torch.empty(N, device=logits.device)
    loss = torch.zeros(1, device=logits.device)
    L.check(L.load().sat_ce_rows(logits.data_ptr(), logits.stride(0), targets.data_ptr(), N, V, 1.0 / N, 0, row_loss.data_ptr(),
                                 loss.data_ptr(), L.stream()), "sat_ce_rows")
    return loss


def kept_tokens(ids, end_id):
    """eval.py:103-109: per row, the number of ids in front of the first `end_id` (the row length when there is none):
    i32 [B] on the device."""
    L.require_gpu(ids, "ids")
    if ids.dim() != 2 or ids.dtype != torch.int64 or ids.stride(1) != 1:
        raise TypeError("ids must be an int64 matrix with contiguous rows")
    kept = torch.empty(ids.shape[0], dtype=torch.int32, device=ids.device)
    L.check(L.load().sat_kept_tokens(ids.data_ptr(), ids.stride(0), ids.shape[0], ids.shape[1], int(end_id), kept.data_ptr(),
                                     L.stream()), "sat_kept_tokens")
    return kept


@torch.no_grad()
def validation_step(model, images, captions, lengths, state=None, end_id=2, beam_size=1, scorer=None, image_index=None,
                    bleu=None, rouge=None, *, suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False,
                    length_penalty=0.0, num_beam_groups=1, diversity_penalty=0.0, consensus=None, caption_logp=False):
    """One iteration of the loop body eval.py:71-118 (the caller has put the model in eval mode, eval.py:65).
    Returns dict(loss f32[1], ids i64[B,20], kept i32[B]) -- all on the device, nothing synchronised.  With a `CiderScorer`
    and `image_index` (the corpus image of every row) the dict gains cider f64[1] and cider_scores f64[B] of `ids`; with a
    `BleuScorer` as `bleu`, bleu_scores f64[B,4] (and `bleu.update` has run on the rows: `bleu.compute()` after the last batch
    is the corpus Bleu_1..4); with a `RougeLScorer` as `rouge`, rouge_l f64[1] and rouge_l_scores f64[B].
    The keyword-only beam constraints (`sample_beam`'s; all off by default) go to the beam decode: with any of them on the
    decode is `sample_beam` also at beam_size=1 -- the constrained greedy decode -- which starts from the zero state.
    num_beam_groups / diversity_penalty (`sample_beam`'s diverse beam search; one group by default) go there too.
    consensus: a `ConsensusReranker` (consensus.py).  With one and beam_size > 1 the decoded `ids` are the consensus pick of the
    beam_size hypotheses (equal weights; the reranker's end_id must be `end_id`) instead of the likelihood winner, and the dict
    gains consensus_best i64[B] and consensus_utility f64[B,beam_size]; with beam_size == 1 there is nothing to pick from:
    ValueError.
    caption_logp: also caption_logp f64[B], the log-probability of every given caption (the sum over its rows of the packed
    logits `loss` averages, `score.logits_caption_logp`), and caption_token_count i32[B], the rows it sums: the token-weighted
    mean of -caption_logp is `loss`.  Off (the default): the calls and the keys are what they were."""
    from .models import check_beam_constraints, check_beam_groups
    cons = dict(suppress_ids=suppress_ids, min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size,
                block_repeat=block_repeat, length_penalty=length_penalty)
    constraints = cons if check_beam_constraints(end_id=end_id, **cons).active else {}
    if check_beam_groups(beam_size, num_beam_groups, diversity_penalty)[0] > 1:
        constraints = dict(constraints, num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty)
    if bleu is None and rouge is None:
        if (scorer is None) != (image_index is None):
            raise ValueError("scorer and image_index go together")
    elif image_index is None:
        raise ValueError("bleu and rouge need image_index, the corpus image of every row")
    if consensus is not None:
        if beam_size <= 1:
            raise ValueError("consensus reranking needs beam_size > 1: one hypothesis per image leaves nothing to pick from")
        if consensus.end_id != end_id:
            raise ValueError("the reranker ends rows at id %d, validation_step at %d" % (consensus.end_id, end_id))
    if model.training:
        raise RuntimeError("validation_step expects model.eval() (eval.py:65)")
    targets, pi = pack_validation_targets(captions, lengths)
    outputs = model(images, captions, lengths)                          # eval.py:93
    if not outputs.is_contiguous():
        outputs = outputs.contiguous()
    loss = mean_cross_entropy(outputs, targets)                         # eval.py:95
    if beam_size > 1 or constraints:
        if constraints and state is not None:
            raise ValueError("the constrained decode is `sample_beam`, which takes no initial state")
        if consensus is not None:
            ids = consensus.decode(model, images, beam_size=beam_size, **constraints)
        else:
            ids = model.sample_beam(images, beam_size=beam_size, end_id=end_id, **constraints)
    else:
        ids = model.sample(images, state)                               # eval.py:99
        if ids.dim() == 1:                                              # squeezed at batch 1 (models.py:67): one row
            ids = ids.view(1, -1)
    out = {"loss": loss, "ids": ids, "kept": kept_tokens(ids, end_id)}
    if caption_logp:
        from .score import logits_caption_logp
        out["caption_logp"], out["caption_token_count"], _ = logits_caption_logp(outputs, targets, pi)
    if consensus is not None:
        out["consensus_best"], out["consensus_utility"] = consensus.last_best, consensus.last_utility
    if scorer is not None:
        out["cider"], out["cider_scores"] = scorer.score(ids, image_index, end_id=end_id, kept=out["kept"])
    if bleu is not None:
        out["bleu_scores"] = bleu.update(ids, image_index, end_id=end_id, kept=out["kept"])
    if rouge is not None:
        out["rouge_l"], out["rouge_l_scores"] = rouge.score(ids, image_index, end_id=end_id, kept=out["kept"])
    return out


def sentences(ids, kept, idx2word):
    """eval.py:101-110 on the host: `' '.join(words in front of '<end>')` per row.  ids / kept: tensors (any device) or lists."""
    ids = ids.tolist() if hasattr(ids, "tolist") else ids
    kept = kept.tolist() if hasattr(kept, "tolist") else kept
    return [" ".join(idx2word[w] for w in row[:n]) for row, n in zip(ids, kept)]
