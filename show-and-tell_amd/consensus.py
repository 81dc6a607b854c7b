"""Consensus (minimum-Bayes-risk) reranking of decoded candidates by pairwise CIDEr on the device: the step between "K captions per
image" (`sample_beam(return_all=True)`, diverse beam groups, `sample_stochastic(num_samples=S)`) and "the caption" for images
that have no reference captions.  Every candidate is scored against the OTHER candidates of its image with the corpus's document
frequencies, and the one the rest agree with most is kept.

    scorer = sat.CiderScorer(refs)                         # once: the corpus gives the document frequencies
    rr = sat.ConsensusReranker(scorer, end_id=2)
    ids = rr.decode(model, images, beam_size=5, num_beam_groups=5, diversity_penalty=0.5)     # [B, 20]: the consensus pick
    best, utility = rr.rerank(cands)                       # or: any int64 [B, K, T] device tensor of candidates

The arithmetic is stated at `sat_consensus_rerank` in include/sat_hip.h; the kernels are csrc/sat_cider.hip.  There is no CPU
path.  Out of scope: `Ensemble` as the model of `decode`, the attention maps (`return_alphas`) of the picked hypothesis, BLEU or
ROUGE-L as the utility, and a consensus pick as a self-critical baseline."""
import ctypes as C

import torch

from . import _lib as L
from .cider import MAX_HYP_TOKENS, CiderScorer
from .evaluate import kept_tokens

MAX_CANDIDATES = 64


class ConsensusReranker:
    """scorer: a `CiderScorer`; its table, document frequencies and sigma are used as they are (its references are not read)."""

    def __init__(self, scorer, end_id=2):
        if not isinstance(scorer, CiderScorer):
            raise TypeError("scorer must be a CiderScorer, got %s" % type(scorer).__name__)
        self.scorer, self.end_id = scorer, int(end_id)
        self.last_ids = self.last_scores = self.last_kept = self.last_best = self.last_utility = None

    def rerank(self, ids, kept=None, weights=None, return_pairwise=False):
        """ids: int64 [B, K, T] on the device with stride(2) == 1 (a view of a larger buffer works: the strides are passed through),
        or [K, T] for one image; K <= 64, T <= 64.  Candidate (b, i) ends at kept[b, i] (i32 [B, K] or [B*K] on the device) or,
        without `kept`, in front of its first end_id.  weights: f32 / f64 [B, K] on the device, finite and >= 0 (not checked): the
        weight of candidate j as a reference; None weighs them equally.
        Returns (best i64 [B], utility f64 [B, K]) and, with return_pairwise, pair f64 [B, K, K] (row i: candidate i against every
        other, the diagonal 0).  Everything stays on the device; nothing is synchronised."""
        if ids.dim() == 2:
            ids = ids.unsqueeze(0)
        if ids.dim() != 3 or ids.dtype != torch.int64 or ids.stride(2) != 1:
            raise TypeError("ids must be an int64 [B, K, T] tensor with contiguous rows")
        B, K, T = ids.shape
        if B < 1 or K < 1 or T < 1:
            raise ValueError("ids is empty")
        if K > MAX_CANDIDATES:
            raise ValueError("%d candidates per image; at most %d are supported" % (K, MAX_CANDIDATES))
        if T > MAX_HYP_TOKENS:
            raise ValueError("rows of %d tokens; at most %d are supported" % (T, MAX_HYP_TOKENS))
        cand_stride = ids.stride(1) if K > 1 else T
        image_stride = ids.stride(0) if B > 1 else K * cand_stride
        if cand_stride < T or image_stride < K * cand_stride:
            raise ValueError("ids strides %s: candidates overlap" % (tuple(ids.stride()),))
        if kept is not None and (kept.dtype != torch.int32 or tuple(kept.shape) not in ((B, K), (B * K,))):
            raise TypeError("kept must be an int32 [B, K] or [B*K] tensor")
        if weights is not None:
            if weights.dtype not in (torch.float32, torch.float64):
                raise TypeError("weights must be float32 or float64")
            if tuple(weights.shape) != (B, K):
                raise ValueError("weights must be [B, K] = [%d, %d], got %s" % (B, K, tuple(weights.shape)))
        dev = ids.device
        for t, name in ((ids, "ids"), (kept, "kept"), (weights, "weights")):
            if t is not None:
                L.require_gpu(t, name)
                if t.device != self.scorer.table_keys.device:
                    raise ValueError("%s is on %s, the corpus on %s" % (name, t.device, self.scorer.table_keys.device))
        kept = kept.contiguous() if kept is not None else None
        weights = weights.double().contiguous() if weights is not None else None          # f32 -> f64 is exact
        with torch.cuda.device(dev):
            lib = L.load()
            utility = torch.empty(B, K, dtype=torch.float64, device=dev)
            best = torch.empty(B, dtype=torch.int64, device=dev)
            pair = torch.empty(B, K, K, dtype=torch.float64, device=dev) if return_pairwise else None
            wsb = lib.sat_consensus_ws_bytes(B, K)
            ws, ws_ptr = L.workspace256(wsb, dev)
            L.check(lib.sat_consensus_rerank(C.byref(self.scorer._corpus), ids.data_ptr(), image_stride, cand_stride, B, K, T,
                                             L.ptr(kept), self.end_id, self.scorer.sigma, L.ptr(weights), utility.data_ptr(),
                                             best.data_ptr(), L.ptr(pair), ws_ptr, wsb, L.stream()), "sat_consensus_rerank")
        return (best, utility, pair) if return_pairwise else (best, utility)

    @staticmethod
    def select(ids, best):
        """the picked rows: ids [B, K, T], best i64 [B] -> [B, T] (a gather; no sync)"""
        if ids.dim() != 3 or best.dim() != 1 or best.shape[0] != ids.shape[0]:
            raise ValueError("select takes ids [B, K, T] and best [B]")
        return ids.gather(1, best.view(-1, 1, 1).expand(-1, 1, ids.shape[2])).squeeze(1)

    def _pick(self, ids, scores, weights):
        B, K, T = ids.shape
        kept = kept_tokens(ids.reshape(B * K, T), self.end_id).view(B, K)
        best, utility = self.rerank(ids, kept=kept, weights=weights)
        self.last_ids, self.last_scores, self.last_kept, self.last_best, self.last_utility = ids, scores, kept, best, utility
        return self.select(ids, best)

    @torch.no_grad()
    def decode(self, model, inputs, beam_size=5, weights=None, **beam_kw):
        """`model.sample_beam(inputs, beam_size, end_id=self.end_id, return_all=True, **beam_kw)` (a `ShowAndTell` or
        `ShowAttendTellModel` with images, a `DecoderRNN` with features), then `kept_tokens`, `rerank` and `select`: ids
        [B, steps], the consensus pick of the K beam hypotheses.  weights: None, a [B, K] tensor, or "scores" for
        softmax(scores.double(), 1) of the returned beam scores.  Leaves last_ids [B, K, steps], last_scores [B, K], last_kept,
        last_best and last_utility."""
        if isinstance(weights, str) and weights != "scores":
            raise ValueError('weights must be None, a [B, K] tensor or "scores", got %r' % (weights,))
        if int(beam_size) < 2:
            raise ValueError("a consensus needs beam_size > 1, got %r" % (beam_size,))
        if "return_all" in beam_kw or "end_id" in beam_kw or "return_alphas" in beam_kw:
            raise ValueError("decode sets return_all and end_id itself; return_alphas of the picked hypothesis is not supported")
        ids, scores = model.sample_beam(inputs, int(beam_size), end_id=self.end_id, return_all=True, **beam_kw)
        if isinstance(weights, str):
            weights = torch.softmax(scores.double(), 1)
        return self._pick(ids, scores, weights)

    @torch.no_grad()
    def decode_samples(self, model, inputs, num_samples, **sample_kw):
        """the same over `model.sample_stochastic(inputs, num_samples=S, **sample_kw)`: the consensus pick of S draws per image,
        equally weighted.  last_scores is None.  sample_kw also carries the constraints of `sample_stochastic` (suppress_ids,
        min_length with end_id, no_repeat_ngram_size, block_repeat, repetition_penalty): the candidates then hold no <unk>, no
        stutter and no two-token captions before the reranker sees them."""
        if int(num_samples) < 2:
            raise ValueError("a consensus needs num_samples > 1, got %r" % (num_samples,))
        if sample_kw.get("return_logprobs") or sample_kw.get("return_logits"):
            raise ValueError("decode_samples returns the picked ids only")
        ids = model.sample_stochastic(inputs, num_samples=int(num_samples), **sample_kw)
        return self._pick(ids, None, None)
