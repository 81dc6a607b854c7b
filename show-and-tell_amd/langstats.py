"""BLEU-1..4 and ROUGE-L on the device, beside CIDEr: the other plain-arithmetic entries of the reference's `lang_stats`
(`language_eval`, eval.py:17-56; pycocoevalcap/eval.py:39-45) for token-id captions, without a host read.

    cider = sat.CiderScorer(refs)                                    # refs: nested id lists (see `encode_references`)
    bleu, rouge = sat.BleuScorer.from_scorer(cider), sat.RougeLScorer.from_scorer(cider)     # the corpus already on the device
    for batch: bleu.update(ids, image_index, kept=kept); ...         # per-image Bleu_1..4 back, corpus totals accumulate
    bleu.compute()                                                   # f64 [4] on the device: Bleu_1..Bleu_4 of the corpus
    mean, scores = rouge.score(ids, image_index, kept=kept)          # ROUGE_L, batch mean and per caption

`score(ids, image_index, end_id=, kept=) -> (mean, scores)` is the shape `SelfCritical` takes a reward in, and `MixedReward`
adds several up: `SelfCritical(sat.MixedReward([(cider, 1.0), (bleu, 0.5)]))` (Rennie et al. 2017, section 5).

The arithmetic is stated at `sat_bleu_comps` / `sat_rouge_l_score` in include/sat_hip.h; the kernels are csrc/sat_langstats.hip.
BLEU is `BleuScorer.compute_score(option='closest')` (pycocoevalcap/bleu/bleu_scorer.py), ROUGE-L is `Rouge.calc_score`
(pycocoevalcap/rouge/rouge.py).  Captions are ids in the extended id space of cider.py.  There is no CPU path.  METEOR and SPICE
(Java) and the PTB tokenizer stay out; skipping an image that comes twice (eval.py:113-116) is the caller's business."""
import ctypes as C
import math

import torch

from . import _lib as L
from .cider import MAX_HYP_TOKENS, CiderScorer, _dev, flatten_references

ORDERS = 4
COMPS = 10          # testlen, reflen, guess[4], correct[4]


class _RefCorpus:
    """The flat reference corpus on the device (`struct sat_ref_corpus`) and the host checks of a batch of rows."""

    def _build(self, refs, device):
        tokens, ref_off, img_off = flatten_references(refs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("show-and-tell_amd: the reference corpus lives on the MI355X; the HIP path has no CPU fallback")
        self.ref_tokens, self.ref_offsets, self.image_offsets = (_dev(a, self.device) for a in (tokens, ref_off, img_off))
        self._bind(len(tokens), max(1, int((ref_off[1:] - ref_off[:-1]).max())))

    def _share(self, other):
        """the corpus arrays of another scorer (a `CiderScorer` or one of this module's), not copied"""
        for name in ("ref_tokens", "ref_offsets", "image_offsets", "_corpus"):
            if not hasattr(other, name):
                raise TypeError("from_scorer takes a CiderScorer, BleuScorer or RougeLScorer, got %r" % (type(other).__name__,))
        self.device = other.ref_tokens.device
        self.ref_tokens, self.ref_offsets, self.image_offsets = other.ref_tokens, other.ref_offsets, other.image_offsets
        self._bind(int(other._corpus.n_tokens), int(other._corpus.max_ref_tokens))

    def _bind(self, n_tokens, max_ref_tokens):
        self.n_refs, self.n_images = self.ref_offsets.numel() - 1, self.image_offsets.numel() - 1
        self._corpus = L.SatRefCorpus(ref_tokens=self.ref_tokens.data_ptr(), ref_offsets=self.ref_offsets.data_ptr(),
                                      image_offsets=self.image_offsets.data_ptr(), n_tokens=n_tokens, n_refs=self.n_refs,
                                      n_images=self.n_images, max_ref_tokens=max_ref_tokens, reserved=0)

    _image_index = CiderScorer._image_index           # the same rule and the same words for every scorer

    def _rows(self, ids, image_index, kept):
        """`CiderScorer.score`'s checks: (ids [B, T], stride, B, T, image index i32 [B] on the device)"""
        L.require_gpu(ids, "ids")
        if ids.dim() == 1:
            ids = ids.view(1, -1)
        if ids.dim() != 2 or ids.dtype != torch.int64 or ids.stride(1) != 1:
            raise TypeError("ids must be an int64 matrix with contiguous rows")
        if ids.device != self.ref_tokens.device:
            raise ValueError("ids are on %s, the corpus on %s" % (ids.device, self.ref_tokens.device))
        B, T = ids.shape
        if B < 1 or T < 1:
            raise ValueError("ids is empty")
        if T > MAX_HYP_TOKENS:
            raise ValueError("rows of %d tokens; at most %d are supported" % (T, MAX_HYP_TOKENS))
        if kept is not None:
            L.require_gpu(kept, "kept")
            if kept.dtype != torch.int32 or kept.dim() != 1 or kept.numel() != B or not kept.is_contiguous():
                raise TypeError("kept must be a contiguous int32 vector with one entry per row")
        return ids, (ids.stride(0) if B > 1 else T), B, T, self._image_index(image_index, B)


class BleuScorer(_RefCorpus):
    """refs: per image, a list of reference captions, each a list of int ids in [0, 2**31) (see `encode_references`).
    `score` is the per-sentence BLEU of a batch; `update` / `compute` / `reset` accumulate the corpus-level Bleu_1..4 in ten
    int64 totals on the device."""

    def __init__(self, refs, n=4, device="cuda"):
        self._params(n)
        self._build(refs, device)
        self._state()

    @classmethod
    def from_scorer(cls, scorer, n=4):
        """a BleuScorer over the corpus `scorer` (a `CiderScorer`, ...) already holds on the device: nothing is copied"""
        self = object.__new__(cls)
        self._params(n)
        self._share(scorer)
        self._state()
        return self

    def _params(self, n):
        if n != ORDERS:
            raise ValueError("only n = 4 is implemented (the reference's default), got n = %r" % (n,))
        self.n = n

    def _state(self):
        self.totals = torch.zeros(COMPS, dtype=torch.int64, device=self.device)
        self.last_sentence = self.last_comps = None

    def _launch(self, ids, image_index, end_id, kept, totals):
        ids, stride, B, T, idx = self._rows(ids, image_index, kept)
        comps = torch.empty(B, COMPS, dtype=torch.int64, device=ids.device)
        sentence = torch.empty(B, ORDERS, dtype=torch.float64, device=ids.device)
        mean = torch.empty(ORDERS, dtype=torch.float64, device=ids.device)
        L.check(L.load().sat_bleu_comps(C.byref(self._corpus), ids.data_ptr(), stride, B, T, L.ptr(kept), int(end_id), idx.data_ptr(),
                                        comps.data_ptr(), sentence.data_ptr(), mean.data_ptr(), L.ptr(totals), L.stream()),
                "sat_bleu_comps")
        self.last_sentence, self.last_comps = sentence, comps
        return sentence, mean

    def score(self, ids, image_index, end_id=2, kept=None, order=4):
        """ids, image_index, end_id, kept as for `CiderScorer.score`.  Returns (mean f64 [1], scores f64 [B]): the per-sentence
        Bleu_`order` of every row (the reference's `bleu_list[order - 1]`) and its batch mean.  Leaves last_sentence f64 [B, 4]
        (all four orders) and last_comps i64 [B, 10] (testlen, reflen, guess[4], correct[4]).  The totals are not touched;
        nothing is synchronised."""
        if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= ORDERS:
            raise ValueError("order must be 1, 2, 3 or 4, got %r" % (order,))
        sentence, mean = self._launch(ids, image_index, end_id, kept, None)
        return mean[order - 1:order], sentence[:, order - 1].contiguous()

    def update(self, ids, image_index, end_id=2, kept=None):
        """the same launch with the batch's components added into the device totals; returns the per-sentence BLEU f64 [B, 4]"""
        return self._launch(ids, image_index, end_id, kept, self.totals)[0]

    def compute(self):
        """f64 [4] on the device: the corpus-level Bleu_1..Bleu_4 of every row given to `update` since `reset`"""
        bleu = torch.empty(ORDERS, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.load().sat_bleu_finalize(self.totals.data_ptr(), bleu.data_ptr(), L.stream()), "sat_bleu_finalize")
        return bleu

    def reset(self):
        self.totals.zero_()


class RougeLScorer(_RefCorpus):
    """ROUGE-L (`Rouge.calc_score`, beta = 1.2) of decoded rows against the references of their images; refs as for
    `BleuScorer`.  An empty caption is one token that equals only another empty caption's (the reference's `split(" ")`)."""

    def __init__(self, refs, beta=1.2, device="cuda"):
        self._params(beta)
        self._build(refs, device)

    @classmethod
    def from_scorer(cls, scorer, beta=1.2):
        """a RougeLScorer over the corpus `scorer` (a `CiderScorer`, ...) already holds on the device: nothing is copied"""
        self = object.__new__(cls)
        self._params(beta)
        self._share(scorer)
        return self

    def _params(self, beta):
        beta = float(beta)
        if not (beta > 0.0 and math.isfinite(beta)):
            raise ValueError("beta must be positive and finite")
        self.beta = beta

    def score(self, ids, image_index, end_id=2, kept=None):
        """ids, image_index, end_id, kept as for `CiderScorer.score`.  Returns (mean f64 [1], scores f64 [B]) on the device;
        nothing is synchronised."""
        ids, stride, B, T, idx = self._rows(ids, image_index, kept)
        scores = torch.empty(B, dtype=torch.float64, device=ids.device)
        mean = torch.empty(1, dtype=torch.float64, device=ids.device)
        L.check(L.load().sat_rouge_l_score(C.byref(self._corpus), ids.data_ptr(), stride, B, T, L.ptr(kept), int(end_id),
                                           idx.data_ptr(), self.beta, scores.data_ptr(), mean.data_ptr(), L.stream()),
                "sat_rouge_l_score")
        return mean, scores


class MixedReward:
    """members: [(scorer, weight), ...].  `score` is sum(weight * scorer.score(...)[1]) per row in f64, members in the order
    given, and its mean -- torch arithmetic on the members' device results, no host read.  Anything with
    `score(ids, image_index, end_id=, kept=) -> (mean, scores f64 [B])` is a member; a `BleuScorer` contributes Bleu_4."""

    def __init__(self, members):
        members = list(members)
        if not members:
            raise ValueError("MixedReward needs at least one (scorer, weight)")
        self.members = []
        for m in members:
            if not isinstance(m, (tuple, list)) or len(m) != 2:
                raise TypeError("a member is a (scorer, weight) pair, got %r" % (m,))
            scorer, weight = m
            if not callable(getattr(scorer, "score", None)):
                raise TypeError("%r has no score(ids, image_index, end_id=, kept=)" % (type(scorer).__name__,))
            if isinstance(weight, bool) or not isinstance(weight, (int, float)):
                raise TypeError("a weight must be a number, got %r" % (weight,))
            if not math.isfinite(weight):
                raise ValueError("a weight must be finite, got %r" % (weight,))
            self.members.append((scorer, float(weight)))
        self.last_scores = None

    def score(self, ids, image_index, end_id=2, kept=None):
        """(mean f64 [1], scores f64 [B]); leaves last_scores, the members' own per-row scores in order"""
        parts, total = [], None
        for scorer, weight in self.members:
            _, s = scorer.score(ids, image_index, end_id=end_id, kept=kept)
            if s.dtype != torch.float64 or s.dim() != 1:
                raise TypeError("%s.score returned %s %s, not an f64 vector" % (type(scorer).__name__, s.dtype, tuple(s.shape)))
            parts.append(s)
            total = s * weight if total is None else total + s * weight
        self.last_scores = parts
        return total.mean(dim=0, keepdim=True), total
