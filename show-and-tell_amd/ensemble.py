"""Ensemble decode: a beam search over the mixed distribution of several trained models (the ensembles of checkpoints that
Show-and-Tell and the self-critical paper report; the reference keeps one `model-best.pth` per run, train.py:169-177).

Every member computes its own logits on its own decoder state; `sat_ensemble_logprobs` (include/sat_hip.h) turns the M logits
matrices into ONE matrix of combined log-probabilities on the device, and the unchanged selection kernels -- plain, constrained,
grouped -- take it as they take a model's logits.  All members follow the hypotheses the ensemble selects.

Out of scope (each raises or does not exist): `return_alphas` for ensembles, stochastic ensemble decode (the combine kernel already
makes it possible: its output is a valid `logits` argument of `sat_sample_filtered`), `validation_step`, and SCST with an
ensemble baseline."""
import ctypes as C
import math

import torch

from . import _lib as L
from .attend import ShowAttendTellModel, _EvalDecoder
from .models import DecoderRNN, ShowAndTell, _as_f32, _f32c, check_beam_constraints, check_beam_groups

ENSEMBLE_MAX = 8                                   # include/sat_hip.h, sat_ensemble_logprobs
MODES = {"prob": 0, "logprob": 1}


class Ensemble:
    """`Ensemble(models, weights=None, mode="prob")`: 1..8 members of ONE family -- all `DecoderRNN` (then only
    `sample_beam_features`, on a list of per-member features), all `ShowAndTell`, or all `ShowAttendTellModel` -- with one
    `vocab_size`.  weights: positive finite numbers, normalised to sum 1 (None: uniform).  mode "prob" averages the members'
    probabilities (the usual captioning ensemble), "logprob" their log-probabilities (a product of experts; the selection
    renormalises it).  Everything is checked on the host, before the device is touched: a mixed family raises NotImplementedError,
    the rest ValueError.

    `scores` of an ensemble hypothesis are the sum over its tokens of log_softmax(combined row) as the step kernel forms it; in
    "prob" mode that is the log of the averaged probability.  One member alone delegates to that member's own method: its bits."""

    last_beam_norm_scores = last_beam_order = last_beam_groups = None      # as on a model, set by constrained / grouped calls

    def __init__(self, models, weights=None, mode="prob"):
        try:
            models = list(models)
        except TypeError:
            raise ValueError("models must be a sequence of models, got %r" % (models,))
        if mode not in MODES:
            raise ValueError("mode must be 'prob' or 'logprob', got %r" % (mode,))
        if not 1 <= len(models) <= ENSEMBLE_MAX:
            raise ValueError("an ensemble has 1..%d members, got %d" % (ENSEMBLE_MAX, len(models)))
        for family in (DecoderRNN, ShowAndTell, ShowAttendTellModel):
            if all(isinstance(m, family) for m in models):
                break
        else:
            raise NotImplementedError("the members of an ensemble are all DecoderRNN, all ShowAndTell or all ShowAttendTellModel, got %s"
                                      % ([type(m).__name__ for m in models],))
        vs = [(m.decoder if family is ShowAndTell else m).vocab_size for m in models]
        if len(set(vs)) != 1:
            raise ValueError("the members of an ensemble share one vocabulary, got vocab_size %s" % (vs,))
        if weights is not None:
            try:
                weights = [_as_f32(w) for w in (weights.tolist() if hasattr(weights, "tolist") else weights)]
            except TypeError:
                raise ValueError("weights must be None or a sequence of numbers, got %r" % (weights,))
            if len(weights) != len(models):
                raise ValueError("%d weights for %d members" % (len(weights), len(models)))
            if any(w is None or not math.isfinite(w) or w <= 0 for w in weights):
                raise ValueError("weights must be finite numbers > 0 (as float32), got %r" % (weights,))
        self.models, self.family, self.weights, self.mode, self.vocab_size = models, family, weights, mode, vs[0]

    # ---- public methods ----
    @torch.no_grad()
    def sample(self, images):
        """the greedy ensemble decode: beam width 1 through the same path.  ids i64 [B, 20]"""
        return self.sample_beam(images, beam_size=1)

    @torch.no_grad()
    def sample_beam(self, images, beam_size=5, end_id=None, return_all=False, *, suppress_ids=None, min_length=0,
                    no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0, num_beam_groups=1, diversity_penalty=0.0):
        """`sample_beam` of a model, over the ensemble's distribution: every member's encoder runs in its own eval-mode forward on
        the same images, then `sample_beam_features`.  Keywords, return values and the `last_beam_*` attributes as
        `DecoderRNN.sample_beam` documents them (checked before any encoder runs)."""
        if self.family is DecoderRNN:
            raise NotImplementedError("an ensemble of DecoderRNN members has no encoder: use sample_beam_features(features_list, ...)")
        kw = dict(suppress_ids=suppress_ids, min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size,
                  block_repeat=block_repeat, length_penalty=length_penalty)
        check_beam_constraints(end_id=end_id, vocab_size=self.vocab_size, **kw)
        if check_beam_groups(beam_size, num_beam_groups, diversity_penalty)[0] > 1:
            kw.update(num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty)
        if len(self.models) == 1:                        # the member's own call: its bits
            m = self.models[0]
            out = m.sample_beam(images, beam_size, end_id=end_id, return_all=return_all, **kw)
            return self._adopt(m, out)
        feats = []
        for m in self.models:
            was = m.training
            if was:                                      # (a member left in training mode: batch statistics have no place in a decode)
                m.eval()
            try:
                feats.append(m.encoder(images) if self.family is ShowAndTell else m._encode(images)[0])
            finally:
                if was:
                    m.train(True)
        return self.sample_beam_features(feats, beam_size, end_id, return_all=return_all, **kw)

    @torch.no_grad()
    def sample_beam_features(self, features_list, beam_size=5, end_id=None, steps=20, return_all=False, *, start_id=1,
                             suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0,
                             num_beam_groups=1, diversity_penalty=0.0):
        """The beam search on given features, one entry of `features_list` per member ([B, E_m] for the Show-and-Tell family,
        [B, P_m, C_m] for Show-Attend-Tell; `start_id` is read by the latter only).  Returns ids i64 [B, steps] of the best
        hypothesis; with return_all (ids [B, K, steps] best first, scores [B, K]).

        Show-and-Tell family: ONE `sat_beam_decode_ensemble` call.  Show-Attend-Tell family: the members' `_EvalDecoder` objects in
        lock step -- per step M `sat_vocab_logits_fwd`, the combine, one `sat_beam_step` / `_ex` / `_groups` as
        `ShowAttendTellModel.sample_beam_features` chooses, then per member the `sat_beam_gather_rows` of h, c and the context, and
        `feed`."""
        kw = dict(suppress_ids=suppress_ids, min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size,
                  block_repeat=block_repeat, length_penalty=length_penalty)
        cons = check_beam_constraints(end_id=end_id, vocab_size=self.vocab_size, steps=steps, **kw)
        G, lam = check_beam_groups(beam_size, num_beam_groups, diversity_penalty)
        K = int(beam_size)
        if K < 1 or K > 8:
            raise ValueError("beam_size must be in 1..8")
        features_list = list(features_list)
        if len(features_list) != len(self.models):
            raise ValueError("%d feature tensors for %d members" % (len(features_list), len(self.models)))
        if len({f.shape[0] for f in features_list}) != 1:
            raise ValueError("the members' features differ in batch size: %s" % ([tuple(f.shape) for f in features_list],))
        if len(self.models) == 1:                        # the member's own call: its bits
            if G > 1:
                kw.update(num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty)
            m = self.models[0]
            if self.family is ShowAttendTellModel:
                out = m.sample_beam_features(features_list[0], K, None, end_id, steps, start_id, return_all, **kw)
            else:
                dec = m.decoder if self.family is ShowAndTell else m
                out = dec.sample_beam(features_list[0], K, end_id, steps, return_all, **kw)
                m = dec
            return self._adopt(m, out)
        if self.last_beam_order is not None:
            self.last_beam_norm_scores = self.last_beam_order = self.last_beam_groups = None
        if self.family is ShowAttendTellModel:
            ids, scores = self._attend_beam(features_list, K, end_id, int(steps), start_id, cons, G, lam)
        else:
            ids, scores = self._decoder_beam(features_list, K, end_id, int(steps), cons, G, lam)
        if return_all:
            return ids, scores
        return ids[:, 0].contiguous()

    # ---- internals ----
    def _adopt(self, member, out):
        self.last_beam_norm_scores, self.last_beam_order = member.last_beam_norm_scores, member.last_beam_order
        self.last_beam_groups = member.last_beam_groups
        return out

    def _weight_array(self):
        return None if self.weights is None else (C.c_float * len(self.weights))(*self.weights)

    def _decoder_beam(self, features_list, K, end_id, steps, cons, G, lam):
        decs = [m.decoder if self.family is ShowAndTell else m for m in self.models]
        M, V = len(decs), self.vocab_size
        feats = [_f32c(f, "features") for f in features_list]
        for d, f in zip(decs, feats):
            if f.dim() != 2 or f.shape[1] != d.embed_size:
                raise ValueError("features of a member with embed_size %d must be [B, %d], got %s" % (d.embed_size, d.embed_size, tuple(f.shape)))
        lib, dev, B = L.load(), feats[0].device, feats[0].shape[0]
        lstm = [d._lstm_ptrs() for d in decs]            # kept alive to the end of the call: the structs point into them
        models = (L.SatDecoderModel * M)()
        for j, (d, f) in enumerate(zip(decs, feats)):
            models[j] = L.SatDecoderModel(f.data_ptr(), d.embed.weight.data_ptr(), C.cast(lstm[j], C.POINTER(C.c_void_p)), d.num_layers,
                                          d.linear.weight.data_ptr(), d.linear.bias.data_ptr(), d.embed_size, d.hidden_size)
        eid = -1 if end_id is None else int(end_id)
        ids = torch.empty(B, K, steps, dtype=torch.int64, device=dev)
        scores = torch.empty(B, K, device=dev)
        ranked = cons.active or G > 1
        norm = torch.empty(B, K, device=dev) if ranked else None
        order = torch.empty(B, K, dtype=torch.int32, device=dev) if ranked else None
        wsb = lib.sat_beam_decode_ensemble_ws_bytes(models, M, B, K, V, steps)
        ws, ws_ptr = L.workspace256(wsb, dev)
        L.check(lib.sat_beam_decode_ensemble(models, M, self._weight_array(), MODES[self.mode], B, K, V, steps, eid,
                                             cons.struct(dev) if cons.active else None, G, lam, ids.data_ptr(), L.ptr(scores), L.ptr(norm),
                                             L.ptr(order), ws_ptr, wsb, L.stream()), "sat_beam_decode_ensemble")
        if ranked:
            self.last_beam_norm_scores, self.last_beam_order = norm, order
            if G > 1:
                self.last_beam_groups = order // (K // G)
        return ids, scores

    def _attend_beam(self, features_list, K, end_id, steps, start_id, cons, G, lam):
        ds = [_EvalDecoder(m, f, None, K, steps, start_id, False) for m, f in zip(self.models, features_list)]
        lib, st, dev = ds[0].lib, L.stream(), features_list[0].device
        M, V, R = len(ds), self.vocab_size, ds[0].dims[0]
        B, ldl = R // K, L.pad4(V)
        logits = [torch.zeros(R, ldl, device=dev) for _ in ds]
        ptrs = (C.c_void_p * M)(*[t.data_ptr() for t in logits])
        weights, mode = self._weight_array(), MODES[self.mode]
        comb = torch.zeros(R, ldl, device=dev)
        c2 = [torch.empty(R, d.dims[4], device=dev) for d in ds]
        ctx2 = [torch.empty(R, d.dims[2], device=dev) for d in ds]
        scores = torch.full((B, K), float("-inf"), device=dev)
        scores[:, ::K // G] = 0.0                        # the first slot of every group (one group: hypothesis 0)
        scores2 = torch.empty(B, K, device=dev)
        bws = torch.empty(lib.sat_beam_step_ws_bytes(B, K), dtype=torch.uint8, device=dev)
        parents = torch.empty(steps, R, dtype=torch.int32, device=dev)
        tokens = torch.empty(steps, R, dtype=torch.int64, device=dev)
        eid = -1 if end_id is None else int(end_id)
        cstruct = cons.struct(dev) if cons.active else None
        for i in range(steps):
            for d, lg in zip(ds, logits):
                d.step(None, d.start if i == 0 else None)
                cls = d.m.classifier
                L.check(lib.sat_vocab_logits_fwd(L.ptr(d.Z), L.ptr(cls.weight), L.ptr(cls.bias), R, d.dims[3], V, L.ptr(lg), ldl, st),
                        "sat_vocab_logits_fwd")
            L.check(lib.sat_ensemble_logprobs(ptrs, M, ldl, weights, mode, R, V, L.ptr(comb), ldl, st), "sat_ensemble_logprobs")
            last = tokens[i - 1].data_ptr() if (i > 0 and eid >= 0) else None
            par, tok = parents[i].data_ptr(), tokens[i].data_ptr()
            if G > 1:
                L.check(lib.sat_beam_step_groups(L.ptr(comb), ldl, L.ptr(scores), last, eid, B, K, V, cstruct, L.ptr(parents),
                                                 L.ptr(tokens), i, steps, G, lam, par, tok, L.ptr(scores2), L.ptr(bws), bws.numel(), st),
                        "sat_beam_step_groups")
            elif cstruct is not None:
                L.check(lib.sat_beam_step_ex(L.ptr(comb), ldl, L.ptr(scores), last, eid, B, K, V, cstruct, L.ptr(parents), L.ptr(tokens),
                                             i, steps, par, tok, L.ptr(scores2), L.ptr(bws), bws.numel(), st), "sat_beam_step_ex")
            else:
                L.check(lib.sat_beam_step(L.ptr(comb), ldl, L.ptr(scores), last, eid, B, K, V, par, tok, L.ptr(scores2), L.ptr(bws),
                                          bws.numel(), st), "sat_beam_step")
            scores, scores2 = scores2, scores
            for j, d in enumerate(ds):                   # every member follows the ensemble's survivors
                H, Cw = d.dims[4], d.dims[2]
                src_ctx = d.ctxb
                if K > 1:
                    for (a, b_) in ((d.h, d.h2), (d.c, c2[j])):
                        L.check(lib.sat_beam_gather_rows(L.ptr(a), par, B, K, H, L.ptr(b_), st), "sat_beam_gather_rows")
                    d.h, d.h2, d.c, c2[j] = d.h2, d.h, c2[j], d.c
                    L.check(lib.sat_beam_gather_rows(L.ptr(d.ctxb), par, B, K, Cw, L.ptr(ctx2[j]), st), "sat_beam_gather_rows")
                    src_ctx = ctx2[j]
                d.feed(tok, 1, src_ctx)
        ids = torch.empty(B, K, steps, dtype=torch.int64, device=dev)
        L.check(lib.sat_beam_backtrack(L.ptr(parents), L.ptr(tokens), steps, B, K, L.ptr(ids), st), "sat_beam_backtrack")
        if cstruct is not None or G > 1:                 # the K results of an image by score / length^alpha (alpha 0: by score)
            ids2, ranked = torch.empty_like(ids), torch.empty(B, K, device=dev)
            norm, order = torch.empty(B, K, device=dev), torch.empty(B, K, dtype=torch.int32, device=dev)
            L.check(lib.sat_beam_rerank(L.ptr(ids), L.ptr(scores), B, K, steps, eid, cons.length_penalty, L.ptr(ids2), L.ptr(ranked),
                                        L.ptr(norm), L.ptr(order), st), "sat_beam_rerank")
            ids, scores = ids2, ranked
            self.last_beam_norm_scores, self.last_beam_order = norm, order
            if G > 1:
                self.last_beam_groups = order // (K // G)
        return ids, scores
