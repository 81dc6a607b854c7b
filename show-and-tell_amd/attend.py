"""Show-Attend-Tell behind the same boundary: `ShowAttendTellModel` with the reference's constructor,
`forward(images, captions, lengths)` and `sample(images, states)` (the reference's `model2.py:9-111`, the model
`train.py:37` constructs), every tensor op a libsat_hip.so kernel.  Here: the decoder's forward paths and the model class.

    encoder  : `vgg.py` -- VGG16 `features[:-3]` (model2.py:15-16), frozen (model2.py:17) unless `finetune(allow=True)`
    setup    : `_DecoderSetup` -- context_encode = features @ image_att_w, init_lstm, the tapes, Wz = [W_c2o | W_h2o]; it also
               writes the record `attend_backward` reads
    training : `_AttendFn` -- per packed step the weight_hh projection, sat_attention_fwd (tanh / softmax / weighted mean,
               model2.py:73-78) and sat_lstmcell_fwd (model2.py:58), output_layer batched over all packed rows after the loop
               (model2.py:80-85); with ss_prob > 0 (scheduled sampling, train.py:109-113) the whole loop, output layer and
               Gumbel-max draws per step, is one `sat_ss_attend_fwd` call.  `_AttendRolloutFn` (`rollout`, `scst_forward`: self-
               critical training) feeds the decoder its own tokens -- drawn, or the arg-max -- as one `sat_rollout_attend_fwd` call
    eval     : `_EvalDecoder` -- the setup for R rows, one decode step and the loop around it; `sample_features` (R = B),
               `sample_stochastic_features` (R = B * S) and `sample_beam_features` (R = B * K) each supply the choice of a step's tokens
    backward : `attend_bwd.py`, hand-written (sat_attention_bwd, LSTMCell BPTT, batched weight-gradient GEMMs) behind
               torch.autograd, so `loss.backward()` (train.py:144) works unchanged

state_dict keys equal the reference's: `encoder.{0,2,5,...}.weight/bias`, `image_att_w`, `init_hidden.*`, `init_memory.*`,
`weight_hh.*`, `weight_att`, `embedding.weight`, `lstmcell.{weight_ih,weight_hh,bias_ih,bias_hh}`, `context2out.*`,
`hidden2tout.*`, `classifier.*`.  GPU only: there is no CPU fallback.
"""
import math

import torch
import torch.nn as nn

from . import _lib as L
from .attend_bwd import PARAM_ORDER, attend_backward
from .decoder import dropout_rows
from .models import check_beam_constraints, check_beam_groups, check_dropout_p, check_sample_args, check_sample_constraints, draw_ss_seed, lookahead_stream, refuse_dropout_with, stochastic_result
from .pack import PackInfo
from .scst import SelfCritical, check_group, repeat_rows
from .vgg import VGG16_FEATURES, VggFeatures, VggProgram, _VggFn  # noqa: F401  (VggFeatures is re-exported by the package)
from .watch import IdGuard


class _Lin(nn.Module):
    def __init__(self, fin, fout):
        super().__init__()
        k = 1.0 / math.sqrt(fin)
        self.weight = nn.Parameter(torch.empty(fout, fin).uniform_(-k, k))         # nn.Linear default init
        self.bias = nn.Parameter(torch.empty(fout).uniform_(-k, k))


class _Emb(nn.Module):
    def __init__(self, v, e):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(v, e).normal_(0, 1))                # nn.Embedding default init


class _Cell(nn.Module):
    def __init__(self, fin, h):
        super().__init__()
        k = 1.0 / math.sqrt(h)
        self.weight_ih = nn.Parameter(torch.empty(4 * h, fin).uniform_(-k, k))     # nn.LSTMCell default init
        self.weight_hh = nn.Parameter(torch.empty(4 * h, h).uniform_(-k, k))
        self.bias_ih = nn.Parameter(torch.empty(4 * h).uniform_(-k, k))
        self.bias_hh = nn.Parameter(torch.empty(4 * h).uniform_(-k, k))


_SS_WEIGHTS = ("weight_hh.weight", "weight_hh.bias", "weight_att", "embedding.weight", "lstmcell.weight_ih", "lstmcell.weight_hh",
               "lstmcell.bias_ih", "lstmcell.bias_hh", "context2out.weight", "context2out.bias", "hidden2tout.weight",
               "hidden2tout.bias", "classifier.weight", "classifier.bias")      # include/sat_hip.h SAT_SSA_* order
_SS_TAPES = ("PROJ", "ALPHA", "X", "GATES", "CS", "HS", "Zin", "Z")                # SAT_SSA_PROJ .. SAT_SSA_Z


def _context_encode(lib, m, f2):
    """context_encode = features @ image_att_w (model2.py:46) for the flattened features f2 [rows * P, C]"""
    C = f2.shape[1]
    ctx_enc = torch.empty_like(f2)
    L.gemm(lib, 0, 1, f2, C, m.image_att_w, C, ctx_enc, C, f2.shape[0], C, C)
    return ctx_enc


def _context_encode_group(lib, m, src, S, f2):
    """`_context_encode(f2)` for f2 = the features of `src` [B, P, C] with every image S times in a row, encoded ONCE per image
    and the result repeated (data movement): the bits of encoding all R * P rows, for 1 / S of the GEMM.  A row of
    `sat_gemm_f32`'s result does not depend on how many rows the call has: the row count only picks the workgroup tile (64 x 64,
    128 x 64 or 128 x 128, `launch_f32_auto`), and every tile walks K in the same steps of 32 with the same 32x32x2 f32 MFMA in
    the same order, so B * P rows and R * P rows may take different tiles and still agree bit for bit.  The split-K kernel's K
    split does depend on the row count: where `L.gemm` would hand the R * P-row call to it (`L.gemm_splits_k`, the rule `L.gemm`
    itself dispatches by), the repeated matrix is encoded as it stands."""
    B, P, C = src.shape
    if L.gemm_splits_k(0, 1, C, C, C, f2.shape[0], C, C):
        return _context_encode(lib, m, f2)
    enc = torch.empty(B * P, C, device=src.device)
    L.check(lib.sat_gemm_f32(0, 1, L.ptr(src), C, L.ptr(m.image_att_w), C, L.ptr(enc), C, None, None, B * P, C, C, L.stream()),
            "sat_gemm_f32")
    return enc.view(B, P * C).repeat_interleave(S, 0).view(B * S * P, C)


def _output_weight(lib, m):
    """Wz = [W_c2o | W_h2o] [E, C + H]: the output layer (model2.py:80-85) as one GEMM z = [ctx | h] Wz^T + b1 + b2, and the
    backward's dZin = dZ Wz"""
    (E, C), H = m.context2out.weight.shape, m.hidden_size
    st = L.stream()
    Wz = torch.empty(E, C + H, device=m.context2out.weight.device)
    L.check(lib.sat_rows_copy(L.ptr(m.context2out.weight), C, None, 0, E, E, C, L.ptr(Wz), C + H, st), "sat_rows_copy")
    L.check(lib.sat_rows_copy(L.ptr(m.hidden2tout.weight), H, None, 0, E, E, H, Wz.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
    return Wz


class _DecoderSetup:
    """What every training forward of the decoder starts from, for N packed rows: f2 (the features as [B * P, C]), ctx_enc (its
    GEMM), HSX = [h_0 ; h of every packed row] (h_{t-1} of any row is one gather away) with h0 = HSX[:B] and c0 from init_lstm
    (model2.py:67-71, two GEMMs), the tapes `tp` named as in `_SS_TAPES` (HS = HSX[B:]), the token buffer toks [N] and Wz.
    with_wz=False leaves Wz to the caller: the teacher-forced loop builds it behind its steps."""

    def __init__(self, lib, m, features, fmean, N, with_wz=True, group=None):
        """group: None, or (src [B / S, P, C], S) when `features` is src with every image S times in a row (`rollout(num_samples=S)`)"""
        dev = features.device
        B, P, C = features.shape
        E, H = m.embed_size, m.hidden_size
        self.m, self.fmean = m, fmean
        self.f2 = features.view(B * P, C)
        self.ctx_enc = _context_encode(lib, m, self.f2) if group is None else _context_encode_group(lib, m, *group, self.f2)
        self.HSX = torch.empty(B + N, H, device=dev)
        self.h0, self.c0 = self.HSX[:B], torch.empty(B, H, device=dev)
        L.gemm(lib, 0, 0, fmean, C, m.init_hidden.weight, C, self.h0, H, B, H, C, m.init_hidden.bias)
        L.gemm(lib, 0, 0, fmean, C, m.init_memory.weight, C, self.c0, H, B, H, C, m.init_memory.bias)
        self.tp = dict(PROJ=torch.empty(N, C, device=dev), ALPHA=torch.empty(N, P, device=dev), X=torch.empty(N, H, device=dev),
                       GATES=torch.empty(N, 4 * H, device=dev), CS=torch.empty(N, H, device=dev), HS=self.HSX[B:],
                       Zin=torch.empty(N, C + H, device=dev), Z=torch.empty(N, E, device=dev))
        self.toks = torch.empty(N, dtype=torch.int64, device=dev)
        self.Wz = _output_weight(lib, m) if with_wz else None

    def ssa_tables(self):
        """the weight and tape pointer arrays (SAT_SSA_* order) of `sat_ss_attend_fwd` / `sat_rollout_attend_fwd`"""
        named = dict(self.m.named_parameters())
        w = (L.C.c_void_p * len(_SS_WEIGHTS))(*[named[k].data_ptr() for k in _SS_WEIGHTS])
        tapes = (L.C.c_void_p * len(_SS_TAPES))(*[self.tp[k].data_ptr() for k in _SS_TAPES])
        return w, tapes

    def record(self, ctx, pi, fed):
        """what `attend_backward` reads, onto ctx: the model, the packing, the tokens fed and the tapes"""
        ctx.m, ctx.pi, ctx.captions = self.m, pi, fed
        ctx.tapes = dict(f2=self.f2, fmean=self.fmean, ctx_enc=self.ctx_enc, h0=self.h0, c0=self.c0, Wz=self.Wz, toks=self.toks,
                         HSX=self.HSX, **self.tp)


class _AttendFn(torch.autograd.Function):
    """decoder half of model2.py:38-65 given the encoder features (the conv stack is frozen, model2.py:17)."""

    @staticmethod
    def forward(ctx, model, features, fmean, captions, pi, ss, ex, *params):
        """ss: None (teacher forcing) or dict(prob, seed, rank) -- scheduled sampling through `sat_ss_attend_fwd`; receives
        "used", the tokens fed [B, T].  ex: dict(alpha_c) -- receives "alphas", the packed [N, P] attention tape; with
        alpha_c > 0 the doubly stochastic penalty is a second output (`_attend_outputs`); dropout: None or (p, seed, rank) -- the Z
        tape is dropped in place (site 0) between the output layer and the classifier, its only readers being the classifier GEMM
        and the backward's dW = dlogits^T Z (teacher forcing only)."""
        lib, m, st, dev = L.load(), model, L.stream(), features.device
        s = _DecoderSetup(lib, m, features, fmean, pi.N, with_wz=ss is not None)
        if ss is not None:
            logits = _ss_attend_forward(lib, s, captions, pi, ss)
        else:
            B, P, C = features.shape
            E, H, V, Hin, N = m.embed_size, m.hidden_size, m.vocab_size, m.hidden_size, pi.N
            PROJ, ALPHA, X, GATES, CS, HS, Zin, Z = (s.tp[k] for k in _SS_TAPES)
            c = s.c0.clone()
            att_ws = torch.empty(B * P, device=dev)
            # the embedding half of every step's LSTMCell input [emb | ctx] (model2.py:55-57) in one gather
            L.check(lib.sat_pack_tokens(captions.data_ptr(), captions.stride(0), pi.prefix_dev.data_ptr(), pi.T, N, 0, s.toks.data_ptr(), st),
                    "sat_pack_tokens")
            L.check(lib.sat_rows_copy(L.ptr(m.embedding.weight), E, s.toks.data_ptr(), 1, V, N, E, L.ptr(X), Hin, st), "sat_rows_copy")
            for t, bs in enumerate(pi.batch_sizes):                                                  # model2.py:54-62
                r0 = pi.prefix[t]
                hprev = s.h0.data_ptr() if t == 0 else L.rows(HS, pi.prefix[t - 1])
                L.gemm(lib, 0, 0, hprev, H, m.weight_hh.weight, H, L.rows(PROJ, r0), C, bs, C, H, m.weight_hh.bias)
                # the context lands in its half of the LSTMCell input row (ld = Hin)
                L.check(lib.sat_attention_fwd(L.ptr(s.ctx_enc), L.ptr(s.f2), L.rows(PROJ, r0), C, L.ptr(m.weight_att), bs, P, C, L.rows(ALPHA, r0),
                                              L.rows(X, r0) + E * 4, Hin, att_ws.data_ptr(), att_ws.numel() * 4, st), "sat_attention_fwd")
                L.check(lib.sat_lstmcell_fwd(L.rows(X, r0), hprev, L.ptr(c), L.ptr(m.lstmcell.weight_ih), L.ptr(m.lstmcell.weight_hh),
                                             L.ptr(m.lstmcell.bias_ih), L.ptr(m.lstmcell.bias_hh), bs, Hin, H, L.rows(HS, r0),
                                             L.rows(GATES, r0), L.rows(CS, r0), st), "sat_lstmcell_fwd")
            # output_layer over all packed rows at once (model2.py:80-85): z = [ctx | h] [W_c2o | W_h2o]^T + b1 + b2
            L.check(lib.sat_rows_copy(X.data_ptr() + E * 4, Hin, None, 0, N, N, C, L.ptr(Zin), C + H, st), "sat_rows_copy")
            L.check(lib.sat_rows_copy(L.ptr(HS), H, None, 0, N, N, H, Zin.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
            s.Wz = _output_weight(lib, m)
            L.gemm(lib, 0, 0, Zin, C + H, s.Wz, C + H, Z, E, N, E, C + H, m.context2out.bias, m.hidden2tout.bias)
            if ex.get("dropout") is not None:               # where the reference keeps its unused nn.Dropout (model2.py:34)
                dropout_rows(lib, Z, *ex["dropout"], 0)
            logits = L.logits_buffer(N, V, dev)
            L.gemm(lib, 0, 0, Z, E, m.classifier.weight, E, logits, logits.shape[1], N, V, E, m.classifier.bias)
        s.record(ctx, pi, captions)
        ctx.tapes["dropout"] = ex.get("dropout") if ss is None else None
        return _attend_outputs(ctx, lib, ex, logits, m.vocab_size)

    @staticmethod
    def backward(ctx, dlogits, *dpen):
        want = ctx.needs_input_grad[1]                     # features carry a graph only when the conv stack is fine-tuned
        extra = scale = None
        if ctx.cov_grad is not None:
            # the penalty's incoming gradient stays on the device (autograd hands zeros for an output the loss never used)
            extra, scale = ctx.cov_grad, dpen[0].to(torch.float32).contiguous()
        grads, d_feats, d_fmean = attend_backward(ctx.m, ctx.pi, ctx.captions, ctx.tapes, dlogits, want_dfeat=want,
                                                  d_alpha_extra=extra, d_alpha_scale=scale)
        return (None, d_feats, d_fmean if ctx.needs_input_grad[2] else None, None, None, None, None) + tuple(grads)


def _ss_attend_forward(lib, s, captions, pi, ss):
    """the recurrence of `_AttendFn.forward` with scheduled sampling (model2.py:54-62 + 80-85 per step, the input of step t >= 1
    drawn from the logits of step t-1 with probability ss["prob"]): one `sat_ss_attend_fwd` call leaves the same tapes, so
    attend_backward runs unchanged on the tokens fed"""
    m, st, dev = s.m, L.stream(), s.f2.device
    B, P, C = pi.B, s.tp["ALPHA"].shape[1], s.f2.shape[1]
    E, H, V, N, T = m.embed_size, m.hidden_size, m.vocab_size, pi.N, pi.T
    w, tapes = s.ssa_tables()
    used = torch.empty(B, T, dtype=torch.int64, device=dev)
    logits = L.logits_buffer(N, V, dev)
    wsb = lib.sat_ss_attend_fwd_ws_bytes(B, P, C, E, H, V)
    ws = torch.empty(wsb // 4, device=dev)
    L.check(lib.sat_ss_attend_fwd(s.f2.data_ptr(), s.ctx_enc.data_ptr(), s.h0.data_ptr(), s.c0.data_ptr(), captions.data_ptr(),
                                  captions.stride(0), pi.bs_c, pi.prefix_dev.data_ptr(), T, P, C, E, H, V, w, tapes,
                                  s.toks.data_ptr(), logits.data_ptr(), logits.shape[1], float(ss["prob"]), int(ss["seed"]),
                                  int(ss["rank"]), used.data_ptr(), used.stride(0), ws.data_ptr(), wsb, st), "sat_ss_attend_fwd")
    ss["used"] = used
    return logits


def _attend_outputs(ctx, lib, ex, logits, V):
    """What `_AttendFn.forward` returns, teacher-forced or sampled: the logits, and with ex["alpha_c"] > 0 also the doubly
    stochastic penalty alpha_c * mean_{b,p} (1 - sum_t alpha[b,t,p])^2 as a 0-dim tensor -- one `sat_attention_coverage` call over
    the packed tape; its grad [B, P] stays on ctx for the backward."""
    pi, ALPHA = ctx.pi, ctx.tapes["ALPHA"]
    ex["alphas"] = ALPHA
    ctx.cov_grad = None
    out = logits if logits.shape[1] == V else logits[:, :V]
    if not ex["alpha_c"] > 0:
        return out
    B, P, dev = pi.B, ALPHA.shape[1], ALPHA.device
    grad, pen = torch.empty(B, P, device=dev), torch.empty((), device=dev)
    wsb = lib.sat_attention_coverage_ws_bytes(B, P)
    ws = torch.empty(wsb // 4, device=dev)
    L.check(lib.sat_attention_coverage(ALPHA.data_ptr(), pi.prefix_dev.data_ptr(), pi.T, B, P, float(ex["alpha_c"]) / (B * P), None,
                                       grad.data_ptr(), pen.data_ptr(), ws.data_ptr(), wsb, L.stream()), "sat_attention_coverage")
    ctx.cov_grad = grad
    return out, pen


class _AttendRolloutFn(torch.autograd.Function):
    """The rollout of the decoder half (self-critical training): `sat_rollout_attend_fwd` feeds every step the token it took from
    the previous step's logits -- a draw, or the arg-max -- and leaves the tapes of the teacher-forced forward on those tokens, so
    the backward is `attend_backward` on `fed`."""

    @staticmethod
    def forward(ctx, model, features, fmean, steps, greedy, start_id, seed, rank, out, *params):
        """out: dict that receives "ids" [B, steps], "fed" [B, steps] (the tokens fed) and "alphas", the packed attention tape;
        it may bring "group" = (src, S): `features` / `fmean` are then src's rows S times each (`_DecoderSetup`)"""
        lib, m, dev = L.load(), model, features.device
        B, P, C = features.shape
        E, H, V = m.embed_size, m.hidden_size, m.vocab_size
        pi = PackInfo.get([steps] * B, dev)
        N = pi.N
        s = _DecoderSetup(lib, m, features, fmean, N, group=out.pop("group", None))
        w, tapes = s.ssa_tables()
        ids = torch.empty(B, steps, dtype=torch.int64, device=dev)
        fed = torch.empty(B, steps, dtype=torch.int64, device=dev)
        logits = L.logits_buffer(N, V, dev)
        wsb = lib.sat_rollout_attend_fwd_ws_bytes(B, P, C, E, H, V)
        ws = torch.empty(wsb // 4, device=dev)
        L.check(lib.sat_rollout_attend_fwd(s.f2.data_ptr(), s.ctx_enc.data_ptr(), s.h0.data_ptr(), s.c0.data_ptr(),
                                           pi.prefix_dev.data_ptr(), B, steps, P, C, E, H, V, w, tapes, s.toks.data_ptr(),
                                           logits.data_ptr(), logits.shape[1], 1 if greedy else 0, start_id, seed, rank,
                                           ids.data_ptr(), ids.stride(0), fed.data_ptr(), fed.stride(0), ws.data_ptr(), wsb,
                                           L.stream()), "sat_rollout_attend_fwd")
        if not greedy:
            # The loop's Z rows came from per-step split-K GEMMs (the draws need each step's logits).  The backward reads Z once, for
            # the classifier's weight gradient: give it the tape `_AttendFn.forward` leaves -- the output layer over all packed rows
            # as ONE GEMM with the two biases added in turn -- so that the gradients are, bit for bit, those of `decode` on `fed`.
            L.gemm(lib, 0, 0, s.tp["Zin"], C + H, s.Wz, C + H, s.tp["Z"], E, N, E, C + H, m.context2out.bias, m.hidden2tout.bias)
        out["ids"], out["fed"], out["alphas"] = ids, fed, s.tp["ALPHA"]
        s.record(ctx, pi, fed)
        return logits if logits.shape[1] == V else logits[:, :V]

    @staticmethod
    def backward(ctx, dlogits):
        grads, d_feats, d_fmean = attend_backward(ctx.m, ctx.pi, ctx.captions, ctx.tapes, dlogits, want_dfeat=ctx.needs_input_grad[1])
        return (None, d_feats, d_fmean if ctx.needs_input_grad[2] else None) + (None,) * 6 + tuple(grads)


class _EvalDecoder:
    """The eval-mode decode of `sample` / `sample_stochastic` / `sample_beam` (model2.py:91-111) over R = B * rows rows: the setup
    all three share, one decode step, and the loop around it, which leaves only the choice of a step's tokens to its caller.

    Setup: `states` is checked before anything touches the device; the features (repeated `rows` times per image, row b * rows + r)
    as f2 [R * P, C] and their attention encoding; the state h, c as PRIVATE copies of `states` (zeros for None) -- the caller's
    tensors are never written; h2 is where the LSTMCell writes (the two swap); this step's context ctxb, the LSTMCell input X =
    [embedding | context] and the output layer's Z [R, E], which the token choice reads; the `start` column step 0 feeds; with
    return_alphas the maps of every step, amaps [steps, R, P] (step i's slice is the attention kernel's alpha output)."""

    def __init__(self, m, features, states, rows, steps, start_id, return_alphas):
        B, P, C = features.shape
        E, H = m.embed_size, m.hidden_size
        _check_states(states, B, H)
        L.require_gpu(features, "features")
        lib, dev, R = L.load(), features.device, B * rows
        feats = features.contiguous()
        if rows > 1:
            feats = feats.repeat_interleave(rows, 0).contiguous()
        self.lib, self.m, self.steps = lib, m, steps
        self.f2 = f2 = feats.view(R * P, C)
        self.ctx_enc = _context_encode(lib, m, f2)
        if states is None:
            self.h, self.c = torch.zeros(R, H, device=dev), torch.zeros(R, H, device=dev)
        elif rows > 1:
            self.h, self.c = (s.to(dev).float().repeat_interleave(rows, 0).contiguous() for s in states)
        else:
            self.h, self.c = (s.to(dev).float().contiguous().clone() for s in states)
        self.dims = R, P, C, E, H, m.vocab_size
        self.h2 = torch.empty(R, H, device=dev)
        self.proj, self.X = torch.empty(R, C, device=dev), torch.empty(R, H, device=dev)
        self.ctxb, self.Zin, self.Z = torch.empty(R, C, device=dev), torch.empty(R, C + H, device=dev), torch.empty(R, E, device=dev)
        self.Wz = _output_weight(lib, m)
        self.att_ws = torch.empty(f2.shape[0], device=dev)        # R * P
        self.start = torch.full((R,), int(start_id), dtype=torch.int64, device=dev)
        self.amaps = torch.empty(steps, R, P, device=dev) if return_alphas else None

    def run(self, pick):
        """The decode loop.  `pick(i)` chooses step i's tokens from this step's Z (and may re-order the state); it returns what is
        fed with them: (device pointer of the R int64 tokens, their stride, the context rows)."""
        for i in range(self.steps):
            self.step(self.amaps[i].data_ptr() if self.amaps is not None else None, self.start if i == 0 else None)
            self.feed(*pick(i))

    def maps(self, lead):
        """the recorded maps, rows first: f32 [*lead, steps, P] (lead: the shape the R rows are viewed as)"""
        return self.amaps.transpose(0, 1).contiguous().view(tuple(lead) + (self.steps, self.dims[1]))

    def step(self, alpha=None, first=None):
        """h, c -> the next h, c and Z.  alpha: None or the device pointer that receives this step's maps [R, P]; first: the
        token column [R] of step 0, whose input is [embedding(first) | step 0's own context] (model2.py:101-102)"""
        lib, m, st = self.lib, self.m, L.stream()
        R, P, C, E, H, V = self.dims
        L.gemm(lib, 0, 0, self.h, H, m.weight_hh.weight, H, self.proj, C, R, C, H, m.weight_hh.bias)
        L.check(lib.sat_attention_fwd(L.ptr(self.ctx_enc), L.ptr(self.f2), L.ptr(self.proj), C, L.ptr(m.weight_att), R, P, C, alpha,
                                      L.ptr(self.ctxb), C, self.att_ws.data_ptr(), self.att_ws.numel() * 4, st), "sat_attention_fwd")
        if first is not None:
            self.feed(first.data_ptr(), 1, self.ctxb)
        L.check(lib.sat_lstmcell_fwd(L.ptr(self.X), L.ptr(self.h), L.ptr(self.c), L.ptr(m.lstmcell.weight_ih),
                                     L.ptr(m.lstmcell.weight_hh), L.ptr(m.lstmcell.bias_ih), L.ptr(m.lstmcell.bias_hh), R, H, H,
                                     L.ptr(self.h2), None, None, st), "sat_lstmcell_fwd")
        self.h, self.h2 = self.h2, self.h
        L.check(lib.sat_rows_copy(L.ptr(self.ctxb), C, None, 0, R, R, C, L.ptr(self.Zin), C + H, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(self.h), H, None, 0, R, R, H, self.Zin.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
        L.gemm(lib, 0, 0, self.Zin, C + H, self.Wz, C + H, self.Z, E, R, E, C + H, m.context2out.bias, m.hidden2tout.bias)

    def feed(self, tokens, stride, context):
        """the next LSTMCell input = [embedding(token) | context] (model2.py:107-108: THIS step's context); tokens: device pointer
        of R int64 ids `stride` elements apart"""
        lib, m, st = self.lib, self.m, L.stream()
        R, P, C, E, H, V = self.dims
        L.check(lib.sat_rows_copy(L.ptr(m.embedding.weight), E, tokens, stride, V, R, E, L.ptr(self.X), H, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(context), C, None, 0, R, R, C, self.X.data_ptr() + E * 4, H, st), "sat_rows_copy")


def _check_states(states, B, H):
    if states is not None and (len(states) != 2 or any(tuple(s.shape) != (B, H) for s in states)):
        raise ValueError("states must be (h, c), each [B=%d, H=%d] (model2.py:99), got %s"
                         % (B, H, [tuple(s.shape) for s in states]))


class ShowAttendTellModel(nn.Module):
    """model2.py:9-111.  `compute_dtype` ('bf16' conv stack / 'f32' parity) and `vgg_cfg` are build extensions."""

    last_beam_norm_scores = last_beam_order = None     # set by a constrained `sample_beam` (None after a plain one)
    last_beam_groups = None                            # set by a grouped `sample_beam`: [B,K] i32, the group of the hypothesis at r

    def __init__(self, hidden_size, context_size, vocab_size, embed_size, opt=None, feature_size=(196, 512),
                 compute_dtype="bf16", vgg_cfg=VGG16_FEATURES):
        super().__init__()
        feat = int(feature_size[1])
        if embed_size + feat != hidden_size:
            raise ValueError("the LSTMCell input is cat[embedding, context] (model2.py:57-58): hidden_size must equal "
                             "embed_size + %d" % feat)
        if context_size != feat:
            raise ValueError("weight_hh(hidden) is added to context_encode (model2.py:74): context_size must equal %d" % feat)
        if feat % 4 or hidden_size % 4 or embed_size % 4:
            raise ValueError("feature, hidden and embed sizes must be multiples of 4")
        self.opt = opt
        self.encoder = VggFeatures(vgg_cfg)                                             # model2.py:15-16
        if self.encoder.out_channels != feat:
            raise ValueError("the conv stack ends in %d channels, feature_size says %d" % (self.encoder.out_channels, feat))
        self.compute_dtype = compute_dtype
        self.finetune(allow=False)                                                      # model2.py:17
        self.image_att_w = nn.Parameter(torch.empty(feat, feat).normal_(0, 0.05))       # model2.py:20 (uninitialised there)
        self.init_hidden, self.init_memory = _Lin(feat, hidden_size), _Lin(feat, hidden_size)
        self.weight_hh = _Lin(hidden_size, context_size)
        self.weight_att = nn.Parameter(torch.empty(feat, 1).normal_(0, 0.05))           # model2.py:25 (uninitialised there)
        self.embedding = _Emb(vocab_size, embed_size)
        self.lstmcell = _Cell(hidden_size, hidden_size)
        self.context2out, self.hidden2tout = _Lin(context_size, embed_size), _Lin(hidden_size, embed_size)
        self.classifier = _Lin(embed_size, vocab_size)
        self.hidden_size, self.embed_size, self.vocab_size, self.feat = hidden_size, embed_size, vocab_size, feat
        self.ss_prob = 0                  # scheduled sampling (train.py:109-113; schedule: trainer.ss_prob_for_epoch), training mode only
        self.ss_rank = 0                  # data-parallel rank: a stream of draws of its own per rank
        self.last_ss_inputs = self.last_ss_seed = None   # tokens fed [B, T] and seed of the last sampled forward
        self.alpha_c = 0                  # weight of the doubly stochastic attention penalty (Xu et al. 2015, section 4.2.1); 0 = off
        self.last_alphas = self.last_attention_penalty = None    # set by every decode / forward
        self.last_rollout_inputs = self.last_rollout_seed = None # tokens fed [B, steps] and seed of the last `rollout`
        self.last_scst = None                                    # the `SelfCritical` object of the last `scst_forward`
        self.last_sample_seed = None                             # seed of the last `sample_stochastic`
        # dropout on Z = context2out(ctx) + hidden2tout(h) in front of the classifier, training mode only: where model2.py:34 builds
        # an nn.Dropout(p=0.5) it never calls (masks: include/sat_hip.h `sat_dropout_f32`, site 0, rank `ss_rank`); 0 = off
        self.dropout_p = 0.0
        self.last_dropout_seed = None                            # seed of the last forward that dropped anything
        self._programs, self._guard = {}, None
        self._pf_list = []          # features in flight: [(images, feats, fmean, event, weights signature, instance)]
        self.register_load_state_dict_post_hook(lambda mod, k: mod._programs.clear())
        self.encoder.register_load_state_dict_post_hook(lambda mod, k: self._programs.clear())

    def finetune(self, allow=False):
        """model2.py:87-89: (un)freeze the conv stack.  Fine-tuning runs the stack with a hand-written backward (dgrad through
        the forward conv kernel on flipped weights, wgrad as split-K GEMMs, ReLU / max-pool routing) in the f32 parity mode."""
        # compute_dtype='bf16': mixed precision -- the parameters ARE the f32 master weights; the stack runs on bf16 copies
        # refreshed from them before every forward (VggProgram.refresh_weights), gradients come back in f32 (VggProgram.backward)
        for p in self.encoder.parameters():
            p.requires_grad = True if allow else False

    def _apply(self, fn, *a, **k):
        self._programs.clear()
        return super()._apply(fn, *a, **k)

    PF_DEPTH = 2      # batches whose features may be in flight (own program instance and side stream each)

    def prefetch_features(self, images):
        """Start the FROZEN conv stack (model2.py:17 `finetune(allow=False)`) of a LATER batch on a side stream, under the current
        batch's decoder forward / backward / optimizer (hundreds of small launches that leave most of the chip idle).  The
        features depend on the images and the frozen weights only, so this changes the schedule, not a bit of the result;
        `forward(images, ...)` / `sample(images)` of the SAME tensor object picks them up; other tensors are computed as usual
        and leave the batches in flight alone.  No-op while fine-tuning."""
        if images is None or any(p.requires_grad for p in self.encoder.parameters()):
            return False
        if any(e[0] is images for e in self._pf_list) or len(self._pf_list) >= self.PF_DEPTH:
            return False
        busy = {e[5] for e in self._pf_list}
        inst = next(i for i in range(self.PF_DEPTH) if i not in busy)
        stream = lookahead_stream(images.device, inst)
        main = torch.cuda.current_stream(images.device)
        stream.wait_stream(main)
        ready = getattr(images, "_sat_ready_event", None)      # a DevicePrefetcher copy still in flight on its own stream
        if ready is not None:
            stream.wait_event(ready)
        with torch.cuda.stream(stream), torch.no_grad():
            feats, fmean = self._program_for(images, instance=inst).run(images)
            feats, fmean = feats.clone(), fmean.clone()
            ev = torch.cuda.Event()
            ev.record(stream)
        feats.record_stream(main)
        fmean.record_stream(main)
        self._pf_list.append((images, feats, fmean, ev, self._encoder_sig(), inst))
        return True

    def _encoder_sig(self):
        """Frozen stack: changes when a weight is replaced or written in place (the program's kernel-layout copies are then
        rebuilt).  While fine-tuning the weights change EVERY step, so the program is keyed on the storage only and its copies
        are refreshed in place before each forward (`VggProgram.refresh_weights`)."""
        if any(p.requires_grad for p in self.encoder.parameters()):
            return -1 - (sum(p.data_ptr() & 0xffffffff for p in self.encoder.parameters()) & ((1 << 40) - 1))
        return sum(p._version * 7 + (p.data_ptr() & 0xffffffff) for p in self.encoder.parameters())

    def _program_for(self, images, instance=None):
        """instance None: the program `forward` runs; 0, 1: independent copies (own buffers) for batches in flight"""
        N, _, H, W = images.shape
        dt = L.SAT_BF16 if self.compute_dtype == "bf16" else L.SAT_F32
        sig = self._encoder_sig()
        key = (N, H, W, dt, str(images.device), sig, instance)
        prog = self._programs.get(key)
        if prog is None:
            for k in [k for k in self._programs if k[5] != sig or len(self._programs) >= 6]:
                del self._programs[k]
            prog = self._programs[key] = VggProgram(self.encoder, N, H, W, dt, images.device)
        return prog

    def _encode(self, images):
        L.require_gpu(images, "images")
        frozen = not any(p.requires_grad for p in self.encoder.parameters())
        for k, e in enumerate(self._pf_list):
            if e[0] is images:
                del self._pf_list[k]
                torch.cuda.current_stream(images.device).wait_event(e[3])
                if frozen and e[4] == self._encoder_sig():
                    return e[1], e[2]
                break                                  # weights changed meanwhile: compute again
        prog = self._program_for(images)
        tuned = [p for p in self.encoder.parameters() if p.requires_grad]
        if tuned:
            prog.refresh_weights()
        if tuned and torch.is_grad_enabled():
            if len(tuned) != 2 * len(self.encoder.conv_names):
                raise NotImplementedError("fine-tune all of the conv stack or none of it (model2.py:87-89)")
            params = []
            for cv in self.encoder.convs():
                params += [cv.weight, cv.bias]
            feats, fmean = _VggFn.apply(prog, images, *params)
        else:
            with torch.no_grad():
                feats, fmean = prog.run(images)
            feats, fmean = feats.clone(), fmean.clone()   # the program's buffers are overwritten by the next forward
        if feats.shape[2] != self.feat:
            raise ValueError("encoder features have %d channels, expected %d" % (feats.shape[2], self.feat))
        return feats, fmean

    def _params(self):
        d = dict(self.named_parameters())
        return [d[k] for k in PARAM_ORDER]

    def dropout_plan(self, sampling=False, what="ss_prob > 0 (scheduled sampling)"):
        """`dropout_p` as float32 when a training forward drops, else None (eval mode or 0).  Host checks only, nothing drawn:
        ValueError for a probability outside [0, 1), NotImplementedError when the mask is active and `sampling` says the forward
        is one of the step loops that project inside one library call (`what`)."""
        p = check_dropout_p(self.dropout_p, "dropout_p")
        if not (self.training and p > 0):
            return None
        if sampling:
            refuse_dropout_with(["dropout_p"], what)
        return p

    def forward(self, images, captions, lengths):
        """model2.py:38-65: logits f32 [sum(lengths), V], rows in time-major packed order."""
        self.dropout_plan(sampling=self.training and self.ss_prob > 0)        # refuse before the conv stack runs
        feats, fmean = self._encode(images)
        return self.decode(feats, fmean, captions, lengths)

    def decode(self, features, fmean, captions, lengths):
        """The decoder half of `forward`.  In training mode with ss_prob > 0 the embedding half of the input of step t >= 1 is,
        with probability ss_prob, a token drawn from softmax(logits of step t-1) (scheduled sampling; seed drawn from torch's CPU
        generator); the tokens fed and the seed are kept as `last_ss_inputs` / `last_ss_seed`.

        Every call leaves `last_alphas`, the attention maps as the packed [N, P] tape (detached, no copy; row n belongs to the
        logits' row n).  With `alpha_c > 0` it also leaves `last_attention_penalty`, a 0-dim tensor WITH a graph equal to
        alpha_c * mean_{b,p} (1 - sum_t alpha[b,t,p])^2 (doubly stochastic attention), None otherwise; a training loop adds it:
        `loss = criterion(out, targets) + model.last_attention_penalty`.  The mean is over this call's B images: under data
        parallelism B is the rank's own batch.

        In training mode with `dropout_p` > 0 the output layer's Z is dropped in front of the classifier; the mask's seed (one
        `draw_ss_seed()`) stays on `last_dropout_seed`.  Together with ss_prob > 0 that raises NotImplementedError."""
        p_drop = self.dropout_plan(sampling=self.training and self.ss_prob > 0)
        L.require_gpu(captions, "captions")
        if len(lengths) != features.shape[0]:
            raise ValueError("len(lengths) != batch size")
        pi = PackInfo.get(lengths, features.device)
        if pi.T > captions.shape[1]:
            raise ValueError("a length exceeds captions.shape[1]")
        if captions.dtype != torch.int64 or captions.stride(1) != 1:
            captions = captions.long().contiguous()
        if self._guard is None or self._guard.status.device != features.device:
            self._guard = IdGuard(features.device)
        self._guard.submit(captions, pi.T, self.vocab_size, "captions")
        ss = None
        if self.training and self.ss_prob > 0:
            ss = dict(prob=float(self.ss_prob), seed=draw_ss_seed(), rank=int(self.ss_rank))
        ex = dict(alpha_c=float(self.alpha_c))
        if p_drop is not None:
            self.last_dropout_seed = draw_ss_seed()
            ex["dropout"] = (p_drop, self.last_dropout_seed, int(self.ss_rank))
        out = _AttendFn.apply(self, features, fmean, captions, pi, ss, ex, *self._params())
        self.last_attention_penalty = None
        if ex["alpha_c"] > 0:
            out, self.last_attention_penalty = out
        self.last_alphas = ex.get("alphas")
        if ss is not None:
            self.last_ss_inputs, self.last_ss_seed = ss["used"], ss["seed"]
        return out

    def rollout(self, features, fmean, steps=20, greedy=False, start_id=1, num_samples=1):
        """The decoder half of `forward` fed its OWN tokens (self-critical sequence training, Rennie et al. 2017): step 0 takes
        <start>, step t >= 1 the token of step t-1 -- a DRAW from softmax(logits of step t-1), or with `greedy` their arg-max.
        Returns (ids i64 [B, steps], logits f32 [steps * B, V]), logits row t * B + b those of step t of row b.  One
        `sat_rollout_attend_fwd` call, nothing read back.  Training mode only.

        Sampled: the logits carry autograd -- their backward is the teacher-forced backward on the tokens fed, which stay as
        `last_rollout_inputs` ([B, steps] = [start_id | ids[:, :steps-1]]).  The seed comes from torch's CPU generator
        (`draw_ss_seed`) and is kept as `last_rollout_seed`; the draws are `ss_rank`'s stream.  Rows keep running behind their
        <end>: `scst_loss` masks them.

        greedy=True: no graph (the logits come back detached), no seed consumed, `last_rollout_seed` untouched.  This is the
        arg-max decode of the policy the draws come from -- h0 / c0 from init_lstm and every step its own context -- and so the
        baseline of a self-critical loss; `sample()` keeps model2.py:91-111's zero state and lagging context and is another decode.

        Either way `last_alphas` is the packed [steps * B, P] attention tape: `.view(steps, B, P)` is where the model looked for
        each word it emitted.  `ss_prob` and `alpha_c` do not act on a rollout, and `last_attention_penalty` is set to None:
        `sat_attention_coverage` counts every step a row is alive in, and here every row is alive behind its <end>, so the penalty
        would pull the maps of steps the loss masks towards covering the image.  (A length-masked penalty is a separate change.)

        num_samples = S > 1 (sampled only; with greedy=True a ValueError, an arg-max decode has one answer): S captions per image.
        features and fmean are repeated to R = B * S rows (row r = b * S + s) and the same call runs on R rows with draw row r: ids
        [B, S, steps], logits [steps * R, V] with row t * R + r, `last_rollout_inputs` [R, steps] and `last_alphas` [steps * R, P]
        -- bit for bit the rollout of the inputs repeated by hand.  The attention encoding of the features is computed once per
        image and repeated (`_context_encode_group`); the repeated features and their encoding are S x [B, P, C] each while the
        graph lives.  The R-row gradients of features and fmean come back summed per image (`sat_group_sum_rows`)."""
        S = check_group(num_samples)[0]
        if greedy and S > 1:
            raise ValueError("rollout(greedy=True) is an arg-max decode, which has one answer per image: num_samples must be 1")
        if not self.training:
            raise RuntimeError("ShowAttendTellModel.rollout is a training forward (model.train()); eval mode decodes with sample()")
        self.dropout_plan(sampling=True, what="a rollout")
        L.require_gpu(features, "features")
        L.require_gpu(fmean, "fmean")
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        if features.dtype != torch.float32 or fmean.dtype != torch.float32:
            raise TypeError("features and fmean must be float32")
        features, fmean = features.contiguous(), fmean.contiguous()
        out = {}
        if S > 1:
            out["group"] = (features.detach(), S)
            features, fmean = repeat_rows(features, S), repeat_rows(fmean, S)
        if greedy:
            with torch.no_grad():
                logits = _AttendRolloutFn.apply(self, features, fmean, steps, True, int(start_id), 0, 0, out, *self._params())
        else:
            seed = draw_ss_seed()
            logits = _AttendRolloutFn.apply(self, features, fmean, steps, False, int(start_id), seed, int(self.ss_rank), out,
                                            *self._params())
            self.last_rollout_seed = seed
        self.last_rollout_inputs, self.last_alphas, self.last_attention_penalty = out["fed"], out["alphas"], None
        ids = out["ids"]
        return (ids if S == 1 else ids.view(-1, S, steps)), logits

    def scst_forward(self, images, image_index, scorer, end_id=2, steps=20, num_samples=1, baseline="greedy"):
        """The self-critical loss of one batch (`scst.SelfCritical.attend`) behind the conv stack: sampled rollout, arg-max rollout
        of the same policy as the baseline, CIDEr of both, weighted cross entropy.  image_index: the corpus image of every row, as
        for `CiderScorer.score`.  With `finetune(allow=True)` `loss.backward()` also reaches the conv stack.  The `SelfCritical`
        object (its last_reward, last_baseline, last_ids, last_greedy_ids) is kept as `last_scst`.  num_samples, baseline:
        `SelfCritical`'s -- S sampled captions per image from ONE pass of the conv stack, baseline "greedy" or "sample_mean"
        (leave-one-out: no arg-max rollout)."""
        self.dropout_plan(sampling=True, what="a rollout (scst_forward)")     # refuse before the conv stack runs
        check_group(num_samples, baseline)
        feats, fmean = self._encode(images)
        self.last_scst = SelfCritical(scorer, end_id, num_samples=num_samples, baseline=baseline)
        return self.last_scst.attend(self, feats, fmean, image_index, steps)

    @torch.no_grad()
    def score_captions(self, images, captions, lengths, *, cross=False, normalize="none", return_tokens=False):
        """The log-probability of GIVEN captions (`score.CaptionScores`), one image per caption: `score_captions_features` behind
        the encoder."""
        if cross:
            raise NotImplementedError("cross scoring for Show-Attend-Tell is out of scope: score pairs (cross=False)")
        feats, fmean = self._encode(images)
        return self.score_captions_features(feats, fmean, captions, lengths, normalize=normalize, return_tokens=return_tokens)

    @torch.no_grad()
    def score_captions_features(self, features, fmean, captions, lengths, *, cross=False, normalize="none", return_tokens=False):
        """... given the features [C, P, F] and their mean (`_encode`).  Scored tokens are the ones the model is trained on
        (train.py:134-139): captions[:, 1:] with lengths - 1, so `lengths` (a Python list, ANY order, each >= 2) count the
        `<start>` that is fed but not scored, and `length` of the result is lengths - 1.  The logits come from `decode`, the
        model's own forward (a fixed, affordable size here), then `sat_ce_rows` without a gradient and `sat_caption_logp_sum`.
        Eval or train mode, and as `DecoderRNN.score_captions` never with dropout or scheduled sampling: the forward runs as in
        eval mode.  Paired only: cross=True raises NotImplementedError."""
        from .score import attend_score_captions_features
        return attend_score_captions_features(self, features, fmean, captions, lengths, cross=cross, normalize=normalize,
                                              return_tokens=return_tokens)

    @torch.no_grad()
    def sample(self, images, states=None, return_alphas=False):
        """Greedy search, 20 steps (model2.py:91-111; torch-0.1 keepdim semantics): i64 [B,20].  `states`: None = zeros (what
        eval.py:82-83 passes), a (h, c) pair of [B,H] tensors, or eval.py:89's stacked [2,B,H] tensor.  return_alphas: also the
        attention maps f32 [B, 20, P] -- where the model looked for each word."""
        feats, _ = self._encode(images)
        if return_alphas:
            ids, alphas = self.sample_features(feats, states, return_alphas=True)
            return ids.squeeze(), alphas
        return self.sample_features(feats, states).squeeze()      # model2.py:111: [20] at batch 1

    @torch.no_grad()
    def sample_features(self, features, states=None, steps=20, start_id=1, return_alphas=False):
        """`sample` given the features [B, P, C]: `_EvalDecoder.run` on B rows, `sat_vocab_argmax` picks each step's token."""
        d = _EvalDecoder(self, features, states, 1, steps, start_id, return_alphas)
        lib, st, cls = d.lib, L.stream(), self.classifier
        B, P, C, E, H, V = d.dims
        ids = torch.full((B, steps), int(start_id), dtype=torch.int64, device=features.device)
        wsb = lib.sat_vocab_argmax_ws_bytes(B, V)
        ws = torch.empty(wsb // 4, device=features.device)

        def pick(i):
            col = ids[:, i]
            L.check(lib.sat_vocab_argmax(L.ptr(d.Z), L.ptr(cls.weight), L.ptr(cls.bias), B, E, V, col.data_ptr(), ids.stride(0),
                                         L.ptr(ws), wsb, st), "sat_vocab_argmax")
            return col.data_ptr(), ids.stride(0), d.ctxb

        d.run(pick)
        return (ids, d.maps((B,))) if return_alphas else ids

    @torch.no_grad()
    def sample_stochastic(self, images, states=None, *, suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False,
                          repetition_penalty=1.0, end_id=None, **kw):
        """`sample_stochastic_features` behind the conv stack, its constraints included (arguments checked before it runs)."""
        check_sample_args(kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0), kw.get("num_samples", 1), kw.get("seed"))
        cons = dict(suppress_ids=suppress_ids, min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size,
                    block_repeat=block_repeat, repetition_penalty=repetition_penalty, end_id=end_id)
        if check_sample_constraints(vocab_size=self.vocab_size, steps=kw.get("steps", 20), **cons).active:
            kw.update(cons)
        feats, _ = self._encode(images)
        return self.sample_stochastic_features(feats, states, **kw)

    @torch.no_grad()
    def sample_stochastic_features(self, features, states=None, steps=20, start_id=1, temperature=1.0, top_k=0, top_p=1.0,
                                   num_samples=1, seed=None, return_logprobs=False, return_logits=False, return_alphas=False, *,
                                   suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False,
                                   repetition_penalty=1.0, end_id=None):
        """`sample_features` with a DRAW where it takes the arg-max: every step's token comes from softmax(logits / temperature)
        restricted to the top_k most likely tokens (0: all) and then to the nucleus, the shortest most-likely-first prefix holding
        top_p of the remaining mass (1: all).  The loop is `sample_features`' own -- `_EvalDecoder.step`, the classifier as one
        exact-f32 GEMM, `sat_sample_filtered` with t = the step, `_EvalDecoder.feed` -- with model2.py:91-111's zero state and
        lagging context, so top_k=1 decodes what `sample` decodes (up to ties between logits).  No tapes; eval or train mode.

        Returns ids i64 [B, steps], or [B, S, steps] with num_samples = S > 1 (features and states repeated per image, draw row
        b * S + s).  Then, in this order, as asked: return_logprobs a dict(logp f32, kept i32) shaped like ids; return_logits the
        exact-f32 logits [steps, B*S, V]; return_alphas the attention maps f32 [B, steps, P] ([B, S, steps, P]).  seed=None takes
        `draw_ss_seed()`; the seed used stays on `last_sample_seed`; the draws are `ss_rank`'s stream.
        Constraints as `DecoderRNN.sample_stochastic` documents them (all off by default: the calls are then the ones above): the
        draw of every step is `sat_sample_filtered_ex` with the ids drawn so far as the prefix; at most 64 steps."""
        tau, top_k, top_p, S, seed = check_sample_args(temperature, top_k, top_p, num_samples, seed)
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        cons = check_sample_constraints(suppress_ids, min_length, no_repeat_ngram_size, block_repeat, repetition_penalty, end_id,
                                        self.vocab_size, steps)
        d = _EvalDecoder(self, features, states, S, steps, start_id, return_alphas)
        lib, st, dev, cls = d.lib, L.stream(), features.device, self.classifier
        R, P, C, E, H, V = d.dims
        if seed is None:
            seed = draw_ss_seed()
        ids = torch.full((R, steps), int(start_id), dtype=torch.int64, device=dev)
        ldl = L.pad4(V)
        logits = torch.zeros(steps if return_logits else 1, R, ldl, device=dev)
        logp = torch.empty(steps, R, device=dev) if return_logprobs else None
        kept = torch.empty(steps, R, dtype=torch.int32, device=dev) if return_logprobs else None
        wsb = lib.sat_sample_filtered_ws_bytes(R, V)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def pick(i):
            lg, col = logits[i if return_logits else 0], ids[:, i]
            L.check(lib.sat_vocab_logits_fwd(L.ptr(d.Z), L.ptr(cls.weight), L.ptr(cls.bias), R, E, V, lg.data_ptr(), ldl, st),
                    "sat_vocab_logits_fwd")
            head = (lg.data_ptr(), ldl, R, V, tau, top_k, top_p, seed, i, int(self.ss_rank), col.data_ptr(), ids.stride(0),
                    logp[i].data_ptr() if return_logprobs else None, kept[i].data_ptr() if return_logprobs else None)
            if cons.active:
                L.check(lib.sat_sample_filtered_ex(*head, cons.struct(dev), ids.data_ptr(), ids.stride(0), L.ptr(ws), wsb, st),
                        "sat_sample_filtered_ex")
            else:
                L.check(lib.sat_sample_filtered(*head, L.ptr(ws), wsb, st), "sat_sample_filtered")
            return col.data_ptr(), ids.stride(0), d.ctxb

        d.run(pick)
        self.last_sample_seed = seed
        lead = (R // S, S) if S > 1 else (R,)
        return stochastic_result(ids.view(lead + (steps,)),
                                 dict(logp=logp.t().contiguous().view(lead + (steps,)),
                                      kept=kept.t().contiguous().view(lead + (steps,))) if return_logprobs else None,
                                 logits[:, :, :V] if return_logits else None, d.maps(lead) if return_alphas else None)

    @torch.no_grad()
    def sample_beam_features(self, features, beam_size=5, states=None, end_id=None, steps=20, start_id=1, return_all=False,
                             return_alphas=False, *, suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False,
                             length_penalty=0.0, num_beam_groups=1, diversity_penalty=0.0):
        """Beam search over `sample`'s loop (model2.py:91-111; the reference's `sample_beam` is a stub, model2.py:113-114, so parity
        is pinned only at beam_size=1 == the greedy goldens).  Rows are (image b, hypothesis k) = b*K + k: the features and their
        attention encoding are replicated per hypothesis once (data movement), every step is `_EvalDecoder.step` on B*K rows,
        `sat_beam_step` keeps the best K of the K*V candidates per image, and h, c and the carried context follow their parent
        (`sat_beam_gather_rows`).  Returns ids i64 [B,steps] of the best hypothesis (return_all: ids [B,K,steps] best-first, scores).
        return_alphas: the attention maps follow as the last value -- [B,steps,P] of the best hypothesis, with return_all
        [B,K,steps,P] best-first.  Every step's maps are recorded per slot and `sat_beam_backtrack_rows` follows the parent chain:
        the map of a step belongs to the slot its survivor was expanded from.
        Constraints as `DecoderRNN.sample_beam` documents them (all off by default: the calls are then the ones above): every step
        is `sat_beam_step_ex` over this loop's own (parents, tokens) records, and `sat_beam_rerank` re-orders ids, scores and maps
        once the search is over; `last_beam_norm_scores` / `last_beam_order` [B,K] as there.
        Beam groups as `DecoderRNN.sample_beam` documents them: with num_beam_groups > 1 the first slot of every group starts live,
        every step is `sat_beam_step_groups`, the rerank always runs (maps included) and `last_beam_groups` is set."""
        cons = check_beam_constraints(suppress_ids, min_length, no_repeat_ngram_size, block_repeat, length_penalty, end_id,
                                      self.vocab_size, steps)
        G, lam = check_beam_groups(beam_size, num_beam_groups, diversity_penalty)
        K = int(beam_size)
        if K < 1 or K > 8:
            raise ValueError("beam_size must be in 1..8")
        d = _EvalDecoder(self, features, states, K, steps, start_id, return_alphas)
        lib, st, dev, cls = d.lib, L.stream(), features.device, self.classifier
        R, P, C, E, H, V = d.dims
        B = R // K
        c2, ctx2 = torch.empty(R, H, device=dev), torch.empty(R, C, device=dev)
        ldl = L.pad4(V)
        logits = torch.zeros(R, ldl, device=dev)
        scores = torch.full((B, K), float("-inf"), device=dev)
        scores[:, ::K // G] = 0.0                        # the first slot of every group (one group: hypothesis 0)
        scores2 = torch.empty(B, K, device=dev)
        bws = torch.empty(lib.sat_beam_step_ws_bytes(B, K), dtype=torch.uint8, device=dev)
        parents = torch.empty(steps, R, dtype=torch.int32, device=dev)
        tokens = torch.empty(steps, R, dtype=torch.int64, device=dev)
        eid = -1 if end_id is None else int(end_id)
        cstruct = cons.struct(dev) if cons.active else None
        if self.last_beam_order is not None:
            self.last_beam_norm_scores = self.last_beam_order = self.last_beam_groups = None

        def pick(i):
            nonlocal scores, scores2, c2
            L.check(lib.sat_vocab_logits_fwd(L.ptr(d.Z), L.ptr(cls.weight), L.ptr(cls.bias), R, E, V, L.ptr(logits), ldl, st),
                    "sat_vocab_logits_fwd")
            last = tokens[i - 1].data_ptr() if (i > 0 and eid >= 0) else None
            if G > 1:
                L.check(lib.sat_beam_step_groups(L.ptr(logits), ldl, L.ptr(scores), last, eid, B, K, V, cstruct, L.ptr(parents),
                                                 L.ptr(tokens), i, steps, G, lam, parents[i].data_ptr(), tokens[i].data_ptr(),
                                                 L.ptr(scores2), L.ptr(bws), bws.numel(), st), "sat_beam_step_groups")
            elif cstruct is not None:
                L.check(lib.sat_beam_step_ex(L.ptr(logits), ldl, L.ptr(scores), last, eid, B, K, V, cstruct, L.ptr(parents), L.ptr(tokens),
                                             i, steps, parents[i].data_ptr(), tokens[i].data_ptr(), L.ptr(scores2), L.ptr(bws),
                                             bws.numel(), st), "sat_beam_step_ex")
            else:
                L.check(lib.sat_beam_step(L.ptr(logits), ldl, L.ptr(scores), last, eid, B, K, V, parents[i].data_ptr(),
                                          tokens[i].data_ptr(), L.ptr(scores2), L.ptr(bws), bws.numel(), st), "sat_beam_step")
            scores, scores2 = scores2, scores
            src_ctx = d.ctxb
            if K > 1:                                    # the survivors' state: h, c and THIS step's context follow their parent
                for (a, b_) in ((d.h, d.h2), (d.c, c2)):
                    L.check(lib.sat_beam_gather_rows(L.ptr(a), parents[i].data_ptr(), B, K, H, L.ptr(b_), st), "sat_beam_gather_rows")
                d.h, d.h2, d.c, c2 = d.h2, d.h, c2, d.c
                L.check(lib.sat_beam_gather_rows(L.ptr(d.ctxb), parents[i].data_ptr(), B, K, C, L.ptr(ctx2), st), "sat_beam_gather_rows")
                src_ctx = ctx2
            return tokens[i].data_ptr(), 1, src_ctx

        d.run(pick)
        ids = torch.empty(B, K, steps, dtype=torch.int64, device=dev)
        L.check(lib.sat_beam_backtrack(L.ptr(parents), L.ptr(tokens), steps, B, K, L.ptr(ids), st), "sat_beam_backtrack")
        order = None
        if cstruct is not None or G > 1:                 # the K results of an image by score / length^alpha (alpha 0: by score)
            ids2, ranked = torch.empty_like(ids), torch.empty(B, K, device=dev)
            norm, order = torch.empty(B, K, device=dev), torch.empty(B, K, dtype=torch.int32, device=dev)
            L.check(lib.sat_beam_rerank(L.ptr(ids), L.ptr(scores), B, K, steps, eid, cons.length_penalty, L.ptr(ids2), L.ptr(ranked),
                                        L.ptr(norm), L.ptr(order), st), "sat_beam_rerank")
            ids, scores = ids2, ranked
            self.last_beam_norm_scores, self.last_beam_order = norm, order
            if G > 1:
                self.last_beam_groups = order // (K // G)
        if return_alphas:
            alphas = torch.empty(B, K, steps, P, device=dev)
            L.check(lib.sat_beam_backtrack_rows(L.ptr(parents), L.ptr(d.amaps), steps, B, K, P, L.ptr(alphas), st), "sat_beam_backtrack_rows")
            if order is not None and (cons.length_penalty > 0 or G > 1):      # the maps follow their hypothesis
                ranked_maps = torch.empty_like(alphas)
                L.check(lib.sat_beam_gather_rows(L.ptr(alphas), L.ptr(order), B, K, steps * P, L.ptr(ranked_maps), st),
                        "sat_beam_gather_rows")
                alphas = ranked_maps
            if return_all:
                return ids, scores, alphas
            return ids[:, 0].contiguous(), alphas[:, 0].contiguous()
        if return_all:
            return ids, scores
        return ids[:, 0].contiguous()

    @torch.no_grad()
    def sample_beam(self, images, beam_size=5, states=None, end_id=None, return_all=False, return_alphas=False, *, suppress_ids=None,
                    min_length=0, no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0, num_beam_groups=1,
                    diversity_penalty=0.0):
        """`sample_beam(images, ...)`: the method the reference leaves as a stub (model2.py:113-114); BASELINE configs[4] asks beam 5.
        Constraints and beam groups as `sample_beam_features` (checked before the encoder runs)."""
        cons = dict(suppress_ids=suppress_ids, min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size,
                    block_repeat=block_repeat, length_penalty=length_penalty)
        check_beam_constraints(end_id=end_id, vocab_size=self.vocab_size, **cons)
        if check_beam_groups(beam_size, num_beam_groups, diversity_penalty)[0] > 1:
            cons.update(num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty)
        feats, _ = self._encode(images)
        return self.sample_beam_features(feats, beam_size, states, end_id, return_all=return_all, return_alphas=return_alphas, **cons)
