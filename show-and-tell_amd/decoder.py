"""The decoder's host pass (models.py:49-53 and its backward), shared by the autograd path (`models.DecoderRNN.forward`) and the
fused step (`trainer.TrainStep`): `decoder_forward`, `decoder_backward` and the owner of the LSTM workspaces, `LSTMWorkspaces`.
Parameters and gradients are keyed by the decoder's own parameter names (`embed.weight`, `lstm.weight_ih_l0`, ..., `linear.bias`)."""
import collections
import ctypes as C

import torch

from . import _lib as L
from .pack import PackInfo
from .watch import ResidencyWatch

LSTM_NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")

# the bf16 throughput mode's projection + cross entropy (train.py:143) as one call, `sat_vocab_ce_fwd_bf16`: targets i64 [N],
# inv_denom the loss scale, row_loss f32 [N], loss_out the 1-element loss slot, ws the uint8 workspace that keeps
# d(loss)/d(logits) (bf16) for the backward's `sat_vocab_ce_bwd_bf16`.  smoothing > 0: label smoothing, `sat_vocab_ce_fwd_bf16_ls`, with
# the plain NLL of the rows in row_nll f32 [N] and their scaled sum in nll_out f32 [1]; with 0 those two are not touched.
# alpha > 0: the unlikelihood term on top, `sat_vocab_ce_fwd_bf16_ul` over the pack layout of the call, with the rows' unweighted
# terms in row_ul f32 [N] and their scaled sum in ul_out f32 [1] (row_nll / nll_out are then written too)
VocabCE = collections.namedtuple("VocabCE", "targets inv_denom row_loss loss_out ws smoothing row_nll nll_out alpha row_ul ul_out",
                                 defaults=(0.0, None, None, 0.0, None, None))


def lstm_layers(params):
    """(w_ih, w_hh, b_ih, b_hh) of every LSTM layer in `params` (nn.LSTM's names)"""
    layers = []
    while "lstm.weight_ih_l%d" % len(layers) in params:
        layers.append(tuple(params["lstm.%s_l%d" % (n, len(layers))] for n in LSTM_NAMES))
    return layers


class LSTMWorkspaces:
    """The LSTM workspaces of a decoder on ONE stream (two streams must never share an exchange region).  Per layer: the forward
    one (re-zeroed by the library on every call) and, from the first backward on, the FULL backward one, sized with
    `sat_lstm_bwd_ws_bytes_max` for the widest batch seen (its exchange region and status word sit at (B, H)-only offsets).  They
    are replaced only for another batch size or layer shapes, or a wider batch; every backward buffer dropped is announced to the
    library with `sat_lstm_ws_release`.  watch=True (autograd): each call's status word goes to `watch.ResidencyWatch`;
    watch=False (`TrainStep`): the caller folds `fault_words` (pointer array, count) into its step's fault flag."""

    def __init__(self, device, watch):
        self.device, self.watch = device, watch
        self.key, self.n_max, self.fwd, self.bwd, self.fault_words = None, 0, [], [], None

    def fit(self, lib, B, T, dims, backward):
        """Serve a batch of B rows and T steps; dims: (In, H) per layer"""
        key = (B, tuple(dims))
        if key != self.key:
            fwd_off = [lib.sat_lstm_fwd_status_offset(B, H) for _, H in dims]          # -1: no persistent form
            if not self.watch and sum(o >= 0 for o in fwd_off) + len(dims) > 8:
                raise ValueError("at most 4 LSTM layers (8 status words per step)")
            self.release()
            self.key, self.fwd_off = key, fwd_off
            self.fwd = [torch.zeros(max(lib.sat_lstm_fwd_ws_bytes(B, H), 16), dtype=torch.uint8, device=self.device) for _, H in dims]
        if backward and B * T > self.n_max:
            self._release_bwd()
            self.n_max = B * T
            self.bwd = [torch.empty(lib.sat_lstm_bwd_ws_bytes_max(B * T, B, In, H), dtype=torch.uint8, device=self.device)
                        for In, H in dims]
            self.bwd_off = [lib.sat_lstm_bwd_status_offset(B * T, B, In, H) for In, H in dims]
            words = []
            for fws, fo, bws, bo in zip(self.fwd, self.fwd_off, self.bwd, self.bwd_off):
                words += [fws.data_ptr() + fo] if fo >= 0 else []
                bws[bo:bo + 64].zero_()                 # (read by the fault flag even when a call never runs persistently)
                words.append(bws.data_ptr() + bo)
            self.fault_words = ((C.c_void_p * len(words))(*words), len(words))

    def ran(self, l, backward):
        """behind layer l's sat_lstm_fwd / _bwd: a persistent recurrence (`sat_lstm_persist.hip`) whose wait ran out set the status
        word -- garbage outputs: the watch raises (at the latest one call later) after switching to one launch per step"""
        ws, off = (self.bwd[l], self.bwd_off[l]) if backward else (self.fwd[l], self.fwd_off[l])
        if self.watch and off >= 0:
            ResidencyWatch.get(self.device).submit(ws[off:off + 4].view(torch.int32), "the persistent LSTM recurrence",
                                                   lambda: L.load().sat_lstm_persist_enable(0))

    def ran_ss_fwd(self):
        """behind the scheduled-sampling loop, which runs no persistent recurrence: its forward status words report a clean run"""
        for ws, off in zip(self.fwd, self.fwd_off):
            if not self.watch and off >= 0:
                ws[off:off + 64].zero_()

    def _release_bwd(self):
        for ws in self.bwd:
            L.load().sat_lstm_ws_release(ws.data_ptr())      # (a later buffer at this address is cleared again)
        self.n_max, self.bwd, self.fault_words = 0, [], None

    def release(self):
        self._release_bwd()
        self.key, self.fwd = None, []

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


_AUTOGRAD_WS = {}


def autograd_workspaces(device, B, dims):
    """the autograd path's owner for (device, current stream, batch size, layer shapes): at most 16, least recently made first out"""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream, B, tuple(dims))
    ws = _AUTOGRAD_WS.get(key)
    if ws is None:
        if len(_AUTOGRAD_WS) >= 16:
            _AUTOGRAD_WS.pop(next(iter(_AUTOGRAD_WS))).release()
        ws = _AUTOGRAD_WS[key] = LSTMWorkspaces(device, watch=True)
    return ws


def _fit(lib, ws, dev, B, T, layers, backward):
    dims = [(w_ih.shape[1], w_hh.shape[1]) for w_ih, w_hh, _, _ in layers]
    if ws is None:
        ws = autograd_workspaces(dev, B, dims)
    ws.fit(lib, B, T, dims, backward)
    return ws


def _new_tapes(layers, N, B, E, dev, captions):
    """empty tapes of a forward over N packed rows: X[0] the layer-0 input, X[l + 1] layer l's h_t (HS), per layer (GA, CS, HP);
    and the per-layer cell state [B, H]"""
    tapes = {"X": [torch.empty(N, E, device=dev)], "layers": [], "captions": captions}
    cst = []
    for _, w_hh, _, _ in layers:
        H = w_hh.shape[1]
        tapes["layers"].append((torch.empty(N, 4 * H, device=dev), torch.empty(N, H, device=dev), torch.empty(N, H, device=dev)))
        tapes["X"].append(torch.empty(N, H, device=dev))
        cst.append(torch.empty(B, H, device=dev))
    return tapes, cst


def _step_loop_pointers(layers, tapes, cst):
    """the `lstm_w` and `tapes` arguments (lists of device pointers) of the calls that run the decoder step by step"""
    wflat = [t.data_ptr() for layer in layers for t in layer]
    ptrs = [t.data_ptr() for (GA, CS, HP), HS, c in zip(tapes["layers"], tapes["X"][1:], cst) for t in (GA, CS, HS, HP, c)]
    return wflat, ptrs


def dropout_rows(lib, t, p, seed, rank, site):
    """`sat_dropout_f32` in place on the dense f32 [rows, cols] tensor t (a tape in the forward, its gradient in the backward: the
    mask is a function of the arguments, include/sat_hip.h); nothing is launched for p == 0"""
    if p > 0:
        L.check(lib.sat_dropout_f32(L.ptr(t), t.stride(0), L.ptr(t), t.stride(0), t.shape[0], t.shape[1], float(p), int(seed),
                                    int(rank), int(site), L.stream()), "sat_dropout_f32")


def _layer_dropout(dropout, l, num_layers):
    """probability on the output of LSTM layer l (its site is l + 1): p_out on the top layer's, p_lstm on every other's"""
    return 0.0 if dropout is None else dropout[0 if l == num_layers - 1 else 1]


def rollout_forward(lib, features, params, steps, seed, rank, ws=None, logits=None):
    """The SAMPLED forward of self-critical training (`sat_rollout_decoder_fwd`, one library call): `steps` steps of all B rows, the
    input of step t >= 1 the token drawn from step t-1's logits.  Returns (ids i64 [B, steps], logits f32 [steps * B, pad4(V)],
    tapes, PackInfo of [steps] * B): the tapes are a teacher-forced forward's on ids[:, :steps-1], so `decoder_backward` applies.
    ws, logits: as for `decoder_forward`."""
    dev = features.device
    embed_w, lin_w, lin_b = params["embed.weight"], params["linear.weight"], params["linear.bias"]
    layers = lstm_layers(params)
    E, V = embed_w.shape[1], lin_w.shape[0]
    B, steps = features.shape[0], int(steps)
    if steps < 1:
        raise ValueError("steps must be >= 1")
    pi = PackInfo.get([steps] * B, dev)
    ws = _fit(lib, ws, dev, B, steps, layers, backward=False)
    ids = torch.empty(B, steps, dtype=torch.int64, device=dev)
    tapes, cst = _new_tapes(layers, pi.N, B, E, dev, ids[:, :steps - 1])
    if logits is None:
        logits = L.logits_buffer(pi.N, V, dev)
    wflat, ptrs = _step_loop_pointers(layers, tapes, cst)
    sws_bytes = lib.sat_rollout_decoder_fwd_ws_bytes(B, V)
    sws = torch.empty(max(sws_bytes // 4, 4), device=dev)
    L.check(lib.sat_rollout_decoder_fwd(L.ptr(features), L.ptr(embed_w), B, steps, E, V, (C.c_void_p * len(wflat))(*wflat), len(layers),
                                        layers[0][1].shape[1], L.ptr(lin_w), L.ptr(lin_b), (C.c_void_p * len(ptrs))(*ptrs),
                                        L.ptr(tapes["X"][0]), L.ptr(logits), logits.stride(0), int(seed), int(rank), ids.data_ptr(),
                                        ids.stride(0), L.ptr(sws), sws_bytes, L.stream()), "sat_rollout_decoder_fwd")
    ws.ran_ss_fwd()
    return ids, logits, tapes, pi


def decoder_forward(lib, features, params, captions, pi, ws=None, logits=None, ce=None, mixed_ws=None, ss=None, store_logits=True,
                    dropout=None):
    """embed+cat+pack -> L x LSTM -> vocab logits (models.py:49-53).  Returns (logits f32 [N, pad4(V)], tapes).
    params: the decoder's tensors by parameter name; ws: the `LSTMWorkspaces` of the calls (None: the autograd path's); logits:
    a buffer to fill (else a new one, `L.logits_buffer`); store_logits=False with `ss`: draws only, no f32 logits.
    ss: None (teacher forcing) or (prob, seed, rank): scheduled sampling (models.py:38 `ss_prob`, train.py:109-113) -- the input of
    step t >= 2 is, with probability prob, a token drawn from softmax(logits of step t-1) instead of captions[:, t-1]
    (`sat_ss_decoder_fwd`, one library call for the whole loop; the draws are functions of (seed, rank, row, step, token),
    include/sat_hip.h).  tapes["captions"] is then the tokens fed, i64 [B, T-1], so the backward is unchanged.
    ce: a `VocabCE`: the bf16 throughput mode's projection + CE (the loop above then draws without storing f32 logits);
    mixed_ws: workspace of the LSTM layers' batched GEMMs on the bf16 matrix pipe (teacher forcing).
    dropout: None or (p_out, p_lstm, seed, rank), teacher forcing only: layer l's output tape X[l + 1] is dropped IN PLACE behind
    the layer's call, with p_out for the top layer (in front of the projection) and p_lstm for the others (nn.LSTM(dropout=)),
    site l + 1.  In place is safe: the recurrence carries h through the HP tape, and X[l + 1] is read only by the next layer's
    batched input GEMMs and the projection, forward and backward -- all of which must see the dropped values.  The tuple stays in
    tapes["dropout"] for `decoder_backward`."""
    if dropout is not None and ss is not None:
        raise NotImplementedError("dropout inside the scheduled-sampling loop (sat_ss_decoder_fwd) is not built")
    dev = features.device
    embed_w, lin_w, lin_b = params["embed.weight"], params["linear.weight"], params["linear.bias"]
    layers = lstm_layers(params)
    E, V = embed_w.shape[1], lin_w.shape[0]
    N, T, B = pi.N, pi.T, pi.B
    st = L.stream()
    if captions.dtype != torch.int64 or captions.stride(1) != 1:
        captions = captions.long().contiguous()
    if captions.shape[1] < T - 1:
        raise ValueError("captions has %d columns but lengths need %d" % (captions.shape[1], T - 1))
    cap_ptr, cap_stride = (captions.data_ptr(), captions.stride(0)) if T > 1 else (None, 0)
    ws = _fit(lib, ws, dev, B, T, layers, backward=False)
    tapes, cst = _new_tapes(layers, N, B, E, dev, captions)
    tapes["dropout"] = dropout
    X = tapes["X"][0]
    if logits is None:
        logits = L.logits_buffer(N, V, dev)
    if ss is not None:
        prob, seed, rank = ss
        used = torch.empty(B, max(T - 1, 1), dtype=torch.int64, device=dev)[:, :T - 1]
        tapes["captions"] = used
        wflat, ptrs = _step_loop_pointers(layers, tapes, cst)
        sws_bytes = lib.sat_ss_decoder_fwd_ws_bytes(B, V)
        sws = torch.empty(max(sws_bytes // 4, 4), device=dev)
        L.check(lib.sat_ss_decoder_fwd(L.ptr(features), L.ptr(embed_w), cap_ptr, captions.stride(0), pi.bs_c, L.ptr(pi.prefix_dev),
                                       T, E, V, (C.c_void_p * len(wflat))(*wflat), len(layers), layers[0][1].shape[1], L.ptr(lin_w),
                                       L.ptr(lin_b), (C.c_void_p * len(ptrs))(*ptrs), L.ptr(X),
                                       L.ptr(logits) if store_logits and ce is None else None,
                                       logits.stride(0), float(prob), int(seed), int(rank), used.data_ptr() if T > 1 else None,
                                       used.stride(0), L.ptr(sws), sws_bytes, st), "sat_ss_decoder_fwd")
        ws.ran_ss_fwd()
    else:
        L.check(lib.sat_embed_concat_fwd(L.ptr(features), L.ptr(embed_w), cap_ptr, cap_stride, L.ptr(pi.prefix_dev),
                                         T, N, B, E, embed_w.shape[0], L.ptr(X), st), "sat_embed_concat_fwd")
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
            In, H = w_ih.shape[1], w_hh.shape[1]
            (GA, CS, HP), inp, HS = tapes["layers"][l], tapes["X"][l], tapes["X"][l + 1]
            fws, fwsb = ws.fwd[l], lib.sat_lstm_fwd_ws_bytes(B, H)
            args = (L.ptr(inp), L.ptr(w_ih), L.ptr(w_hh), L.ptr(b_ih), L.ptr(b_hh), pi.bs_c, T, In, H, L.ptr(GA), L.ptr(CS), L.ptr(HS),
                    L.ptr(HP), L.ptr(cst[l]), L.ptr(fws), fwsb)
            if mixed_ws is not None:          # bf16 throughput mode: the x-gates GEMM on the bf16 matrix pipe
                L.check(lib.sat_lstm_fwd_bf16(*args, L.ptr(mixed_ws), mixed_ws.numel(), st), "sat_lstm_fwd_bf16")
            else:
                L.check(lib.sat_lstm_fwd(*args, st), "sat_lstm_fwd")
            ws.ran(l, backward=False)
            if dropout is not None:
                dropout_rows(lib, HS, _layer_dropout(dropout, l, len(layers)), dropout[2], dropout[3], l + 1)
        if ce is None:
            L.check(lib.sat_vocab_logits_fwd(L.ptr(tapes["X"][-1]), L.ptr(lin_w), L.ptr(lin_b), N, lin_w.shape[1],
                                             V, L.ptr(logits), logits.stride(0), st), "sat_vocab_logits_fwd")
    if ce is not None:
        # bf16 throughput mode: the projection on the bf16 matrix pipe (f32 accumulate, f32 logits), CE in f32 from them,
        # d(loss)/d(logits) left as bf16 in the workspace for decoder_backward
        if ce.alpha > 0:
            L.check(lib.sat_vocab_ce_fwd_bf16_ul(L.ptr(tapes["X"][-1]), L.ptr(lin_w), L.ptr(lin_b), L.ptr(ce.targets), L.ptr(pi.prefix_dev),
                                                 pi.T, N, lin_w.shape[1], V, float(ce.inv_denom), float(ce.smoothing), float(ce.alpha),
                                                 L.ptr(logits), logits.stride(0), L.ptr(ce.row_loss), L.ptr(ce.row_nll),
                                                 L.ptr(ce.row_ul), L.ptr(ce.loss_out), L.ptr(ce.nll_out), L.ptr(ce.ul_out),
                                                 L.ptr(ce.ws), ce.ws.numel(), st), "sat_vocab_ce_fwd_bf16_ul")
        elif ce.smoothing > 0:
            L.check(lib.sat_vocab_ce_fwd_bf16_ls(L.ptr(tapes["X"][-1]), L.ptr(lin_w), L.ptr(lin_b), L.ptr(ce.targets), N, lin_w.shape[1],
                                                 V, float(ce.inv_denom), float(ce.smoothing), L.ptr(logits), logits.stride(0),
                                                 L.ptr(ce.row_loss), L.ptr(ce.row_nll), L.ptr(ce.loss_out), L.ptr(ce.nll_out),
                                                 L.ptr(ce.ws), ce.ws.numel(), st), "sat_vocab_ce_fwd_bf16_ls")
        else:
            L.check(lib.sat_vocab_ce_fwd_bf16(L.ptr(tapes["X"][-1]), L.ptr(lin_w), L.ptr(lin_b), L.ptr(ce.targets), N, lin_w.shape[1], V,
                                              float(ce.inv_denom), L.ptr(logits), logits.stride(0), L.ptr(ce.row_loss),
                                              L.ptr(ce.loss_out), L.ptr(ce.ws), ce.ws.numel(), st), "sat_vocab_ce_fwd_bf16")
    return logits, tapes


def decoder_backward(lib, dlogits, tapes, params, pi, grads, ws, on_stage=None, ce=None, mixed_ws=None):
    """Backward of decoder_forward.  `dlogits`: f32 [N, pad4(V)] with zero pad columns (unused with `ce`: the gradient is in
    ce.ws).  grads: preallocated f32 tensors to fill, by parameter name, plus "features"; ws: as decoder_forward's.
    on_stage(i) is called when gradient group i is final (0 vocab projection, 1 LSTM) -- the data-parallel
    wrapper launches that bucket's all-reduce there, under the remaining backward kernels.  With tapes["dropout"] the gradient of
    every dropped tape gets the same mask (regenerated, in place) before the layer that produced the tape reads it."""
    dev = dlogits.device
    st = L.stream()
    N, T, B = pi.N, pi.T, pi.B
    embed_w, lin_w = params["embed.weight"], params["linear.weight"]
    layers = lstm_layers(params)
    V, Hl = lin_w.shape
    dH = torch.empty(N, Hl, device=dev)
    if ce is not None:
        L.check(lib.sat_vocab_ce_bwd_bf16(N, Hl, V, L.ptr(grads["linear.weight"]), L.ptr(grads["linear.bias"]), L.ptr(dH), L.ptr(ce.ws),
                                          ce.ws.numel(), st), "sat_vocab_ce_bwd_bf16")
    else:
        vwsb = lib.sat_vocab_ce_bwd_ws_bytes(N, Hl, V)
        vws = torch.empty(max(vwsb // 4, 4), device=dev)
        L.check(lib.sat_vocab_ce_bwd(L.ptr(dlogits), dlogits.stride(0), L.ptr(tapes["X"][-1]), L.ptr(lin_w), N, Hl, V,
                                     L.ptr(grads["linear.weight"]), L.ptr(grads["linear.bias"]), L.ptr(dH), L.ptr(vws), vwsb, st),
                "sat_vocab_ce_bwd")
    if on_stage is not None:
        on_stage(0)
    ws = _fit(lib, ws, dev, B, T, layers, backward=True)
    dropout = tapes.get("dropout")
    for l in reversed(range(len(layers))):
        w_ih, w_hh, _, _ = layers[l]
        if dropout is not None:                 # dH is d(dropped X[l + 1]): back through the mask of site l + 1
            dropout_rows(lib, dH, _layer_dropout(dropout, l, len(layers)), dropout[2], dropout[3], l + 1)
        H, In = w_hh.shape[1], w_ih.shape[1]
        GA, CS, HP = tapes["layers"][l]
        DG = torch.empty(N, 4 * H, device=dev)
        dX = torch.empty(N, In, device=dev)
        dw_ih, dw_hh, db_ih, db_hh = (grads["lstm.%s_l%d" % (n, l)] for n in LSTM_NAMES)
        args = (L.ptr(dH), L.ptr(tapes["X"][l]), L.ptr(w_ih), L.ptr(w_hh), L.ptr(GA), L.ptr(CS), L.ptr(HP), pi.bs_c, T, In, H,
                L.ptr(DG), L.ptr(dw_ih), L.ptr(dw_hh), L.ptr(db_ih), L.ptr(db_hh), L.ptr(dX), L.ptr(ws.bwd[l]), ws.bwd[l].numel())
        if mixed_ws is not None:
            L.check(lib.sat_lstm_bwd_bf16(*args, L.ptr(mixed_ws), mixed_ws.numel(), st), "sat_lstm_bwd_bf16")
        else:
            L.check(lib.sat_lstm_bwd(*args, st), "sat_lstm_bwd")
        ws.ran(l, backward=True)
        dH = dX
    if on_stage is not None:
        on_stage(1)
    caps = tapes["captions"]
    cap_ptr, cap_stride = (None, 0) if T <= 1 else (caps.data_ptr(), caps.stride(0))
    L.check(lib.sat_embed_concat_bwd(L.ptr(dH), cap_ptr, cap_stride, L.ptr(pi.prefix_dev), T, N, B, embed_w.shape[1],
                                     embed_w.shape[0], L.ptr(grads["embed.weight"]), L.ptr(grads["features"]), st),
            "sat_embed_concat_bwd")
