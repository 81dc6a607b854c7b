"""Show-Attend-Tell behind the same boundary: `ShowAttendTellModel` with the reference's constructor,
`forward(images, captions, lengths)` and `sample(images, states)` (`/root/reference/model2.py:9-111`, the model
`train.py:37` constructs), every tensor op a libsat_hip.so kernel.

    encoder  : VGG16 `features[:-3]` (model2.py:15-16), frozen (model2.py:17, 87-89) -- the conv op program of the ResNet
               path (implicit-GEMM conv with the bias + ReLU riding in the bf16 conv epilogue, SAT_OP_MAXPOOL2)
    decoder  : context_encode = features @ image_att_w (sat_gemm_f32); init_lstm; per packed step: weight_hh projection,
               sat_attention_fwd (tanh / softmax / weighted mean, model2.py:73-78), sat_lstmcell_fwd (model2.py:58);
               output_layer batched over all packed rows after the loop (model2.py:80-85); in training with ss_prob > 0
               (scheduled sampling, train.py:109-113) the whole loop, output layer and Gumbel-max draws per step, is one
               `sat_ss_attend_fwd` call; `rollout` (self-critical training, `scst_forward`) feeds the decoder its own tokens --
               drawn, or the arg-max -- through the same per-step launches as one `sat_rollout_attend_fwd` call
    backward : hand-written (sat_attention_bwd, LSTMCell BPTT, batched weight-gradient GEMMs) behind torch.autograd, so
               `loss.backward()` (train.py:144) works unchanged; `finetune(allow=True)` (model2.py:87-89) adds the conv-stack
               backward (f32 mode): dgrad = the forward conv kernel on flipped weights, wgrad = split-K GEMMs over the flat
               zero-bordered pixel index, ReLU mask / max-pool routing kernels.

state_dict keys equal the reference's: `encoder.{0,2,5,...}.weight/bias`, `image_att_w`, `init_hidden.*`, `init_memory.*`,
`weight_hh.*`, `weight_att`, `embedding.weight`, `lstmcell.{weight_ih,weight_hh,bias_ih,bias_hh}`, `context2out.*`,
`hidden2tout.*`, `classifier.*`.  GPU only: there is no CPU fallback.
"""
import math
import os

import torch
import torch.nn as nn

from . import _lib as L
from . import tune as T
from .pack import PackInfo
from .program import act_op, avgpool, conv_op, image_prep, tdtype
from .watch import IdGuard

VGG16_FEATURES = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512]    # vgg16.features[:-3]


class _ConvB(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.cin, self.cout = cin, cout
        w = torch.empty(cout, cin, 3, 3)
        nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")          # torchvision vgg init
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(cout))


class VggFeatures(nn.Module):
    """`nn.Sequential(*list(vgg16.features)[:-3])` as a parameter tree with the same child names ("0", "2", "5", ...)."""

    def __init__(self, cfg=VGG16_FEATURES):
        super().__init__()
        self.cfg = list(cfg)
        i, c = 0, 3
        self.conv_names = []
        for v in self.cfg:
            if v == "M":
                i += 1
            else:
                self.add_module(str(i), _ConvB(c, v))
                self.conv_names.append(str(i))
                c, i = v, i + 2
        self.out_channels = c

    def convs(self):
        return [getattr(self, n) for n in self.conv_names]


class VggProgram:
    """Device buffers + sat_op array of the frozen VGG stack for one (batch, H, W, dtype): images f32 NCHW ->
    features f32 [N, P, C] (model2.py:44-45's view + transpose is the NHWC flattening) and their mean over P."""

    def __init__(self, stack, N, H, W, dtype, device):
        self.N, self.H, self.W, self.dtype, self.stack = N, H, W, dtype, stack
        td = tdtype(dtype)
        ch = 8 if dtype == L.SAT_BF16 else 4
        self.keep, ops = [], []

        def alloc(shape, dt=td, zero=False):
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dt, device=device)
            self.keep.append(t)
            return t

        # 3-channel input: zero-bordered NHWC image with the channels padded to one 16-byte chunk per pixel
        cpad = ch
        self.img_pad = alloc((N, H + 2, W + 2, cpad), zero=True)
        ops += image_prep(dtype, self.img_pad, N, H, W, 1, cout=cpad)
        x, h, w, c = self.img_pad, H, W, cpad
        first = True
        self.layers, self.run_id = [], 0            # (kind, ...) in forward order: the tapes of the backward
        self.wcopies = []                           # (conv, kernel-layout weight copy, bias copy, Cin): refresh_weights()
        ones = {}
        convs = iter(stack.convs())
        for v in stack.cfg:
            if v == "M":
                out = alloc((N, h // 2, w // 2, c))
                ops.append(L.op(L.OP_MAXPOOL2, dtype, in0=x, out=out, N=N, Hin=h, Win=w, Cout=c))
                self.layers.append(("pool", x, out, h, w, c))
                x, h, w = out, h // 2, w // 2
                continue
            conv = next(convs)
            wt = conv.weight.detach().to(device=device, dtype=torch.float32)
            if first:                                    # pad Cin 3 -> chunk width with zero weights
                wp = torch.zeros(v, cpad, 3, 3, device=device)
                wp[:, :3] = wt
                wt = wp
            wk = wt.permute(0, 2, 3, 1).contiguous().to(td).reshape(v, -1)
            bias = conv.bias.detach().to(device=device, dtype=torch.float32).clone()     # a copy: never an alias of the live parameter
            self.keep += [wk, bias]
            self.wcopies.append((conv, wk, bias, 3 if first else c))
            out = alloc((N, h, w, v))
            if v not in ones:
                ones[v] = alloc((v,), torch.float32)
                ones[v].fill_(1.0)
            cin = c
            # the first conv's border is in the image: no padding arithmetic in the kernel
            hin, win, pad = (h + 2, w + 2, 0) if first else (h, w, 1)
            if dtype == L.SAT_BF16:                      # bias + ReLU ride in the conv epilogue (out = relu(acc*1 + bias))
                ops.append(conv_op(dtype, x, wk, out, N, hin, win, cin, h, w, v, 3, 3, 1, pad, scale1=ones[v], shift1=bias, flags=1))
            else:                                        # f32 parity mode: conv, then the elementwise affine + ReLU kernel
                raw = alloc((N, h, w, v))
                ops.append(conv_op(dtype, x, wk, raw, N, hin, win, cin, h, w, v, 3, 3, 1, pad))
                ops.append(act_op(L.OP_BN_RELU, dtype, raw, out, N, h, w, v, scale0=ones[v], shift0=bias))
            self.layers.append(("conv", conv, x, out, h, w, cin, v, first))
            x, c, first = out, v, False
        self.P, self.C = h * w, c
        self.fmap = x
        self.fmean = alloc((N, c), torch.float32)
        ops.append(avgpool(dtype, x, self.fmean, h, w))
        self.features = self.fmap.view(N, self.P, c) if dtype == L.SAT_F32 else alloc((N, self.P, c), torch.float32)
        self.ops = (L.SatOp * len(ops))(*ops)
        self.n_ops = len(ops)
        if dtype == L.SAT_BF16:
            # kernel variant per conv geometry: the committed table, the geometry-only default for anything it does not name;
            # timing only on request (tune.py: SAT_AUTOTUNE=1 / force)
            missing = T.assign(self.ops, self.n_ops)
            if missing and T.mode() in ("time", "force"):
                scratch = alloc((4096,), torch.float32)
                L.check(L.load().sat_conv_autotune(self.ops, self.n_ops, 3, scratch.data_ptr(), scratch.numel() * 4, L.stream()),
                        "sat_conv_autotune")
                torch.cuda.synchronize()
                T.save(self.ops, self.n_ops)
            elif missing:
                T.defaults(self.ops, missing)

    @torch.no_grad()
    def refresh_weights(self):
        """Re-derive the kernel-layout copies ([Cout][KH][KW][Cin], the stack's dtype) and the bias copies from the live
        parameters IN PLACE: one strided cast-copy per conv, no rebuild, no re-tune.  Fine-tuning (model2.py:87-89) calls this
        before every forward: an optimizer that updates the parameters through raw pointers (`FusedClampAdam`) or in place
        (`torch.optim.Adam`) is then always seen, and forward and backward use the same weights."""
        for conv, wk, bias, cin in self.wcopies:
            v = wk.shape[0]
            wk.view(v, 3, 3, -1)[..., :cin].copy_(conv.weight.detach().permute(0, 2, 3, 1))
            bias.copy_(conv.bias.detach())

    def run(self, images):
        L.require_gpu(images, "images")
        if images.dtype != torch.float32 or tuple(images.shape) != (self.N, 3, self.H, self.W):
            raise ValueError("images must be float32 [%d,3,%d,%d]" % (self.N, self.H, self.W))
        images = images.contiguous()
        lib = L.load()
        self.ops[0].in0 = images.data_ptr()
        L.check(lib.sat_run_ops(self.ops, self.n_ops, L.stream()), "sat_run_ops")
        self.run_id += 1
        if self.dtype == L.SAT_BF16:
            L.check(lib.sat_cast_bf16_f32(self.fmap.data_ptr(), self.features.data_ptr(), self.features.numel(), L.stream()),
                    "sat_cast_bf16_f32")
        return self.features, self.fmean


def _vgg_backward(self, d_feats, d_fmean):
    """Gradient of the conv stack (f32 NHWC): per 3x3 conv layer the zero-bordered d(pre-activation) (`sat_pad_nhwc_f32` with the
    ReLU mask), the bias gradient (`sat_colsum_f32`), nine split-K GEMMs over the flat padded pixel index for the weight
    gradient, and the forward conv kernel on flipped weights for the input gradient; `sat_maxpool2_bwd_f32` for the pools.
    Returns [dW, db] per conv in forward order (parameter layout)."""
    lib, st = L.load(), L.stream()
    N = self.N
    dev = d_feats.device
    bf = self.dtype == L.SAT_BF16
    # bf16 stack (mixed precision, f32 master weights -- the parameters themselves): the forward ran on bf16 copies of the weights
    # and stored bf16 activations.  Backward: gradients travel between layers in f32; the input gradient runs on the bf16 matrix
    # pipe (the forward conv kernel on flipped bf16 weights over the bf16-rounded zero-bordered d(pre-activation)); the weight
    # gradient stays an exact-f32 split-K GEMM over f32 casts of the stored activations, so dW is accumulated in f32 from bf16
    # activations and f32 gradients, and the optimizer updates f32 masters.

    def f32_of(t):
        if not bf:
            return t
        o = torch.empty(t.shape, dtype=torch.float32, device=dev)
        L.check(lib.sat_cast_bf16_f32(t.data_ptr(), o.data_ptr(), t.numel(), st), "sat_cast_bf16_f32")
        return o
    dY = d_feats.contiguous().clone()                     # [N, P, C] == NHWC of the last map
    if d_fmean is not None:                               # fmean = mean over positions (model2.py:68)
        L.check(lib.sat_bcast_add_f32(d_fmean.contiguous().data_ptr(), N, self.P, self.C, 1.0 / self.P, dY.data_ptr(), st), "sat_bcast_add_f32")
    grads = {}
    for layer in reversed(self.layers):
        if layer[0] == "pool":
            _, x, out, h, w, c = layer
            x = f32_of(x)
            dX = torch.empty_like(x)
            L.check(lib.sat_maxpool2_bwd_f32(x.data_ptr(), dY.data_ptr(), N, h, w, c, dX.data_ptr(), st), "sat_maxpool2_bwd_f32")
            dY = dX
            continue
        _, conv, x, out, h, w, cin, cout, first = layer
        x, out = f32_of(x), f32_of(out)
        hp, wp = h + 2, w + 2
        npix = N * hp * wp
        dZp = torch.empty(npix, cout, device=dev)
        L.check(lib.sat_pad_nhwc_f32(dY.data_ptr(), out.data_ptr(), N, h, w, cout, 1, dZp.data_ptr(), st), "sat_pad_nhwc_f32")
        db = torch.empty(cout, device=dev)
        L.check(lib.sat_colsum_f32(dZp.data_ptr(), cout, npix, cout, db.data_ptr(), st), "sat_colsum_f32")
        # zero-bordered input with a margin of one padded row (+1 pixel) at both ends: a tap is a constant flat offset
        margin = wp + 1
        Xp = torch.zeros(npix + 2 * margin, cin, device=dev)
        inner = Xp.data_ptr() + margin * cin * 4
        if first:                                         # the stem's input is the already padded image
            L.check(lib.sat_rows_copy(x.data_ptr(), cin, None, 0, npix, npix, cin, inner, cin, st), "sat_rows_copy")
        else:
            L.check(lib.sat_pad_nhwc_f32(x.data_ptr(), None, N, h, w, cin, 1, inner, st), "sat_pad_nhwc_f32")
        tiles = ((cout + 63) // 64) * ((cin + 63) // 64)
        ks = max(1, min(64, 512 // tiles, npix // 256))
        slab = cout * cin
        wsl = torch.empty(ks * slab, device=dev)
        tap_out = torch.empty(cout, cin, device=dev)
        dWk = torch.empty(cout, 9 * cin, device=dev)
        for kh in range(3):
            for kw in range(3):
                shift = (kh - 1) * wp + (kw - 1)
                L.check(lib.sat_gemm_f32_splitk(2, 1, dZp.data_ptr(), cout, inner + shift * cin * 4, cin, wsl.data_ptr(), cin, None, None,
                                                cout, cin, npix, ks, slab, st), "sat_gemm_f32_splitk")
                L.check(lib.sat_sum_slabs_f32(wsl.data_ptr(), ks, slab, slab, tap_out.data_ptr(), st), "sat_sum_slabs_f32")
                L.check(lib.sat_rows_copy(tap_out.data_ptr(), cin, None, 0, cout, cout, cin, dWk.data_ptr() + (kh * 3 + kw) * cin * 4,
                                          9 * cin, st), "sat_rows_copy")
        dW = dWk.view(cout, 3, 3, cin)[..., :conv.cin].permute(0, 3, 1, 2).contiguous()       # kernel layout -> [Cout, Cin, 3, 3]
        grads[conv] = (dW, db)
        if first:
            break
        # input gradient = conv of the zero-bordered d(pre-activation) with the flipped, transposed weights (forward kernel)
        wflip = conv.weight.detach().flip(2, 3).permute(1, 2, 3, 0).contiguous().view(cin, 9 * cout)
        dX = torch.empty(N, h, w, cin, device=dev)
        if bf and cin % 8 == 0 and cout % 8 == 0:
            # input gradient on the bf16 matrix pipe: bf16 copies of dZp and of the flipped weights, bf16 result cast back to f32
            dZb = torch.empty(npix, cout, dtype=torch.bfloat16, device=dev)
            L.check(lib.sat_cast_f32_bf16(dZp.data_ptr(), dZb.data_ptr(), dZp.numel(), st), "sat_cast_f32_bf16")
            wfb = wflip.to(torch.bfloat16)
            dXb = torch.empty(N, h, w, cin, dtype=torch.bfloat16, device=dev)
            o = L.SatOp()
            o.kind, o.dtype = L.OP_CONV, L.SAT_BF16
            o.in0, o.w, o.out = dZb.data_ptr(), wfb.data_ptr(), dXb.data_ptr()
            o.N, o.Hin, o.Win, o.Cin, o.Hout, o.Wout, o.Cout = N, hp, wp, cout, h, w, cin
            o.KH, o.KW, o.stride, o.pad = 3, 3, 1, 0
            o.sN, o.sH, o.sW = hp * wp * cout, wp * cout, cout
            ops = (L.SatOp * 1)(o)
            L.check(lib.sat_run_ops(ops, 1, st), "sat_run_ops")
            L.check(lib.sat_cast_bf16_f32(dXb.data_ptr(), dX.data_ptr(), dX.numel(), st), "sat_cast_bf16_f32")
            dY = dX
            continue
        o = L.SatOp()
        o.kind, o.dtype = L.OP_CONV, L.SAT_F32
        o.in0, o.w, o.out = dZp.data_ptr(), wflip.data_ptr(), dX.data_ptr()
        o.N, o.Hin, o.Win, o.Cin, o.Hout, o.Wout, o.Cout = N, hp, wp, cout, h, w, cin
        o.KH, o.KW, o.stride, o.pad = 3, 3, 1, 0
        o.sN, o.sH, o.sW = hp * wp * cout, wp * cout, cout
        ops = (L.SatOp * 1)(o)
        L.check(lib.sat_run_ops(ops, 1, st), "sat_run_ops")
        dY = dX
    out = []
    for conv in self.stack.convs():
        out += list(grads[conv])
    return out


VggProgram.backward = _vgg_backward


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


_SKINNY_WS = {}
_SKINNY_ROWS = int(os.environ.get("SAT_SKINNY_ROWS", "128"))   # per-step GEMMs with at most this many rows take the split-K kernel


def _ptr(x):
    return x if isinstance(x, int) or x is None else x.data_ptr()


def _gemm(lib, amode, bmode, A, lda, B, ldb, Cout, ldc, M, N, K, bias=None, bias2=None):
    """C[M,N] = op(A) op(B) + bias (+ bias2).  A 64 x 64-tiled GEMM of a 64-row decode step runs on N/64 workgroups; those go to
    sat_skinny_gemm_f32, which splits K over waves and grid slices instead."""
    if amode == 0 and M <= _SKINNY_ROWS and bias2 is None and ldc == N and K % 4 == 0 and lda % 4 == 0 and (bmode == 1 or ldb % 4 == 0):
        need = lib.sat_skinny_gemm_ws_bytes(M, N, K)
        dev = torch.cuda.current_device()
        ws = _SKINNY_WS.get(dev)
        if ws is None or ws.numel() * 4 < need:
            ws = _SKINNY_WS[dev] = torch.empty(max(need // 4, 1 << 20), dtype=torch.float32, device="cuda")
        L.check(lib.sat_skinny_gemm_f32(_ptr(A), lda, _ptr(B), ldb, bmode, M, N, K, L.ptr(bias), _ptr(Cout), ldc,
                                        ws.data_ptr(), ws.numel() * 4, L.stream()), "sat_skinny_gemm_f32")
        return
    L.check(lib.sat_gemm_f32(amode, bmode, _ptr(A), lda, _ptr(B), ldb, _ptr(Cout), ldc, L.ptr(bias), L.ptr(bias2), M, N, K,
                             L.stream()), "sat_gemm_f32")


def _p(t, row0=0):
    """device pointer of row `row0` of a 2-D contiguous f32 tensor"""
    return t.data_ptr() + row0 * t.shape[1] * 4


class _AttendFn(torch.autograd.Function):
    """decoder half of model2.py:38-65 given the encoder features (the conv stack is frozen, model2.py:17)."""

    @staticmethod
    def forward(ctx, model, features, fmean, captions, pi, ss, ex, *params):
        """ss: None (teacher forcing) or dict(prob, seed, rank) -- scheduled sampling through `sat_ss_attend_fwd`; receives
        "used", the tokens fed [B, T].  ex: dict(alpha_c) -- receives "alphas", the packed [N, P] attention tape; with
        alpha_c > 0 the doubly stochastic penalty is a second output (`_attend_outputs`)."""
        lib = L.load()
        m = model
        dev = features.device
        st = L.stream()
        B, P, C = features.shape
        E, H, V, Hin = m.embed_size, m.hidden_size, m.vocab_size, m.hidden_size
        N, T = pi.N, pi.T
        f2 = features.view(B * P, C)
        ctx_enc = torch.empty(B * P, C, device=dev)
        _gemm(lib, 0, 1, f2, C, m.image_att_w, C, ctx_enc, C, B * P, C, C)                      # model2.py:46
        HSX = torch.empty(B + N, H, device=dev)            # [h_0 ; h of every packed row]: h_{t-1} of any row is one gather away
        h0, c0 = HSX[:B], torch.empty(B, H, device=dev)
        _gemm(lib, 0, 0, fmean, C, m.init_hidden.weight, C, h0, H, B, H, C, m.init_hidden.bias)  # model2.py:67-71
        _gemm(lib, 0, 0, fmean, C, m.init_memory.weight, C, c0, H, B, H, C, m.init_memory.bias)
        HS, PROJ = HSX[B:], torch.empty(N, C, device=dev)
        X, GATES = torch.empty(N, Hin, device=dev), torch.empty(N, 4 * H, device=dev)
        CS, ALPHA = torch.empty(N, H, device=dev), torch.empty(N, P, device=dev)
        if ss is not None:
            logits = _ss_attend_forward(ctx, lib, m, f2, fmean, ctx_enc, h0, c0, HSX, captions, pi, ss,
                                        dict(PROJ=PROJ, ALPHA=ALPHA, X=X, GATES=GATES, CS=CS, HS=HS))
            return _attend_outputs(ctx, lib, ex, logits, V)
        c = c0.clone()
        watt = m.weight_att.view(-1)
        att_ws = torch.empty(B * P, device=dev)
        # the embedding half of every step's LSTMCell input [emb | ctx] (model2.py:55-57) in one gather
        toks = torch.empty(N, dtype=torch.int64, device=dev)
        L.check(lib.sat_pack_tokens(captions.data_ptr(), captions.stride(0), pi.prefix_dev.data_ptr(), T, N, 0, toks.data_ptr(), st),
                "sat_pack_tokens")
        L.check(lib.sat_rows_copy(L.ptr(m.embedding.weight), E, toks.data_ptr(), 1, V, N, E, L.ptr(X), Hin, st), "sat_rows_copy")
        for t, bs in enumerate(pi.batch_sizes):                                                  # model2.py:54-62
            r0 = pi.prefix[t]
            hprev = h0.data_ptr() if t == 0 else _p(HS, pi.prefix[t - 1])
            _gemm(lib, 0, 0, hprev, H, m.weight_hh.weight, H, _p(PROJ, r0), C, bs, C, H, m.weight_hh.bias)
            # the context lands in its half of the LSTMCell input row (ld = Hin)
            L.check(lib.sat_attention_fwd(L.ptr(ctx_enc), L.ptr(f2), _p(PROJ, r0), C, L.ptr(watt), bs, P, C, _p(ALPHA, r0),
                                          _p(X, r0) + E * 4, Hin, att_ws.data_ptr(), att_ws.numel() * 4, st), "sat_attention_fwd")
            L.check(lib.sat_lstmcell_fwd(_p(X, r0), hprev, L.ptr(c), L.ptr(m.lstmcell.weight_ih), L.ptr(m.lstmcell.weight_hh),
                                         L.ptr(m.lstmcell.bias_ih), L.ptr(m.lstmcell.bias_hh), bs, Hin, H, _p(HS, r0),
                                         _p(GATES, r0), _p(CS, r0), st), "sat_lstmcell_fwd")
        # output_layer over all packed rows at once (model2.py:80-85): z = [ctx | h] [W_c2o | W_h2o]^T + b1 + b2
        Zin, Wz = torch.empty(N, C + H, device=dev), torch.empty(E, C + H, device=dev)
        L.check(lib.sat_rows_copy(X.data_ptr() + E * 4, Hin, None, 0, N, N, C, L.ptr(Zin), C + H, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(HS), H, None, 0, N, N, H, Zin.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(m.context2out.weight), C, None, 0, E, E, C, L.ptr(Wz), C + H, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(m.hidden2tout.weight), H, None, 0, E, E, H, Wz.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
        Z = torch.empty(N, E, device=dev)
        _gemm(lib, 0, 0, Zin, C + H, Wz, C + H, Z, E, N, E, C + H, m.context2out.bias, m.hidden2tout.bias)
        logits = L.logits_buffer(N, V, dev)
        ldl = logits.shape[1]
        _gemm(lib, 0, 0, Z, E, m.classifier.weight, E, logits, ldl, N, V, E, m.classifier.bias)
        ctx.m, ctx.pi, ctx.captions = m, pi, captions
        ctx.tapes = dict(f2=f2, fmean=fmean, ctx_enc=ctx_enc, h0=h0, c0=c0, PROJ=PROJ, HS=HS, X=X, GATES=GATES, CS=CS, ALPHA=ALPHA,
                         Zin=Zin, Wz=Wz, Z=Z, toks=toks, HSX=HSX)
        return _attend_outputs(ctx, lib, ex, logits, V)

    @staticmethod
    def backward(ctx, dlogits, *dpen):
        from .attend_bwd import attend_backward
        want = ctx.needs_input_grad[1]                     # features carry a graph only when the conv stack is fine-tuned
        extra = scale = None
        if ctx.cov_grad is not None:
            # the penalty's incoming gradient stays on the device (autograd hands zeros for an output the loss never used)
            extra, scale = ctx.cov_grad, dpen[0].to(torch.float32).contiguous()
        grads, d_feats, d_fmean = attend_backward(ctx.m, ctx.pi, ctx.captions, ctx.tapes, dlogits, want_dfeat=want,
                                                  d_alpha_extra=extra, d_alpha_scale=scale)
        return (None, d_feats, d_fmean if ctx.needs_input_grad[2] else None, None, None, None, None) + tuple(grads)


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


_SS_WEIGHTS = ("weight_hh.weight", "weight_hh.bias", "weight_att", "embedding.weight", "lstmcell.weight_ih", "lstmcell.weight_hh",
               "lstmcell.bias_ih", "lstmcell.bias_hh", "context2out.weight", "context2out.bias", "hidden2tout.weight",
               "hidden2tout.bias", "classifier.weight", "classifier.bias")      # include/sat_hip.h SAT_SSA_* order
_SS_TAPES = ("PROJ", "ALPHA", "X", "GATES", "CS", "HS", "Zin", "Z")                # SAT_SSA_PROJ .. SAT_SSA_Z


def _ss_attend_forward(ctx, lib, m, f2, fmean, ctx_enc, h0, c0, HSX, captions, pi, ss, tp):
    """the recurrence of _AttendFn.forward with scheduled sampling (model2.py:54-62 + 80-85 per step, the input of step t >= 1
    drawn from the logits of step t-1 with probability ss["prob"]): one `sat_ss_attend_fwd` call leaves the same tapes, so
    attend_backward runs unchanged on the tokens fed"""
    dev, st = f2.device, L.stream()
    B, P, C = pi.B, tp["ALPHA"].shape[1], f2.shape[1]
    E, H, V, N, T = m.embed_size, m.hidden_size, m.vocab_size, pi.N, pi.T
    tp["Zin"], tp["Z"] = torch.empty(N, C + H, device=dev), torch.empty(N, E, device=dev)
    Wz = torch.empty(E, C + H, device=dev)                 # [W_c2o | W_h2o]: the backward's dZin = dZ Wz
    L.check(lib.sat_rows_copy(L.ptr(m.context2out.weight), C, None, 0, E, E, C, L.ptr(Wz), C + H, st), "sat_rows_copy")
    L.check(lib.sat_rows_copy(L.ptr(m.hidden2tout.weight), H, None, 0, E, E, H, Wz.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
    named = dict(m.named_parameters())
    w = (L.C.c_void_p * len(_SS_WEIGHTS))(*[named[k].data_ptr() for k in _SS_WEIGHTS])
    tapes = (L.C.c_void_p * len(_SS_TAPES))(*[tp[k].data_ptr() for k in _SS_TAPES])
    toks = torch.empty(N, dtype=torch.int64, device=dev)
    used = torch.empty(B, T, dtype=torch.int64, device=dev)
    logits = L.logits_buffer(N, V, dev)
    ldl = logits.shape[1]
    wsb = lib.sat_ss_attend_fwd_ws_bytes(B, P, C, E, H, V)
    ws = torch.empty(wsb // 4, device=dev)
    L.check(lib.sat_ss_attend_fwd(f2.data_ptr(), ctx_enc.data_ptr(), h0.data_ptr(), c0.data_ptr(), captions.data_ptr(),
                                  captions.stride(0), pi.bs_c, pi.prefix_dev.data_ptr(), T, P, C, E, H, V, w, tapes, toks.data_ptr(),
                                  logits.data_ptr(), ldl, float(ss["prob"]), int(ss["seed"]), int(ss["rank"]), used.data_ptr(),
                                  used.stride(0), ws.data_ptr(), wsb, st), "sat_ss_attend_fwd")
    ss["used"] = used
    ctx.m, ctx.pi, ctx.captions = m, pi, captions
    ctx.tapes = dict(f2=f2, fmean=fmean, ctx_enc=ctx_enc, h0=h0, c0=c0, Wz=Wz, toks=toks, HSX=HSX, **tp)
    return logits


class _AttendRolloutFn(torch.autograd.Function):
    """The rollout of the decoder half (self-critical training): `sat_rollout_attend_fwd` feeds every step the token it took from
    the previous step's logits -- a draw, or the arg-max -- and leaves the tapes of the teacher-forced forward on those tokens, so
    the backward is `attend_backward` on `fed`."""

    @staticmethod
    def forward(ctx, model, features, fmean, steps, greedy, start_id, seed, rank, out, *params):
        """out: dict that receives "ids" [B, steps], "fed" [B, steps] (the tokens fed) and "alphas", the packed attention tape"""
        lib = L.load()
        m = model
        dev = features.device
        B, P, C = features.shape
        E, H, V = m.embed_size, m.hidden_size, m.vocab_size
        pi = PackInfo.get([steps] * B, dev)
        N = pi.N
        f2 = features.view(B * P, C)
        ctx_enc = torch.empty(B * P, C, device=dev)
        _gemm(lib, 0, 1, f2, C, m.image_att_w, C, ctx_enc, C, B * P, C, C)                      # model2.py:46
        HSX = torch.empty(B + N, H, device=dev)            # [h_0 ; h of every packed row], as in _AttendFn.forward
        h0, c0 = HSX[:B], torch.empty(B, H, device=dev)
        _gemm(lib, 0, 0, fmean, C, m.init_hidden.weight, C, h0, H, B, H, C, m.init_hidden.bias)  # model2.py:67-71
        _gemm(lib, 0, 0, fmean, C, m.init_memory.weight, C, c0, H, B, H, C, m.init_memory.bias)
        tp = dict(PROJ=torch.empty(N, C, device=dev), ALPHA=torch.empty(N, P, device=dev), X=torch.empty(N, H, device=dev),
                  GATES=torch.empty(N, 4 * H, device=dev), CS=torch.empty(N, H, device=dev), HS=HSX[B:],
                  Zin=torch.empty(N, C + H, device=dev), Z=torch.empty(N, E, device=dev))
        st = L.stream()
        Wz = torch.empty(E, C + H, device=dev)                 # [W_c2o | W_h2o]: the backward's dZin = dZ Wz
        L.check(lib.sat_rows_copy(L.ptr(m.context2out.weight), C, None, 0, E, E, C, L.ptr(Wz), C + H, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(m.hidden2tout.weight), H, None, 0, E, E, H, Wz.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
        named = dict(m.named_parameters())
        w = (L.C.c_void_p * len(_SS_WEIGHTS))(*[named[k].data_ptr() for k in _SS_WEIGHTS])
        tapes = (L.C.c_void_p * len(_SS_TAPES))(*[tp[k].data_ptr() for k in _SS_TAPES])
        toks = torch.empty(N, dtype=torch.int64, device=dev)
        ids = torch.empty(B, steps, dtype=torch.int64, device=dev)
        fed = torch.empty(B, steps, dtype=torch.int64, device=dev)
        logits = L.logits_buffer(N, V, dev)
        wsb = lib.sat_rollout_attend_fwd_ws_bytes(B, P, C, E, H, V)
        ws = torch.empty(wsb // 4, device=dev)
        L.check(lib.sat_rollout_attend_fwd(f2.data_ptr(), ctx_enc.data_ptr(), h0.data_ptr(), c0.data_ptr(), pi.prefix_dev.data_ptr(),
                                           B, steps, P, C, E, H, V, w, tapes, toks.data_ptr(), logits.data_ptr(), logits.shape[1],
                                           1 if greedy else 0, start_id, seed, rank, ids.data_ptr(), ids.stride(0), fed.data_ptr(),
                                           fed.stride(0), ws.data_ptr(), wsb, st), "sat_rollout_attend_fwd")
        if not greedy:
            # The loop's Z rows came from per-step split-K GEMMs (the draws need each step's logits).  The backward reads Z once, for
            # the classifier's weight gradient: give it the tape `_AttendFn.forward` leaves -- the output layer over all packed rows
            # as ONE GEMM with the two biases added in turn -- so that the gradients are, bit for bit, those of `decode` on `fed`.
            _gemm(lib, 0, 0, tp["Zin"], C + H, Wz, C + H, tp["Z"], E, N, E, C + H, m.context2out.bias, m.hidden2tout.bias)
        out["ids"], out["fed"], out["alphas"] = ids, fed, tp["ALPHA"]
        ctx.m, ctx.pi, ctx.captions = m, pi, fed
        ctx.tapes = dict(f2=f2, fmean=fmean, ctx_enc=ctx_enc, h0=h0, c0=c0, Wz=Wz, toks=toks, HSX=HSX, **tp)
        return logits if logits.shape[1] == V else logits[:, :V]

    @staticmethod
    def backward(ctx, dlogits):
        from .attend_bwd import attend_backward
        grads, d_feats, d_fmean = attend_backward(ctx.m, ctx.pi, ctx.captions, ctx.tapes, dlogits, want_dfeat=ctx.needs_input_grad[1])
        return (None, d_feats, d_fmean if ctx.needs_input_grad[2] else None) + (None,) * 6 + tuple(grads)


class _VggFn(torch.autograd.Function):
    """the conv stack WITH a backward (fine-tuning, model2.py:87-89 `finetune(allow=True)`): f32 parity mode, or bf16 forward /
    bf16 input-gradient convs with f32 master weights and f32 weight gradients (compute_dtype='bf16')"""

    @staticmethod
    def forward(ctx, prog, images, *params):
        feats, fmean = prog.run(images)
        ctx.prog, ctx.run_id = prog, prog.run_id
        return feats.clone(), fmean.clone()

    @staticmethod
    def backward(ctx, d_feats, d_fmean):
        prog = ctx.prog
        if prog.run_id != ctx.run_id:
            raise RuntimeError("the conv stack ran again before this backward: its activation tapes were overwritten "
                               "(fine-tuning keeps one forward per backward)")
        return (None, None) + tuple(prog.backward(d_feats, d_fmean))


PARAM_ORDER = ("image_att_w", "init_hidden.weight", "init_hidden.bias", "init_memory.weight", "init_memory.bias",
               "weight_hh.weight", "weight_hh.bias", "weight_att", "embedding.weight", "lstmcell.weight_ih", "lstmcell.weight_hh",
               "lstmcell.bias_ih", "lstmcell.bias_hh", "context2out.weight", "context2out.bias", "hidden2tout.weight",
               "hidden2tout.bias", "classifier.weight", "classifier.bias")


class ShowAttendTellModel(nn.Module):
    """model2.py:9-111.  `compute_dtype` ('bf16' conv stack / 'f32' parity) and `vgg_cfg` are build extensions."""

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
        self.compute_dtype = compute_dtype
        self.ss_prob = 0                  # scheduled sampling (train.py:109-113; schedule: trainer.ss_prob_for_epoch), training mode only
        self.ss_rank = 0                  # data-parallel rank: a stream of draws of its own per rank
        self.last_ss_inputs = self.last_ss_seed = None   # tokens fed [B, T] and seed of the last sampled forward
        self.alpha_c = 0                  # weight of the doubly stochastic attention penalty (Xu et al. 2015, section 4.2.1); 0 = off
        self.last_alphas = self.last_attention_penalty = None    # set by every decode / forward
        self.last_rollout_inputs = self.last_rollout_seed = None # tokens fed [B, steps] and seed of the last `rollout`
        self.last_scst = None                                    # the `SelfCritical` object of the last `scst_forward`
        self._programs, self._guard = {}, None
        self._pf_list = []          # features in flight: [(images, feats, fmean, event, weights signature, instance)]
        self.register_load_state_dict_post_hook(lambda mod, k: mod._programs.clear())
        self.encoder.register_load_state_dict_post_hook(lambda mod, k: self._programs.clear())

    def finetune(self, allow=False):
        """model2.py:87-89: (un)freeze the conv stack.  Fine-tuning runs the stack with a hand-written backward (dgrad through
        the forward conv kernel on flipped weights, wgrad as split-K GEMMs, ReLU / max-pool routing) in the f32 parity mode."""
        # compute_dtype='bf16': mixed precision -- the parameters ARE the f32 master weights; the stack runs on bf16 copies
        # refreshed from them before every forward (VggProgram.refresh_weights), gradients come back in f32 (_vgg_backward)
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
        from .models import lookahead_stream
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

    def forward(self, images, captions, lengths):
        """model2.py:38-65: logits f32 [sum(lengths), V], rows in time-major packed order."""
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
        parallelism B is the rank's own batch."""
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
            from .models import draw_ss_seed
            ss = dict(prob=float(self.ss_prob), seed=draw_ss_seed(), rank=int(self.ss_rank))
        ex = dict(alpha_c=float(self.alpha_c))
        out = _AttendFn.apply(self, features, fmean, captions, pi, ss, ex, *self._params())
        self.last_attention_penalty = None
        if ex["alpha_c"] > 0:
            out, self.last_attention_penalty = out
        self.last_alphas = ex.get("alphas")
        if ss is not None:
            self.last_ss_inputs, self.last_ss_seed = ss["used"], ss["seed"]
        return out

    def rollout(self, features, fmean, steps=20, greedy=False, start_id=1):
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
        would pull the maps of steps the loss masks towards covering the image.  (A length-masked penalty is a separate change.)"""
        if not self.training:
            raise RuntimeError("ShowAttendTellModel.rollout is a training forward (model.train()); eval mode decodes with sample()")
        L.require_gpu(features, "features")
        L.require_gpu(fmean, "fmean")
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        if features.dtype != torch.float32 or fmean.dtype != torch.float32:
            raise TypeError("features and fmean must be float32")
        features, fmean = features.contiguous(), fmean.contiguous()
        out = {}
        if greedy:
            with torch.no_grad():
                logits = _AttendRolloutFn.apply(self, features, fmean, steps, True, int(start_id), 0, 0, out, *self._params())
        else:
            from .models import draw_ss_seed
            seed = draw_ss_seed()
            logits = _AttendRolloutFn.apply(self, features, fmean, steps, False, int(start_id), seed, int(self.ss_rank), out,
                                            *self._params())
            self.last_rollout_seed = seed
        self.last_rollout_inputs, self.last_alphas, self.last_attention_penalty = out["fed"], out["alphas"], None
        return out["ids"], logits

    def scst_forward(self, images, image_index, scorer, end_id=2, steps=20):
        """The self-critical loss of one batch (`scst.SelfCritical.attend`) behind the conv stack: sampled rollout, arg-max rollout
        of the same policy as the baseline, CIDEr of both, weighted cross entropy.  image_index: the corpus image of every row, as
        for `CiderScorer.score`.  With `finetune(allow=True)` `loss.backward()` also reaches the conv stack.  The `SelfCritical`
        object (its last_reward, last_baseline, last_ids, last_greedy_ids) is kept as `last_scst`."""
        from .scst import SelfCritical
        feats, fmean = self._encode(images)
        self.last_scst = SelfCritical(scorer, end_id)
        return self.last_scst.attend(self, feats, fmean, image_index, steps)

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
        lib = L.load()
        m, dev, st = self, features.device, L.stream()
        B, P, C = features.shape
        E, H, V, Hin = m.embed_size, m.hidden_size, m.vocab_size, m.hidden_size
        f2 = features.contiguous().view(B * P, C)
        ctx_enc = torch.empty(B * P, C, device=dev)
        _gemm(lib, 0, 1, f2, C, m.image_att_w, C, ctx_enc, C, B * P, C, C)
        if states is None:
            h, c = torch.zeros(B, H, device=dev), torch.zeros(B, H, device=dev)
        else:
            if len(states) != 2 or any(tuple(s.shape) != (B, H) for s in states):
                raise ValueError("states must be (h, c), each [B=%d, H=%d] (model2.py:99), got %s"
                                 % (B, H, [tuple(s.shape) for s in states]))
            h, c = states[0].to(dev).float().contiguous().clone(), states[1].to(dev).float().contiguous().clone()
        h2 = torch.empty(B, H, device=dev)
        proj, X = torch.empty(B, C, device=dev), torch.empty(B, Hin, device=dev)
        ctxb, Zin, Z = torch.empty(B, C, device=dev), torch.empty(B, C + H, device=dev), torch.empty(B, E, device=dev)
        Wz = torch.empty(E, C + H, device=dev)
        L.check(lib.sat_rows_copy(L.ptr(m.context2out.weight), C, None, 0, E, E, C, L.ptr(Wz), C + H, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(m.hidden2tout.weight), H, None, 0, E, E, H, Wz.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
        ids = torch.full((B, steps), int(start_id), dtype=torch.int64, device=dev)
        start = torch.full((B,), int(start_id), dtype=torch.int64, device=dev)
        wsb = lib.sat_vocab_argmax_ws_bytes(B, V)
        ws = torch.empty(wsb // 4, device=dev)
        watt = m.weight_att.view(-1)
        att_ws = torch.empty(B * P, device=dev)
        amaps = torch.empty(steps, B, P, device=dev) if return_alphas else None       # step i's maps: the kernel's alpha output
        for i in range(steps):
            _gemm(lib, 0, 0, h, H, m.weight_hh.weight, H, proj, C, B, C, H, m.weight_hh.bias)
            L.check(lib.sat_attention_fwd(L.ptr(ctx_enc), L.ptr(f2), L.ptr(proj), C, L.ptr(watt), B, P, C,
                                          amaps[i].data_ptr() if return_alphas else None, L.ptr(ctxb), C,
                                          att_ws.data_ptr(), att_ws.numel() * 4, st), "sat_attention_fwd")
            if i == 0:                                                               # model2.py:101-102
                L.check(lib.sat_rows_copy(L.ptr(m.embedding.weight), E, start.data_ptr(), 1, V, B, E, L.ptr(X), Hin, st), "sat_rows_copy")
                L.check(lib.sat_rows_copy(L.ptr(ctxb), C, None, 0, B, B, C, X.data_ptr() + E * 4, Hin, st), "sat_rows_copy")
            L.check(lib.sat_lstmcell_fwd(L.ptr(X), L.ptr(h), L.ptr(c), L.ptr(m.lstmcell.weight_ih), L.ptr(m.lstmcell.weight_hh),
                                         L.ptr(m.lstmcell.bias_ih), L.ptr(m.lstmcell.bias_hh), B, Hin, H, L.ptr(h2), None, None, st),
                    "sat_lstmcell_fwd")
            h, h2 = h2, h
            L.check(lib.sat_rows_copy(L.ptr(ctxb), C, None, 0, B, B, C, L.ptr(Zin), C + H, st), "sat_rows_copy")
            L.check(lib.sat_rows_copy(L.ptr(h), H, None, 0, B, B, H, Zin.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
            _gemm(lib, 0, 0, Zin, C + H, Wz, C + H, Z, E, B, E, C + H, m.context2out.bias, m.hidden2tout.bias)
            col = ids[:, i]
            L.check(lib.sat_vocab_argmax(L.ptr(Z), L.ptr(m.classifier.weight), L.ptr(m.classifier.bias), B, E, V, col.data_ptr(),
                                         ids.stride(0), L.ptr(ws), wsb, st), "sat_vocab_argmax")
            # model2.py:107-108: the NEXT LSTM input = [embedding(predicted), THIS step's context]
            L.check(lib.sat_rows_copy(L.ptr(m.embedding.weight), E, col.data_ptr(), ids.stride(0), V, B, E, L.ptr(X), Hin, st), "sat_rows_copy")
            L.check(lib.sat_rows_copy(L.ptr(ctxb), C, None, 0, B, B, C, X.data_ptr() + E * 4, Hin, st), "sat_rows_copy")
        if return_alphas:
            return ids, amaps.transpose(0, 1).contiguous()
        return ids


@torch.no_grad()
def _sample_beam_features(self, features, beam_size=5, states=None, end_id=None, steps=20, start_id=1, return_all=False,
                          return_alphas=False):
    """Beam search over `sample`'s loop (model2.py:91-111; the reference's `sample_beam` is a stub, model2.py:113-114, so parity
    is pinned only at beam_size=1 == the greedy goldens).  Rows are (image b, hypothesis k) = b*K + k: the features and their
    attention encoding are replicated per hypothesis once (data movement), every step runs the greedy step's kernels on B*K rows,
    `sat_beam_step` keeps the best K of the K*V candidates per image, and h, c and the carried context follow their parent
    (`sat_beam_gather_rows`).  Returns ids i64 [B,steps] of the best hypothesis (return_all: ids [B,K,steps] best-first, scores).
    return_alphas: the attention maps follow as the last value -- [B,steps,P] of the best hypothesis, with return_all [B,K,steps,P]
    best-first.  Every step's maps are recorded per slot and `sat_beam_backtrack_rows` follows the parent chain: the map of a
    step belongs to the slot its survivor was expanded from."""
    lib = L.load()
    m, dev, st = self, features.device, L.stream()
    B, P, C = features.shape
    K = int(beam_size)
    if K < 1 or K > 8:
        raise ValueError("beam_size must be in 1..8")
    E, H, V, Hin = m.embed_size, m.hidden_size, m.vocab_size, m.hidden_size
    R = B * K
    feats = features.contiguous().repeat_interleave(K, 0).contiguous()           # [R, P, C]
    f2 = feats.view(R * P, C)
    ctx_enc = torch.empty(R * P, C, device=dev)
    _gemm(lib, 0, 1, f2, C, m.image_att_w, C, ctx_enc, C, R * P, C, C)
    if states is None:
        h, c = torch.zeros(R, H, device=dev), torch.zeros(R, H, device=dev)
    else:
        h = states[0].to(dev).float().repeat_interleave(K, 0).contiguous()
        c = states[1].to(dev).float().repeat_interleave(K, 0).contiguous()
    h2, c2 = torch.empty(R, H, device=dev), torch.empty(R, H, device=dev)
    proj, X = torch.empty(R, C, device=dev), torch.empty(R, Hin, device=dev)
    ctxb, ctx2 = torch.empty(R, C, device=dev), torch.empty(R, C, device=dev)
    Zin, Z = torch.empty(R, C + H, device=dev), torch.empty(R, E, device=dev)
    Wz = torch.empty(E, C + H, device=dev)
    L.check(lib.sat_rows_copy(L.ptr(m.context2out.weight), C, None, 0, E, E, C, L.ptr(Wz), C + H, st), "sat_rows_copy")
    L.check(lib.sat_rows_copy(L.ptr(m.hidden2tout.weight), H, None, 0, E, E, H, Wz.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
    ldl = L.pad4(V)
    logits = torch.zeros(R, ldl, device=dev)
    scores = torch.full((B, K), float("-inf"), device=dev)
    scores[:, 0] = 0.0
    scores2 = torch.empty(B, K, device=dev)
    bws = torch.empty(lib.sat_beam_step_ws_bytes(B, K), dtype=torch.uint8, device=dev)
    parents = torch.empty(steps, R, dtype=torch.int32, device=dev)
    tokens = torch.empty(steps, R, dtype=torch.int64, device=dev)
    start = torch.full((R,), int(start_id), dtype=torch.int64, device=dev)
    watt = m.weight_att.view(-1)
    att_ws = torch.empty(R * P, device=dev)
    amaps = torch.empty(steps, R, P, device=dev) if return_alphas else None
    eid = -1 if end_id is None else int(end_id)
    for i in range(steps):
        _gemm(lib, 0, 0, h, H, m.weight_hh.weight, H, proj, C, R, C, H, m.weight_hh.bias)
        L.check(lib.sat_attention_fwd(L.ptr(ctx_enc), L.ptr(f2), L.ptr(proj), C, L.ptr(watt), R, P, C,
                                      amaps[i].data_ptr() if return_alphas else None, L.ptr(ctxb), C,
                                      att_ws.data_ptr(), att_ws.numel() * 4, st), "sat_attention_fwd")
        if i == 0:                                                                   # model2.py:101-102
            L.check(lib.sat_rows_copy(L.ptr(m.embedding.weight), E, start.data_ptr(), 1, V, R, E, L.ptr(X), Hin, st), "sat_rows_copy")
            L.check(lib.sat_rows_copy(L.ptr(ctxb), C, None, 0, R, R, C, X.data_ptr() + E * 4, Hin, st), "sat_rows_copy")
        L.check(lib.sat_lstmcell_fwd(L.ptr(X), L.ptr(h), L.ptr(c), L.ptr(m.lstmcell.weight_ih), L.ptr(m.lstmcell.weight_hh),
                                     L.ptr(m.lstmcell.bias_ih), L.ptr(m.lstmcell.bias_hh), R, Hin, H, L.ptr(h2), None, None, st),
                "sat_lstmcell_fwd")
        h, h2 = h2, h
        L.check(lib.sat_rows_copy(L.ptr(ctxb), C, None, 0, R, R, C, L.ptr(Zin), C + H, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(h), H, None, 0, R, R, H, Zin.data_ptr() + C * 4, C + H, st), "sat_rows_copy")
        _gemm(lib, 0, 0, Zin, C + H, Wz, C + H, Z, E, R, E, C + H, m.context2out.bias, m.hidden2tout.bias)
        L.check(lib.sat_vocab_logits_fwd(L.ptr(Z), L.ptr(m.classifier.weight), L.ptr(m.classifier.bias), R, E, V, L.ptr(logits), ldl, st),
                "sat_vocab_logits_fwd")
        last = tokens[i - 1].data_ptr() if (i > 0 and eid >= 0) else None
        L.check(lib.sat_beam_step(L.ptr(logits), ldl, L.ptr(scores), last, eid, B, K, V, parents[i].data_ptr(), tokens[i].data_ptr(),
                                  L.ptr(scores2), L.ptr(bws), bws.numel(), st), "sat_beam_step")
        scores, scores2 = scores2, scores
        src_ctx = ctxb
        if K > 1:                                    # the survivors' state: h, c and THIS step's context follow their parent
            for (a, b_) in ((h, h2), (c, c2)):
                L.check(lib.sat_beam_gather_rows(L.ptr(a), parents[i].data_ptr(), B, K, H, L.ptr(b_), st), "sat_beam_gather_rows")
            h, h2, c, c2 = h2, h, c2, c
            L.check(lib.sat_beam_gather_rows(L.ptr(ctxb), parents[i].data_ptr(), B, K, C, L.ptr(ctx2), st), "sat_beam_gather_rows")
            src_ctx = ctx2
        # model2.py:107-108: the NEXT LSTM input = [embedding(token), THIS step's context]
        L.check(lib.sat_rows_copy(L.ptr(m.embedding.weight), E, tokens[i].data_ptr(), 1, V, R, E, L.ptr(X), Hin, st), "sat_rows_copy")
        L.check(lib.sat_rows_copy(L.ptr(src_ctx), C, None, 0, R, R, C, X.data_ptr() + E * 4, Hin, st), "sat_rows_copy")
    ids = torch.empty(B, K, steps, dtype=torch.int64, device=dev)
    L.check(lib.sat_beam_backtrack(L.ptr(parents), L.ptr(tokens), steps, B, K, L.ptr(ids), st), "sat_beam_backtrack")
    if return_alphas:
        alphas = torch.empty(B, K, steps, P, device=dev)
        L.check(lib.sat_beam_backtrack_rows(L.ptr(parents), L.ptr(amaps), steps, B, K, P, L.ptr(alphas), st), "sat_beam_backtrack_rows")
        if return_all:
            return ids, scores, alphas
        return ids[:, 0].contiguous(), alphas[:, 0].contiguous()
    if return_all:
        return ids, scores
    return ids[:, 0].contiguous()


@torch.no_grad()
def _sample_beam(self, images, beam_size=5, states=None, end_id=None, return_all=False, return_alphas=False):
    """`sample_beam(images, ...)`: the method the reference leaves as a stub (model2.py:113-114); BASELINE configs[4] asks beam 5."""
    feats, _ = self._encode(images)
    return self.sample_beam_features(feats, beam_size, states, end_id, return_all=return_all, return_alphas=return_alphas)


ShowAttendTellModel.sample_beam_features = _sample_beam_features
ShowAttendTellModel.sample_beam = _sample_beam
