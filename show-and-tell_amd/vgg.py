"""The conv stack of Show-Attend-Tell (model2.py:15-17): VGG16 `features[:-3]` as the conv op program of the ResNet path
(implicit-GEMM conv with the bias + ReLU riding in the bf16 conv epilogue, SAT_OP_MAXPOOL2).  `VggFeatures` is the parameter tree,
`VggProgram` the device buffers + sat_op array with `run` and the hand-written `backward` of `finetune(allow=True)`
(model2.py:87-89), `_VggFn` the two behind torch.autograd."""
import torch
import torch.nn as nn

from . import _lib as L
from . import tune as T
from .program import act_op, avgpool, conv_op, image_prep, tdtype

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

    def backward(self, d_feats, d_fmean):
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
                _run_input_grad_conv(lib, st, L.SAT_BF16, dZb, wfb, dXb, N, h, w, cin, cout)
                L.check(lib.sat_cast_bf16_f32(dXb.data_ptr(), dX.data_ptr(), dX.numel(), st), "sat_cast_bf16_f32")
            else:
                _run_input_grad_conv(lib, st, L.SAT_F32, dZp, wflip, dX, N, h, w, cin, cout)
            dY = dX
        out = []
        for conv in self.stack.convs():
            out += list(grads[conv])
        return out


def _run_input_grad_conv(lib, st, dtype, dZp, wflip, dX, N, h, w, cin, cout):
    """dX [N,h,w,cin] = the 3x3 stride-1 conv (no padding arithmetic: strides from the padded shape) of the zero-bordered dZp
    [N,h+2,w+2,cout] with the flipped, transposed weights [cin, 9*cout]: one OP_CONV op, all three tensors of `dtype`"""
    hp, wp = h + 2, w + 2
    o = L.SatOp()
    o.kind, o.dtype = L.OP_CONV, dtype
    o.in0, o.w, o.out = dZp.data_ptr(), wflip.data_ptr(), dX.data_ptr()
    o.N, o.Hin, o.Win, o.Cin, o.Hout, o.Wout, o.Cout = N, hp, wp, cout, h, w, cin
    o.KH, o.KW, o.stride, o.pad = 3, 3, 1, 0
    o.sN, o.sH, o.sW = hp * wp * cout, wp * cout, cout
    L.check(lib.sat_run_ops((L.SatOp * 1)(o), 1, st), "sat_run_ops")


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
