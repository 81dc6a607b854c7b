"""Inception-v3 conv stack (BASELINE.json configs[3]: "Inception-v3 encoder (299x299)") as an op program for libsat_hip.so,
pluggable into `EncoderCNN`'s slot (`/root/reference/models.py:9-29`; the reference itself only has ResNet-152 / VGG16, so
this is a build extension: SURVEY 8f.3).  Parameter names are torchvision's (`Conv2d_1a_3x3.conv.weight`, `Mixed_5b.branch1x1.bn.*`,
..., `fc.*`), so an `inception_v3` state_dict loads as is (its AuxLogits head is not part of the feature path).

Every BasicConv2d = implicit-GEMM conv (asymmetric 1x7 / 7x1 / 1x3 / 3x1 kernels via per-axis padding) with the BatchNorm
statistics in its epilogue + one normalise/ReLU launch that writes straight into the channel slice of the block's
concatenated output (sat_op.ldc); 3x3 max / average pools are their own small kernels.  Train-mode batch statistics
(nothing calls .eval() in train.py), integer-atomic statistics in bf16 as on the ResNet path; eval uses the running ones."""
import torch
import torch.nn as nn

from . import _lib as L
from .program import OpProgram, act_op, avgpool, conv_op, image_prep
from .resnet import _BN, _Conv

BN_EPS = 1e-3

BLOCKS = [("Mixed_5b", "A", 192, 32, 256), ("Mixed_5c", "A", 256, 64, 288), ("Mixed_5d", "A", 288, 64, 288),
          ("Mixed_6a", "B", 288, None, 768), ("Mixed_6b", "C", 768, 128, 768), ("Mixed_6c", "C", 768, 160, 768),
          ("Mixed_6d", "C", 768, 160, 768), ("Mixed_6e", "C", 768, 192, 768), ("Mixed_7a", "D", 768, None, 1280),
          ("Mixed_7b", "E", 1280, None, 2048), ("Mixed_7c", "E", 2048, None, 2048)]


class _ConvI(_Conv):
    """conv weight holder with a rectangular kernel / per-axis padding (frozen, like the ResNet stack: models.py:14-15)"""

    def __init__(self, cin, cout, k, stride=1, pad=0):
        nn.Module.__init__(self)
        self.kh, self.kw = (k, k) if isinstance(k, int) else k
        self.ph, self.pw = (pad, pad) if isinstance(pad, int) else pad
        self.cin, self.cout, self.stride = cin, cout, stride
        w = torch.empty(cout, cin, self.kh, self.kw).normal_(0, (2.0 / (cin * self.kh * self.kw)) ** 0.5)
        self.weight = nn.Parameter(w, requires_grad=False)


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, k, stride=1, pad=0):
        super().__init__()
        self.conv, self.bn = _ConvI(cin, cout, k, stride, pad), _BN(cout)


def _block(kind, cin, arg):
    m = nn.Module()
    B = BasicConv2d
    if kind == "A":
        m.branch1x1, m.branch5x5_1, m.branch5x5_2 = B(cin, 64, 1), B(cin, 48, 1), B(48, 64, 5, 1, 2)
        m.branch3x3dbl_1, m.branch3x3dbl_2, m.branch3x3dbl_3 = B(cin, 64, 1), B(64, 96, 3, 1, 1), B(96, 96, 3, 1, 1)
        m.branch_pool = B(cin, arg, 1)
    elif kind == "B":
        m.branch3x3 = B(cin, 384, 3, 2)
        m.branch3x3dbl_1, m.branch3x3dbl_2, m.branch3x3dbl_3 = B(cin, 64, 1), B(64, 96, 3, 1, 1), B(96, 96, 3, 2)
    elif kind == "C":
        c7 = arg
        m.branch1x1 = B(cin, 192, 1)
        m.branch7x7_1, m.branch7x7_2, m.branch7x7_3 = B(cin, c7, 1), B(c7, c7, (1, 7), 1, (0, 3)), B(c7, 192, (7, 1), 1, (3, 0))
        m.branch7x7dbl_1, m.branch7x7dbl_2 = B(cin, c7, 1), B(c7, c7, (7, 1), 1, (3, 0))
        m.branch7x7dbl_3, m.branch7x7dbl_4 = B(c7, c7, (1, 7), 1, (0, 3)), B(c7, c7, (7, 1), 1, (3, 0))
        m.branch7x7dbl_5 = B(c7, 192, (1, 7), 1, (0, 3))
        m.branch_pool = B(cin, 192, 1)
    elif kind == "D":
        m.branch3x3_1, m.branch3x3_2 = B(cin, 192, 1), B(192, 320, 3, 2)
        m.branch7x7x3_1, m.branch7x7x3_2 = B(cin, 192, 1), B(192, 192, (1, 7), 1, (0, 3))
        m.branch7x7x3_3, m.branch7x7x3_4 = B(192, 192, (7, 1), 1, (3, 0)), B(192, 192, 3, 2)
    else:
        m.branch1x1 = B(cin, 320, 1)
        m.branch3x3_1, m.branch3x3_2a, m.branch3x3_2b = B(cin, 384, 1), B(384, 384, (1, 3), 1, (0, 1)), B(384, 384, (3, 1), 1, (1, 0))
        m.branch3x3dbl_1, m.branch3x3dbl_2 = B(cin, 448, 1), B(448, 384, 3, 1, 1)
        m.branch3x3dbl_3a, m.branch3x3dbl_3b = B(384, 384, (1, 3), 1, (0, 1)), B(384, 384, (3, 1), 1, (1, 0))
        m.branch_pool = B(cin, 192, 1)
    return m


class _FC(nn.Module):
    def __init__(self, fin, fout):
        super().__init__()
        self.in_features, self.out_features = fin, fout
        self.weight = nn.Parameter(torch.empty(fout, fin).normal_(0.0, 0.02))   # models.py:22
        self.bias = nn.Parameter(torch.zeros(fout))                             # models.py:23


class InceptionStack(nn.Module):
    """torchvision `inception_v3` parameter tree (feature path) + the trainable `fc` the reference puts on its encoder."""
    feature_dim = 2048

    def __init__(self, embed_size):
        super().__init__()
        B = BasicConv2d
        self.Conv2d_1a_3x3, self.Conv2d_2a_3x3, self.Conv2d_2b_3x3 = B(3, 32, 3, 2), B(32, 32, 3), B(32, 64, 3, 1, 1)
        self.Conv2d_3b_1x1, self.Conv2d_4a_3x3 = B(64, 80, 1), B(80, 192, 3)
        for name, kind, cin, arg, _ in BLOCKS:
            setattr(self, name, _block(kind, cin, arg))
        self.fc = _FC(self.feature_dim, embed_size)
        self.arch = "inception_v3"

    @property
    def conv1(self):           # EncoderCNN keys its program cache on the first conv
        return self.Conv2d_1a_3x3.conv

    def bns(self):
        return [m.bn for m in self.modules() if isinstance(m, BasicConv2d)]

    def program(self, N, H, W, dtype, training, device, groups=1, signatures=None):
        return InceptionProgram(self, N, H, W, dtype, training, device, groups=groups, signatures=signatures)


class InceptionProgram(OpProgram):
    """op program of the Inception-v3 stack for one (batch, H, W, dtype, training); groups = G > 1 (bf16): G look-ahead batches
    per launch, as in the ResNet program -- train mode: `sat_op.groups` = G, every per-batch buffer G consecutive copies,
    per-group BatchNorm statistics, deferred running statistics; eval mode: the batches concatenate into one program over
    G * N images."""
    BN_EPS = BN_EPS

    def __init__(self, stack, N, H, W, dtype, training, device, groups=1, signatures=None):
        super().__init__(stack, N, H, W, dtype, training, device, groups=groups, signatures=signatures)
        N, G = self.n, self.G
        GN = G * N                                         # images every per-image op (pools, image prep, the final pool) sees
        esz = 2 if dtype == L.SAT_BF16 else 4
        alloc, ops = self.alloc, self.ops

        def basic(m, x, h, w, out=None, out_off=0, out_ld=0):
            """BasicConv2d: conv (+ statistics) -> normalise + ReLU into `out` (a dense tensor or a channel slice).
            x: dense NHWC tensor [N,h,w,cin].  Returns (activation tensor or None when sliced, ho, wo)."""
            cv = m.conv
            cin = x.shape[3]
            ho, wo = (h + 2 * cv.ph - cv.kh) // cv.stride + 1, (w + 2 * cv.pw - cv.kw) // cv.stride + 1
            wt = cv.weight.detach().to(device=device, dtype=torch.float32)
            if wt.shape[1] != cin:                       # the stem's 3 input channels padded to one 16-byte chunk
                wp = torch.zeros(cv.cout, cin, cv.kh, cv.kw, device=device)
                wp[:, :wt.shape[1]] = wt
                wt = wp
            wk = wt.permute(0, 2, 3, 1).contiguous().to(self.td).reshape(cv.cout, -1)
            self.keep.append(wk)
            raw = alloc((GN, ho, wo, cv.cout))
            padw = dict(flags=L.CONV_PADW, pad_w=cv.pw) if cv.ph != cv.pw else {}
            o = conv_op(dtype, x, wk, raw, N, h, w, cin, ho, wo, cv.cout, cv.kh, cv.kw, cv.stride, cv.ph, groups=G, **padw)
            ops.append(o)
            src = self.bn_stats(o, m.bn)
            act = alloc((GN, ho, wo, cv.cout)) if out is None else None
            dst = act if out is None else out.data_ptr() + out_off * esz
            ops.append(src.attach(act_op(L.OP_BN_RELU, dtype, raw, dst, N, ho, wo, cv.cout, groups=G, ldc=out_ld)))
            return act, ho, wo

        def pool(kind, x, h, w, out=None, out_off=0, out_ld=0):
            c = x.shape[3]
            ho, wo = (h, w) if kind == L.OP_AVGPOOL3 else ((h - 3) // 2 + 1, (w - 3) // 2 + 1)
            res = alloc((GN, ho, wo, c)) if out is None else None
            dst = res if out is None else out.data_ptr() + out_off * esz
            # per image: the groups concatenate
            ops.append(L.op(kind, dtype, in0=x, out=dst, N=GN, Hin=h, Win=w, Cout=c, Hout=ho, Wout=wo, ldc=out_ld))
            return res, ho, wo

        # ---- program ----
        cpad = 16 // esz                                 # the 3 image channels padded to one 16-byte chunk per pixel
        self.img = alloc((GN, H, W, cpad), zero=True)
        ops += image_prep(dtype, self.img, self.N, H, W, 0, groups=self.groups, cout=cpad)
        x, h, w = self.img, H, W
        for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            x, h, w = basic(getattr(stack, name), x, h, w)
        x, h, w = pool(L.OP_MAXPOOL3S2, x, h, w)
        for name in ("Conv2d_3b_1x1", "Conv2d_4a_3x3"):
            x, h, w = basic(getattr(stack, name), x, h, w)
        x, h, w = pool(L.OP_MAXPOOL3S2, x, h, w)
        for name, kind, cin, arg, cout in BLOCKS:
            m = getattr(stack, name)
            if kind in ("B", "D"):
                ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            else:
                ho, wo = h, w
            y = alloc((GN, ho, wo, cout))
            off = 0

            def chain(names, src, hh, ww, width):
                nonlocal off
                t = src
                for n_ in names[:-1]:
                    t, hh, ww = basic(getattr(m, n_), t, hh, ww)
                basic(getattr(m, names[-1]), t, hh, ww, y, off, cout)
                off += width

            if kind == "A":
                chain(["branch1x1"], x, h, w, 64)
                chain(["branch5x5_1", "branch5x5_2"], x, h, w, 64)
                chain(["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x, h, w, 96)
                ap, _, _ = pool(L.OP_AVGPOOL3, x, h, w)
                chain(["branch_pool"], ap, h, w, arg)
            elif kind == "B":
                chain(["branch3x3"], x, h, w, 384)
                chain(["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x, h, w, 96)
                pool(L.OP_MAXPOOL3S2, x, h, w, y, off, cout)
                off += cin
            elif kind == "C":
                chain(["branch1x1"], x, h, w, 192)
                chain(["branch7x7_1", "branch7x7_2", "branch7x7_3"], x, h, w, 192)
                chain(["branch7x7dbl_%d" % i for i in range(1, 6)], x, h, w, 192)
                ap, _, _ = pool(L.OP_AVGPOOL3, x, h, w)
                chain(["branch_pool"], ap, h, w, 192)
            elif kind == "D":
                chain(["branch3x3_1", "branch3x3_2"], x, h, w, 320)
                chain(["branch7x7x3_%d" % i for i in range(1, 5)], x, h, w, 192)
                pool(L.OP_MAXPOOL3S2, x, h, w, y, off, cout)
                off += cin
            else:
                chain(["branch1x1"], x, h, w, 320)
                t, _, _ = basic(m.branch3x3_1, x, h, w)
                basic(m.branch3x3_2a, t, h, w, y, off, cout)
                basic(m.branch3x3_2b, t, h, w, y, off + 384, cout)
                off += 768
                t, _, _ = basic(m.branch3x3dbl_1, x, h, w)
                t, _, _ = basic(m.branch3x3dbl_2, t, h, w)
                basic(m.branch3x3dbl_3a, t, h, w, y, off, cout)
                basic(m.branch3x3dbl_3b, t, h, w, y, off + 384, cout)
                off += 768
                ap, _, _ = pool(L.OP_AVGPOOL3, x, h, w)
                chain(["branch_pool"], ap, h, w, 192)
            assert off == cout, (name, off, cout)
            x, h, w = y, ho, wo
        self.pooled = alloc((GN, stack.feature_dim), torch.float32)
        ops.append(avgpool(dtype, x, self.pooled, h, w))
        # per-geometry kernel selection, as on the ResNet path (no activation buffer needs re-randomising: the tuner only times)
        self._finish()

    def _eval_bn(self, bn, c, count):
        """eval: one finalize launch per layer turns the running statistics into a (scale, shift) table"""
        return self._bn_finalize(bn, c, count, 0, 0)[1]
