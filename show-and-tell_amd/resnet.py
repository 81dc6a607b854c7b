"""The frozen ResNet conv stack of `EncoderCNN` (`/root/reference/models.py:13-15,27`) as an op program for
libsat_hip.so.

Host side only: this module owns the parameters (torchvision key names, so a `resnet152` state_dict loads
as is), lays the weights out for the kernels (OHWI, optional bf16 shadow), carves the activation
workspace and emits the `sat_op` array that `sat_run_ops` launches in ONE call per forward.  All arithmetic
is in the HIP kernels (csrc/sat_gemm.hip implicit-GEMM conv, csrc/sat_elementwise.hip batch-norm / pooling).

Layout: activations NHWC (channels contiguous -> the implicit-GEMM K axis is contiguous), dtype bf16
(throughput) or f32 (parity).  Per bottleneck (torchvision v1.5: stride on the 3x3):
    c1 = conv1x1(y)      stats -> (s1,t1)    a1 = relu(c1*s1+t1)
    c2 = conv3x3(a1)     stats -> (s2,t2)    a2 = relu(c2*s2+t2)
    c3 = conv1x1(a2)     stats -> (s3,t3)    [cd = conv1x1(y), stats -> (sd,td)]
    y' = relu(c3*s3+t3 + (cd*sd+td | y))
Training: batch statistics come out of the conv epilogue, as per-tile column sums reduced in fixed order by a finalize
launch, or (bf16, few M-tiles) as fixed-point integer atomics the consuming kernel turns into (scale, shift) itself;
conv3 applies bn2+ReLU to its operand in LDS.  Inference (bf16): every BatchNorm is a per-channel affine folded into
the producing conv's epilogue with the residual add and the ReLU.  The whole program replays as one hipGraph.
"""
import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import _lib as L
from .program import BN_MOMENTUM, BnSource, OpProgram, act_op, avgpool, conv_op, image_prep

RESNET152 = dict(layers=(3, 8, 36, 3), width=64)
BN_EPS = 1e-5


class _Conv(nn.Module):
    def __init__(self, cin, cout, k, stride, pad):
        super().__init__()
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, stride, pad
        w = torch.empty(cout, cin, k, k)
        nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")     # torchvision resnet init
        self.weight = nn.Parameter(w, requires_grad=False)                  # models.py:14-15 (frozen)


class _BN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long))


class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1, self.bn1 = _Conv(inplanes, planes, 1, 1, 0), _BN(planes)
        self.conv2, self.bn2 = _Conv(planes, planes, 3, stride, 1), _BN(planes)
        self.conv3, self.bn3 = _Conv(planes, planes * 4, 1, 1, 0), _BN(planes * 4)
        if downsample:
            self.downsample = nn.ModuleList([_Conv(inplanes, planes * 4, 1, stride, 0), _BN(planes * 4)])
        else:
            self.downsample = None


class _FC(nn.Module):
    def __init__(self, fin, fout):
        super().__init__()
        self.in_features, self.out_features = fin, fout
        self.weight = nn.Parameter(torch.empty(fout, fin).normal_(0.0, 0.02))   # models.py:22
        self.bias = nn.Parameter(torch.zeros(fout))                             # models.py:23


class ResNetStack(nn.Module):
    """Parameter tree with torchvision's names: conv1, bn1, layer{1..4}.{i}.{conv,bn}{1,2,3}, downsample.{0,1}, fc."""

    def __init__(self, embed_size, arch=RESNET152):
        super().__init__()
        self.arch = dict(arch)
        w = arch["width"]
        self.conv1, self.bn1 = _Conv(3, w, 7, 2, 3), _BN(w)
        inplanes = w
        for li, nblocks in enumerate(arch["layers"]):
            planes = w * (2 ** li)
            blocks = []
            for b in range(nblocks):
                stride = 2 if (li > 0 and b == 0) else 1
                ds = b == 0 and (stride != 1 or inplanes != planes * 4)
                blocks.append(_Bottleneck(inplanes, planes, stride, ds))
                inplanes = planes * 4
            setattr(self, "layer%d" % (li + 1), nn.ModuleList(blocks))
        self.feature_dim = inplanes
        self.fc = _FC(inplanes, embed_size)

    def blocks(self):
        for li in range(len(self.arch["layers"])):
            for blk in getattr(self, "layer%d" % (li + 1)):
                yield blk

    def bns(self):
        yield self.bn1
        for blk in self.blocks():
            yield blk.bn1
            yield blk.bn2
            yield blk.bn3
            if blk.downsample is not None:
                yield blk.downsample[1]


def weights_signature(stack):
    """Changes whenever a frozen conv weight is replaced (a new Parameter object on the module) or written in place through the
    Parameter (load_state_dict, copy_): the op program keeps permuted (bf16) copies of the conv weights and must be rebuilt
    then.  Writes through `.data` bypass the version counter -- call `EncoderCNN.refresh_weights()` after those."""
    # the walk over the module tree is cached (155 convs on ResNet-152, 3-4 signatures per step) as (module, weight) pairs; a
    # module whose `.weight` is no longer the cached object (assignment, module conversion) re-walks; `_sig_params` is also
    # dropped by EncoderCNN._invalidate (load_state_dict, device / dtype moves, refresh_weights)
    ws = stack.__dict__.get("_sig_params")
    if ws is None or any(m._parameters.get("weight") is not w for m, w in ws):
        ws = [(m, m.weight) for m in stack.modules() if isinstance(m, _Conv)]
        stack.__dict__["_sig_params"] = ws
    sig = 0
    for _, w in ws:
        sig = (sig * 1000003 + w._version * 7 + (w.data_ptr() & 0xffffffff)) & ((1 << 61) - 1)
    return sig


_Geo = namedtuple("_Geo", "h w h2 w2 inpl planes stride")     # one bottleneck: input map, output map, in-channels, planes, stride


class ConvStackProgram(OpProgram):
    """The ResNet stack's op program (groups, signatures, running and tuning: `OpProgram`).  The stem, then every bottleneck in
    one of four forms: eval-fused (inference), Gram (bf16 training: bn3's statistics from the Gram matrix of conv3's input),
    deferred (opt-in: bn3 + residual add + ReLU inside the next conv1) or standard."""
    BN_EPS = BN_EPS

    def __init__(self, stack, N, H, W, dtype, training, device, groups=1, signatures=None):
        super().__init__(stack, N, H, W, dtype, training, device, groups=groups, signatures=signatures)
        bf16 = dtype == L.SAT_BF16
        ch = 8 if bf16 else 4
        if stack.arch["width"] % ch:
            raise ValueError("conv stack width must be a multiple of %d for this dtype" % ch)
        # IN-PLACE BatchNorm-apply passes (bf16 training): relu(bn1(c1)) overwrites c1, and conv3 writes its raw output straight into
        # the next block-output buffer, which the normalise+add pass then transforms in place -- a bottleneck touches two large
        # buffers instead of three, so a stack's live set in layer 3 drops from ~90 to ~65 MB (+0.7 % under look-ahead)
        self.inplace = training and bf16
        # (SAT_GRAM_BN3 / SAT_GRAM_MAX_PLANES: `_gram_eligible`; SAT_DEFER_BN3 / SAT_DEFER_INPLACE: `_defer_eligible`)
        self.gram_bn3 = training and bf16 and os.environ.get("SAT_GRAM_BN3", "1") != "0"
        self.gram_pmax = int(os.environ.get("SAT_GRAM_MAX_PLANES", "128"))
        self.defer_bn3 = training and bf16 and os.environ.get("SAT_DEFER_BN3", "0") == "1"
        self.defer_inplace = os.environ.get("SAT_DEFER_INPLACE", "0") == "1"
        # a (scale, shift) table per BatchNorm where they are tables (f32 training: finalize launches; eval: the batched eval launch)
        self.scale_shift = None if (training and bf16) else self.alloc((len(list(stack.bns())), 2, stack.feature_dim), torch.float32)
        self._n_tables, self._eval_items = 0, []
        self.gram_blocks = self.deferred_blocks = 0
        self._pending = None             # (raw conv3 tensor, bn3 source) of a deferred bottleneck in front

        self._geometry_and_buffers()
        self._stem()
        blocks = list(zip(stack.blocks(), self.geo))
        for bi, (blk, g) in enumerate(blocks):
            nxt = blocks[bi + 1] if bi + 1 < len(blocks) else None
            if not training and bf16:
                self._eval_fused_block(blk, g)
            elif self._gram_eligible(g):
                self._gram_block(blk, g)
            elif self._defer_eligible(blk, g, nxt):
                self._deferred_block(blk, g)
            else:
                self._standard_block(blk, g)
        self.ops.append(avgpool(dtype, self.y, self.pooled, self.geo[-1].h2, self.geo[-1].w2))   # per image: groups concatenate
        if self._eval_items:
            # eval: (scale, shift) depend on parameters and running statistics only -> ONE batched launch for all BatchNorms
            # right after image prep, before the first consumer, instead of a finalize launch per layer
            arr = (L.SatBnEvalItem * len(self._eval_items))(*self._eval_items)
            self.eval_table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
            self.keep.append(self.eval_table)
            self.ops.insert(self._n_prep, L.op(L.OP_BN_EVAL_BATCH, dtype, in0=self.eval_table, count=len(self._eval_items), eps=BN_EPS))
        self._finish((self.c0, self.c1, self.a1, self.c2, self.a2, self.c3, self.cd, *self.ybuf))

    # ---- geometry, buffers, stem ----
    def _geometry_and_buffers(self):
        n, G, width = self.n, self.G, self.stack.arch["width"]
        self.Ho, self.Wo = (self.H + 6 - 7) // 2 + 1, (self.W + 6 - 7) // 2 + 1
        h, w = (self.Ho + 2 - 3) // 2 + 1, (self.Wo + 2 - 3) // 2 + 1          # after the 3x3/2 max pool
        inpl, self.geo = width, []
        for li, nblocks in enumerate(self.stack.arch["layers"]):
            planes = width * (2 ** li)
            for b in range(nblocks):
                stride = 2 if (li > 0 and b == 0) else 1
                h2, w2 = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
                self.geo.append(_Geo(h, w, h2, w2, inpl, planes, stride))
                h, w, inpl = h2, w2, planes * 4
        g0 = self.geo[0]
        max_c1 = max(n * g.h * g.w * g.planes for g in self.geo)
        max_c2 = max(n * g.h2 * g.w2 * g.planes for g in self.geo)
        max_c3 = max(n * g.h2 * g.w2 * g.planes * 4 for g in self.geo)
        # every per-batch buffer of a grouped program is G consecutive copies of the ungrouped one: a group's slice of an
        # activation buffer starts at g * (elements of THAT tensor), so the ping-pong buffers are sized G x their largest tenant
        self.c0 = self.alloc((G * n * self.Ho * self.Wo * width,))
        self.ybuf = [self.alloc((G * max(n * g0.h * g0.w * width, max_c3),)) for _ in range(2)]
        self.y, self.ynext = self.ybuf
        self.c1, self.a1 = self.alloc((G * max_c1,)), self.alloc((G * max_c1,))
        self.c2, self.a2 = self.alloc((G * max_c2,)), self.alloc((G * max_c2,))
        self.c3, self.cd = self.alloc((G * max_c3,)), self.alloc((G * max_c3,))
        self.pooled = self.alloc((G * n, self.stack.feature_dim), torch.float32)
        gram_geo = [(n * g.h2 * g.w2, g.planes) for g in self.geo if self._gram_eligible(g)]
        if gram_geo:
            self.gram_slabs = self.alloc((G * max(self.lib.sat_gram_slab_floats(m, p) for m, p in gram_geo),), torch.float32)
            pmax = max(p for _, p in gram_geo)
            self.gram_cov3 = self.alloc((G * 3 * pmax * pmax,), torch.bfloat16)
            self.gram_mu = self.alloc((G * pmax,), torch.float64)
            self.gram_T = self.alloc((G * 3 * max(p * p * 4 for _, p in gram_geo),), torch.float32)

    def _stem(self):
        """image prep; the 7x7/2 conv on a zero-bordered NHWC4 image, per kh one contiguous run of 8 pixels x 4 channels; bn1 +
        ReLU + the 3x3/2 max pool in one launch"""
        n, G, width, dt = self.n, self.G, self.stack.arch["width"], self.dtype
        Hp, Wp = self.H + 6, (self.W + 8 + 1) // 2 * 2
        w1 = self.stack.conv1.weight.detach().to(device=self.device, dtype=torch.float32)     # [w,3,7,7]
        wst = torch.zeros(width, 7, 8, 4, device=self.device, dtype=torch.float32)
        wst[:, :, :7, :3] = w1.permute(0, 2, 3, 1)
        wst = wst.reshape(width, 7 * 32).contiguous().to(self.td)
        self.keep.append(wst)
        self.img_pad = self.alloc((G * n, Hp, Wp, 4), zero=True)           # (eval: n is already groups * N)
        self.ops += image_prep(dt, self.img_pad, self.N, self.H, self.W, 3, groups=self.groups)
        cv = conv_op(dt, self.img_pad, wst, self.c0, n, Hp, Wp, 32, self.Ho, self.Wo, width, 7, 1, 2, 0, groups=G,
                     sN=Hp * Wp * 4, sH=Wp * 4, sW=4, **self._tiles(n * self.Ho * self.Wo))
        self.ops.append(cv)
        src = self.bn_stats(cv, self.stack.bn1)
        g0 = self.geo[0]
        self.ops.append(src.attach(L.op(L.OP_BN_RELU_MAXPOOL, dt, groups=G, in0=self.c0, out=self.y, N=n, Hin=self.Ho,
                                        Win=self.Wo, Cout=width, Hout=g0.h, Wout=g0.w)))

    def _tiles(self, m):
        # training convs carry their row-tile count whichever form their statistics take
        return dict(tiles_m=self.lib.sat_conv_tiles_m(m)) if self.training else {}

    def _conv(self, conv, x, out, hin, win, hout, wout):
        """a frozen conv, weights in kernel layout ([Cout][KH][KW][Cin])"""
        wt = conv.weight.detach().to(device=self.device, dtype=torch.float32).permute(0, 2, 3, 1).contiguous().to(self.td)
        wt = wt.reshape(conv.cout, -1)
        self.keep.append(wt)
        cin, n = conv.cin, self.n
        o = conv_op(self.dtype, x, wt, out, n, hin, win, cin, hout, wout, conv.cout, conv.k, conv.k, conv.stride, conv.pad,
                    groups=self.G, **self._tiles(n * hout * wout))
        pw_geom = conv.k == 3 and conv.stride == 1 and conv.pad == 1 and win <= 31
        aw_geom = conv.k == 1 and conv.pad == 0
        if self.dtype == L.SAT_BF16 and cin % 64 == 0 and conv.cout % 128 == 0 and (pw_geom or aw_geom):
            # frozen weights: a second copy in MFMA fragment order lets the tuner pick conv_pw_kernel (3x3) / conv_aw_kernel (1x1):
            # weights straight into registers, two workgroups per CU
            wp = torch.empty_like(wt)
            L.check(self.lib.sat_conv_pack_weights(wt.data_ptr(), wp.data_ptr(), conv.cout, cin, conv.k * conv.k, L.stream()),
                    "sat_conv_pack_weights")
            self.keep.append(wp)
            o.w_packed = wp.data_ptr()
        return o

    # ---- BatchNorm tables ----
    def _bn_table(self, c):
        """the next BatchNorm's slot of `scale_shift` (slots in emission order)"""
        i = self._n_tables
        self._n_tables += 1
        return self.scale_shift[i, 0, :c], self.scale_shift[i, 1, :c]

    def _eval_bn(self, bn, c, count):
        s, t = self._bn_table(c)
        self._eval_items.append(L.SatBnEvalItem(gamma=bn.weight.data_ptr(), beta=bn.bias.data_ptr(), running_mean=bn.running_mean.data_ptr(),
                                                running_var=bn.running_var.data_ptr(), scale_out=s.data_ptr(), shift_out=t.data_ptr(), C=c))
        return BnSource(bn, count, BN_EPS, scale=s.data_ptr(), shift=t.data_ptr())

    # ---- bottleneck forms ----
    def _swap(self):
        self.y, self.ynext = self.ynext, self.y

    def _fuse_bn1(self, g):
        """bf16 training: conv2 (3x3) reads the RAW c1 and applies bn1 + ReLU to its LDS-resident input patch -- where
        conv_pr_kernel runs it (stride 1, 128 <= planes <= 512, rows of <= 31 pixels: the transform touches each 64-channel slice
        of the patch once per workgroup).  Measured (round 3, bench.py, A/B on one box): 15.37 -> 15.95 k img/s with three stacks
        in flight: 44 of the 50 normalise+ReLU launches of ResNet-152 disappear (round 4, with the weights-in-registers kernels:
        un-fusing bn1 / bn2 / both makes the convs 2 / 1.5 / 4 % faster in sequence and the step 0.5 / 2 / 4 % slower -- the
        separate passes' bytes still cost more than the transforms)"""
        return (self.training and self.dtype == L.SAT_BF16 and g.h2 == g.h and g.w2 == g.w and g.planes % 64 == 0 and
                128 <= g.planes <= 512 and g.w <= 31)

    def _fuse_bn2(self, g):
        """bf16: conv3 (1x1) reads the RAW c2 and applies bn2 + ReLU to its A operand in LDS (the operand transform of
        conv_xp_kernel / the ring kernel): a2 never exists in HBM"""
        return self.dtype == L.SAT_BF16 and g.planes <= 512 and g.planes % 64 == 0

    def _gram_eligible(self, g):
        """a bottleneck without projection that the Gram kernels run, within SAT_GRAM_MAX_PLANES"""
        # bf16 training: bn3 + residual add + ReLU in conv3's EPILOGUE, with bn3's batch statistics taken from the Gram matrix of
        # conv3's input (csrc/sat_gram.hip: mean_c = w_c . mu, var_c = w_c^T cov(a2) w_c) -- the raw conv3 tensor and the
        # normalise+add launch (42 % of the stack's memory traffic in round 4, at the HBM roof) never exist.  The kernels run
        # non-projection bottlenecks with planes in {128, 256, 384, 512} (44 of ResNet-152's 50); MEASURED (round 5, interleaved on
        # one box, profiles/r05_gram_ab.txt) it pays only where the normalise+add pass is large against the chain's four small
        # launches: planes 128 (layer 2: +1 % on the step); at planes 256 (layer 3: 35 of the 44) the chain costs 30-45 us per
        # bottleneck against the 19-37 us launch it removes and the step LOSES 9 % -- so the default fuses planes <= 128 only
        # (SAT_GRAM_MAX_PLANES=512: every eligible bottleneck; SAT_GRAM_BN3=0: none, the three-launch form everywhere)
        return (self.gram_bn3 and g.stride == 1 and g.inpl == g.planes * 4 and g.planes % 128 == 0 and
                g.planes <= self.gram_pmax)

    def _defer_eligible(self, blk, g, nxt):
        """a bottleneck without projection followed by another one in the same layer whose conv1 conv_ay_kernel runs (planes a
        multiple of 128: layers 2-4); (checked after `_gram_eligible`: a bottleneck fused through the Gram statistics is not)"""
        # bf16 training, OPT-IN (SAT_DEFER_BN3=1): bn3 + residual add + ReLU of bottleneck k DEFERRED into conv1 of bottleneck k + 1
        # (conv_ay_kernel, SAT_CONV_IN_RESIDUAL): that conv builds its operand relu(bn3(c3_k) + y_{k-1}) on the way to LDS and writes
        # y_k out as it goes -- the normalise + add launch and conv1's re-read of the tensor it wrote disappear (bit-identical
        # results, tests/test_gpu_conv_ay.py).  MEASURED (round 5, interleaved on one box, profiles/r05_defer_ab.txt): per layer-3
        # bottleneck 24 + 38 us -> 39.5 us in sequence (the pass's bytes now stream at the HBM rate under conv1's MFMAs), 8 % fewer
        # bytes per pass, the encoder pipeline ALONE 2.96 -> 2.87 ms per batch -- and the training step unchanged to 1 % slower
        # (3.41 -> 3.42-3.46 ms): under the look-ahead the light normalise + add launches already ran beside the other stacks' convs
        # for free, while the fused conv1 holds a conv workgroup's registers and LDS for 15 us longer -- what the step pays for is
        # conv workgroup-time.  Hence opt-in.  SAT_DEFER_INPLACE=1: y_k overwrites the raw conv3 tensor (two large buffers per
        # bottleneck instead of three; only where one column tile covers conv1's Cout)
        return (self.defer_bn3 and blk.downsample is None and nxt is not None and nxt[0].downsample is None and
                nxt[1].stride == 1 and nxt[1].planes == g.planes and nxt[1].inpl == g.planes * 4 and g.planes % 128 == 0 and
                g.planes * 4 <= 2048)

    def _conv1_conv2(self, blk, g):
        """conv1 + bn1 (finishing a deferred bottleneck in front), conv2 + bn2 -> bn2's source"""
        if self._pending is not None:
            # this conv1 also finishes the bottleneck in front: operand = relu(bn3(c3) + y), written to the other y buffer
            c3_prev, s3 = self._pending
            self._pending = None
            cv1 = s3.conv_input(self._conv(blk.conv1, c3_prev, self.c1, g.h, g.w, g.h, g.w))
            cv1.in1, cv1.out1, cv1.flags = self.y.data_ptr(), self.ynext.data_ptr(), cv1.flags | L.CONV_IN_RESIDUAL
            self._swap()
            self.deferred_blocks += 1
        else:
            cv1 = self._conv(blk.conv1, self.y, self.c1, g.h, g.w, g.h, g.w)
        self.ops.append(cv1)
        s1 = self.bn_stats(cv1, blk.bn1)
        if self._fuse_bn1(g):
            # (padded taps read a row of zeros, so the zero padding stays zero): a1 never exists in HBM
            cv2 = s1.conv_input(self._conv(blk.conv2, self.c1, self.c2, g.h, g.w, g.h2, g.w2))
        else:
            a1 = self.c1 if self.inplace else self.a1
            self.ops.append(s1.attach(act_op(L.OP_BN_RELU, self.dtype, self.c1, a1, self.n, g.h, g.w, g.planes, groups=self.G)))
            cv2 = self._conv(blk.conv2, a1, self.c2, g.h, g.w, g.h2, g.w2)
        self.ops.append(cv2)
        return self.bn_stats(cv2, blk.bn2)

    def _conv3(self, blk, g, s2, out):
        """conv3 (bn2 + ReLU fused into its operand where `_fuse_bn2`) into `out` + bn3 -> bn3's source"""
        if self._fuse_bn2(g):
            cv3 = s2.conv_input(self._conv(blk.conv3, self.c2, out, g.h2, g.w2, g.h2, g.w2))
        else:
            a2 = self.c2 if self.inplace else self.a2
            self.ops.append(s2.attach(act_op(L.OP_BN_RELU, self.dtype, self.c2, a2, self.n, g.h2, g.w2, g.planes, groups=self.G)))
            cv3 = self._conv(blk.conv3, a2, out, g.h2, g.w2, g.h2, g.w2)
        self.ops.append(cv3)
        return self.bn_stats(cv3, blk.bn3)

    def _standard_block(self, blk, g):
        """conv1, conv2, conv3 with their statistics, then one normalise + (projected) residual add + ReLU pass"""
        s2 = self._conv1_conv2(blk, g)
        c3 = self.ynext if self.inplace else self.c3
        s3 = self._conv3(blk, g, s2, c3)
        if blk.downsample is not None:
            cd = self._conv(blk.downsample[0], self.y, self.cd, g.h, g.w, g.h2, g.w2)
            self.ops.append(cd)
            sd = self.bn_stats(cd, blk.downsample[1])
        o = s3.attach(act_op(L.OP_BN_ADD_RELU, self.dtype, c3, self.ynext, self.n, g.h2, g.w2, g.planes * 4, groups=self.G,
                             in1=self.y if blk.downsample is None else self.cd))
        if blk.downsample is not None:
            sd.attach(o, 1)
        self.ops.append(o)
        self._swap()

    def _deferred_block(self, blk, g):
        """conv1, conv2, conv3 with their statistics; the next bottleneck's conv1 applies bn3 + residual + ReLU (y stays y_{k-1}:
        that conv adds it and writes y_k into ynext)"""
        s2 = self._conv1_conv2(blk, g)
        # (in place only where ONE column tile of the consuming conv1 covers its Cout = planes: 128, or 256 with the
        # eight-wave variant -- the library refuses the aliasing otherwise)
        c3 = self.ynext if (self.defer_inplace and g.planes <= 256) else self.c3
        self._pending = (c3, self._conv3(blk, g, s2, c3))

    def _gram_block(self, blk, g):
        """bn3's batch statistics from the Gram matrix of conv3's input, then conv3 with bn3 + residual + ReLU in its epilogue"""
        s2 = self._conv1_conv2(blk, g)
        n, G, dt, bn3 = self.n, self.G, self.dtype, blk.bn3
        P3, N3 = g.planes, g.planes * 4
        cv3 = s2.conv_input(self._conv(blk.conv3, self.c2, self.ynext, g.h2, g.w2, g.h2, g.w2))
        gr = L.op(L.OP_GRAM, dt, groups=G, in0=self.c2, out=self.gram_slabs, N=n, Hout=g.h2, Wout=g.w2, Cout=P3,
                  stat_acc1=s2.acc, gamma1=s2.bn.weight, beta1=s2.bn.bias, count=s2.count, eps=s2.eps)
        co = L.op(L.OP_GRAM_COV, dt, groups=G, in0=self.gram_slabs, out=self.gram_cov3, scale_out=self.gram_mu, N=n, Hout=g.h2,
                  Wout=g.w2, Cout=P3)
        gm = L.op(L.OP_GEMM_BF16_NT, dt, in0=self.gram_cov3, w=cv3.w, out=self.gram_T, N=G * 3 * P3, Hout=1, Wout=1, Cin=P3, Cout=N3)
        tab = self.alloc((G, 2, N3), torch.float32)
        fb = L.op(L.OP_BN_FROM_GRAM, dt, groups=G, in0=self.gram_T, in1=self.gram_mu, w=cv3.w, scale_out=tab, gamma=bn3.weight,
                  beta=bn3.bias, running_mean=bn3.running_mean, running_var=bn3.running_var, Cin=P3, Cout=N3,
                  count=n * g.h2 * g.w2, momentum=BN_MOMENTUM, eps=BN_EPS)
        # no statistics of its own: bn3's came from its input
        cv3.scale1, cv3.shift1, cv3.in1 = tab[0, 0].data_ptr(), tab[0, 1].data_ptr(), self.y.data_ptr()
        cv3.flags = 1 | L.CONV_GROUP_TABLE
        self.ops += [gr, co, gm, fb, cv3]
        self.gram_blocks += 1
        self._swap()

    def _eval_fused_block(self, blk, g):
        """inference: every BatchNorm is a fixed per-channel affine -> it rides in the producing conv's epilogue together with the
        residual add and the ReLU: 3-4 launches per bottleneck instead of 6-8"""
        self._conv_affine(blk.conv1, blk.bn1, self.y, self.a1, g.h, g.w, g.h, g.w, True)
        self._conv_affine(blk.conv2, blk.bn2, self.a1, self.a2, g.h, g.w, g.h2, g.w2, True)
        resid = self.y
        if blk.downsample is not None:
            self._conv_affine(blk.downsample[0], blk.downsample[1], self.y, self.cd, g.h, g.w, g.h2, g.w2, False)
            resid = self.cd
        self._conv_affine(blk.conv3, blk.bn3, self.a2, self.ynext, g.h2, g.w2, g.h2, g.w2, True, resid)
        self._swap()

    def _conv_affine(self, conv, bn, x, out, hin, win, hout, wout, relu, resid=None):
        cv = self._conv(conv, x, out, hin, win, hout, wout)
        src = self.bn_stats(cv, bn)
        cv.scale1, cv.shift1, cv.flags = src.scale, src.shift, 1 if relu else 0
        if resid is not None:
            cv.in1 = resid.data_ptr()
        self.ops.append(cv)


def conv_flops(arch, H=224, W=224):
    """Algorithmic FLOPs (2*MAC) per image of the conv stack (23.02 GFLOP at 224x224 for ResNet-152)."""
    width = arch["width"]
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    fl = 2.0 * Ho * Wo * 3 * 49 * width
    h, w_ = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
    inpl = width
    for li, nblocks in enumerate(arch["layers"]):
        planes = width * (2 ** li)
        for b in range(nblocks):
            stride = 2 if (li > 0 and b == 0) else 1
            h2, w2 = (h + 2 - 3) // stride + 1, (w_ + 2 - 3) // stride + 1
            fl += 2.0 * h * w_ * inpl * planes
            fl += 2.0 * h2 * w2 * planes * planes * 9
            fl += 2.0 * h2 * w2 * planes * planes * 4
            if b == 0 and (stride != 1 or inpl != planes * 4):
                fl += 2.0 * h2 * w2 * inpl * planes * 4
            h, w_, inpl = h2, w2, planes * 4
    return fl
