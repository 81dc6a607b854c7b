"""Plain CPU reference of the elementwise kernels (csrc/sat_elementwise.hip): BatchNorm finalize / slab reducer / derived table,
normalise (+ReLU, +residual, +maxpool), global average pool, the eval table and the deferred running-statistics update, row-wise
softmax cross entropy, column sums, the BatchNorm1d head, clamp + Adam, the embedding gather and scatter.  Written from the formulas
in the kernel comments.  A helper module like attend_step_reference.py: no GPU, no test in it.

Every formula runs in the dtype it is asked for: float64 is the reference, float32 the "restatement" whose error against float64
sets the second tolerance of the GPU test at a case (tests/test_elementwise_reference_host.py measures it, F32_ERR keeps it,
tests/test_gpu_elementwise_edges.py allows TOL_FACTOR x that value).  The functions take the operands the kernels take: BN finalize
the f32 per-tile slabs, the derived table the int64 fixed-point accumulators (scale 2^22); both form mean and variance in float64
as the kernels do, so the restatement differs from the reference in the arithmetic AFTER those sums only.  Hyper-parameters that
cross the C ABI as `float` (momentum, eps, beta1, ...) enter as their float32 values.

The case tables and the seeded inputs of the GPU sweep live here too, so that the host test measures exactly the cases the GPU test
runs."""
import math

import numpy as np
import torch

STAT_SCALE = 2.0 ** 22      # SAT_STAT_SCALE: the fixed point of the integer BatchNorm accumulators
TOL_FACTOR = 8.0            # GPU tolerance = TOL_FACTOR x the f32 restatement's error (the kernels sum in another order than torch)
BF16_ROUND = 2.0 ** -8      # one bf16 rounding of a result, relative
BN_MOMENTUM, BN_EPS = 0.1, 1e-5
F64, F32 = torch.float64, torch.float32


def f32v(x):
    """the value a python float has once it crossed the C ABI as `float`"""
    return float(np.float32(x))


def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))


def bf16_valued(t):
    return t.bfloat16().float()


# ---------------------------------------------------------------------------------------------- the cases of the GPU sweep

BN_SMALL = {"f32": [(1, 1, 1, 8), (3, 10, 10, 32), (2, 5, 5, 24), (2, 7, 7, 2048)],
            "bf16": [(1, 1, 1, 8), (3, 10, 10, 32), (2, 5, 5, 48), (2, 7, 7, 2048)]}
BN_LARGE = {"f32": [(13, 56, 56, 64), (17, 56, 56, 64), (7, 56, 56, 40)], "bf16": [(13, 56, 56, 128), (17, 56, 56, 128)]}
BN_GROUPED = (2, 5, 5, 32)          # per group; groups = 3
BN_GROUPS = 3
SLICE_SHAPES = [(2, 5, 5, 32)]      # into a wide tensor of ldc = 80 at channel offset 16
SLICE_LDC, SLICE_OFF = 80, 16
POOL_SHAPES = [(1, 1, 1, 8), (1, 2, 2, 8), (2, 5, 7, 8), (1, 9, 12, 16), (1, 10, 10, 32)]
POOL_LARGE = (4, 112, 112, 64)      # f32 only: 200,704 items
AVG_HW, AVG_C, AVG_N = [1, 3, 4, 49, 50], [8, 2048], [1, 3]
FIN_TILES, FIN_C = [1, 31, 32, 33, 127, 128, 129, 300], [4, 40, 64]
FIN_ROWS = 8                        # rows per tile of the synthetic activations behind the slabs
SLAB_TILES, SLAB_C = [1, 127, 128, 129, 300], 40
EVAL_C = [1, 255, 256, 257, 600]
CE_V = [1, 3, 4, 5, 255, 1003, 1024, 12288, 12289, 12292]
CE_KINDS = ["equal", "dominant", "low", "shifted", "random"]
CE_INV = 1.0 / 50.0
CE_LOSS_N, CE_LOSS_V = [1, 255, 257], 1003
COLSUM_ROWS, COLSUM_COLS = [1, 7, 8, 9, 24, 25, 32, 33, 57], [1, 31, 32, 33, 100]
ADAM_N, ADAM_CLIP = [1, 3, 4, 5, 1023, 786439], [0.0, 0.1]
ADAM_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
BN1D_SHAPES = [(1, 8, 4), (2, 16, 32), (7, 64, 33), (8, 64, 31), (9, 256, 40), (12, 256, 32)]      # (B, F, E)
BN1D_MOMENTUM = 0.01
# name -> (lengths sorted decreasing, E, V, how the tokens are drawn)
EMBED_CASES = {"t1": ([1, 1, 1], 8, 11, "random"), "ragged_e1": ([6, 4, 4, 1], 1, 9, "random"),
               "ragged_e255": ([5, 3, 2], 255, 7, "random"), "same_e256": ([4, 4, 3, 2, 2], 256, 5, "same"),
               "repeat_e257": ([7, 6, 6, 3, 1, 1], 257, 4, "random"), "clamped": ([4, 3, 3], 8, 6, "bad")}


# ---------------------------------------------------------------------------------------------- BatchNorm statistics

def stats_tail(mean, var, count, gamma, beta, rm, rv, momentum, eps, dtype):
    """(scale, shift) and the running statistics from a float64 (mean, biased variance): the part of bn_finalize_kernel / bn_table
    after the sums, in `dtype`.  The batch statistics enter the running update as their float32 values (bn_table's comment)."""
    m, e = f32v(momentum), f32v(eps)
    scale = gamma.to(dtype) / torch.sqrt(var.to(dtype) + e)
    out = dict(scale=scale, shift=beta.to(dtype) - mean.to(dtype) * scale)
    if rm is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        out["running_mean"] = (1.0 - m) * rm.to(dtype) + m * mean.float().to(dtype)
        out["running_var"] = (1.0 - m) * rv.to(dtype) + m * unbiased.float().to(dtype)
    return out


def bn_finalize(partial, count, gamma, beta, rm, rv, momentum, eps, training, dtype=F64):
    """partial: f32 slabs [tiles, 2, C] (row 0 sums, row 1 sums of squares).  training: batch statistics, var clamped at 0, running
    statistics updated when given; else (scale, shift) from the running statistics, which stay."""
    if not training:
        return stats_tail(rm.double(), rv.double(), count, gamma, beta, None, None, momentum, eps, dtype)
    mean = partial[:, 0].double().sum(0) / count
    var = (partial[:, 1].double().sum(0) / count - mean * mean).clamp(min=0.0)
    return stats_tail(mean, var, count, gamma, beta, rm, rv, momentum, eps, dtype)


def bn_table_from_acc(acc, count, gamma, beta, rm, rv, momentum, eps, dtype=F64):
    """acc: int64 [2, C], the column sums and sums of squares times 2^22"""
    mean = acc[0].double() / (STAT_SCALE * count)
    var = (acc[1].double() / (STAT_SCALE * count) - mean * mean).clamp(min=0.0)
    return stats_tail(mean, var, count, gamma, beta, rm, rv, momentum, eps, dtype)


def slabs_to_acc(partial):
    """int64 [2, C]: what the slab reducer ADDS to the accumulators; exact when every slab value is a small dyadic rational"""
    return torch.round(partial.double().sum(0) * STAT_SCALE).long()


def running_apply(rm, rv, bm, bv, momentum):
    """the deferred update: one float64 expression on float32 operands, rounded once"""
    m = f32v(momentum)
    return ((1.0 - m) * rm.double() + m * bm.double()).float(), ((1.0 - m) * rv.double() + m * bv.double()).float()


# ---------------------------------------------------------------------------------------------- normalise, pools

def bn_act(x, scale, shift, z=None, scale1=None, shift1=None):
    """relu(x*s + t), relu(x*s + t + z), relu(x*s + t + (z*s1 + t1)); NHWC, the tables broadcast over the last axis"""
    y = x * scale + shift
    if z is not None:
        y = y + (z * scale1 + shift1 if scale1 is not None else z)
    return y.clamp(min=0)


def bn_relu_maxpool(x, scale, shift):
    """max over 3x3 windows, stride 2, pad 1, of relu(x*s + t); NHWC.  relu >= 0, so the border pads with 0."""
    a = (x * scale + shift).clamp(min=0)
    N, H, W, C = a.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ap = torch.zeros(N, H + 2, W + 2, C, dtype=a.dtype)
    ap[:, 1:H + 1, 1:W + 1] = a
    out = torch.zeros(N, Ho, Wo, C, dtype=a.dtype)
    for dh in range(3):
        for dw in range(3):
            out = torch.maximum(out, ap[:, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2])
    return out


def avgpool(x):
    """[N, HW, C] -> [N, C]"""
    return x.sum(1) / x.shape[1]


def bn_inputs(dtype_name, shape, seed=0):
    """Seeded operands of one normalise case: x, z (bf16-valued for bf16), two given f32 tables, and two BatchNorms whose statistics
    arrive as integer sums -- well-conditioned synthetic ones (mean ~ N(0.3, 0.5), variance in [0.5, 2]) at count = N*H*W, not the
    statistics of x, so that a one-pixel case does not divide by sqrt(eps)."""
    N, H, W, C = shape
    g = gen(1, N, H, W, C, seed, dtype_name == "bf16")
    r = lambda *s: torch.randn(*s, generator=g)
    x, z = r(N, H, W, C) * 2 + 0.5, r(N, H, W, C)
    if dtype_name == "bf16":
        x, z = bf16_valued(x), bf16_valued(z)
    d = dict(x=x, z=z, count=N * H * W)
    for k in ("", "1"):
        d["scale" + k], d["shift" + k] = torch.rand(C, generator=g) + 0.5, r(C) * 0.3
        d["gamma" + k], d["beta" + k] = torch.rand(C, generator=g) + 0.5, r(C) * 0.1
        d["rm" + k], d["rv" + k] = r(C) * 0.2, torch.rand(C, generator=g) + 0.5
        mean, var = r(C).double() * 0.5 + 0.3, torch.rand(C, generator=g).double() * 1.5 + 0.5
        d["acc" + k] = torch.stack([torch.round(mean * d["count"] * STAT_SCALE),
                                    torch.round((var + mean * mean) * d["count"] * STAT_SCALE)]).long()
    return d


BN_OUTPUTS = ("relu", "add", "add_b1", "relu_derived", "add_derived", "scale", "shift", "running_mean", "running_var")


def bn_case(dtype_name, shape, dtype=F64, seed=0, names=None):
    """every form of the normalise kernels at one shape, in `dtype` (outputs before any bf16 rounding); names: only these forms"""
    d = bn_inputs(dtype_name, shape, seed)
    c = lambda k: d[k].to(dtype)
    t0 = bn_table_from_acc(d["acc"], d["count"], d["gamma"], d["beta"], d["rm"], d["rv"], BN_MOMENTUM, BN_EPS, dtype)
    t1 = bn_table_from_acc(d["acc1"], d["count"], d["gamma1"], d["beta1"], d["rm1"], d["rv1"], BN_MOMENTUM, BN_EPS, dtype)
    forms = dict(relu=lambda: bn_act(c("x"), c("scale"), c("shift")), add=lambda: bn_act(c("x"), c("scale"), c("shift"), c("z")),
                 add_b1=lambda: bn_act(c("x"), c("scale"), c("shift"), c("z"), c("scale1"), c("shift1")),
                 relu_derived=lambda: bn_act(c("x"), t0["scale"], t0["shift"]),
                 add_derived=lambda: bn_act(c("x"), t0["scale"], t0["shift"], c("z"), t1["scale"], t1["shift"]),
                 pool=lambda: bn_relu_maxpool(c("x"), c("scale"), c("shift")),
                 pool_derived=lambda: bn_relu_maxpool(c("x"), t0["scale"], t0["shift"]))
    out = {k: f() for k, f in forms.items() if names is None or k in names}
    out.update(t0)
    out.update({k + "1": v for k, v in t1.items()})
    return out


GROUPED_FORMS = ("relu", "add", "slice", "pool")
GROUPED_OUTPUTS = ("y", "running_mean", "running_var")


def grouped_inputs(dtype_name):
    """one batch per group (seeds 1..G); gamma / beta (and gamma1 / beta1) of group 0 serve every group, as in a grouped program"""
    return [bn_inputs(dtype_name, BN_GROUPED, seed=g + 1) for g in range(BN_GROUPS)]


def grouped_case(dtype_name, form, dtype=F64):
    """a grouped launch with derived tables: every group has its own integer sums and its own row of the running-statistics log"""
    ds = grouped_inputs(dtype_name)
    d0, ys, rms, rvs = ds[0], [], [], []
    for d in ds:
        c = lambda k: d[k].to(dtype)
        t0 = bn_table_from_acc(d["acc"], d["count"], d0["gamma"], d0["beta"], d["rm"], d["rv"], BN_MOMENTUM, BN_EPS, dtype)
        if form == "add":
            t1 = bn_table_from_acc(d["acc1"], d["count"], d0["gamma1"], d0["beta1"], None, None, BN_MOMENTUM, BN_EPS, dtype)
            ys.append(bn_act(c("x"), t0["scale"], t0["shift"], c("z"), t1["scale"], t1["shift"]))
        elif form == "pool":
            ys.append(bn_relu_maxpool(c("x"), t0["scale"], t0["shift"]))
        else:
            ys.append(bn_act(c("x"), t0["scale"], t0["shift"]))
        rms.append(t0["running_mean"])
        rvs.append(t0["running_var"])
    return dict(y=torch.stack(ys), running_mean=torch.stack(rms), running_var=torch.stack(rvs))


def grouped_f32_error(dtype_name, form):
    r64, r32 = grouped_case(dtype_name, form), grouped_case(dtype_name, form, F32)
    return r64, {k: max_err(r32[k], r64[k]) for k in GROUPED_OUTPUTS}


def max_err(a, b):
    return (a.double() - b.double()).abs().max().item() if a.numel() else 0.0


def bn_f32_error(dtype_name, shape, names=BN_OUTPUTS, seed=0):
    r64, r32 = bn_case(dtype_name, shape, F64, seed, names), bn_case(dtype_name, shape, F32, seed, names)
    return r64, {k: max_err(r32[k], r64[k]) for k in names}


def avgpool_inputs(dtype_name, N, HW, C):
    x = torch.randn(N, HW, C, generator=gen(2, N, HW, C)) + 0.5
    return bf16_valued(x) if dtype_name == "bf16" else x


def avgpool_f32_error(dtype_name, N, HW, C):
    x = avgpool_inputs(dtype_name, N, HW, C)
    r64 = avgpool(x.double())
    return r64, dict(out=max_err(avgpool(x), r64))


def finalize_inputs(tiles, C, rows=FIN_ROWS):
    """f32 slabs of `tiles` tiles of `rows` rows of seeded activations; channel 1 is the constant 0.5: its sums are exact, cancel to
    a variance of exactly 0 in float64 too, and scale = gamma / sqrt(eps)"""
    g = gen(3, tiles, C, rows)
    x = torch.randn(tiles, rows, C, generator=g) * 1.5 + 0.7
    x[:, :, 1] = 0.5
    part = torch.stack([x.sum(1), (x * x).sum(1)], 1).contiguous()           # [tiles, 2, C], f32 sums
    return dict(partial=part, count=tiles * rows, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.1,
                rm=torch.randn(C, generator=g) * 0.2, rv=torch.rand(C, generator=g) + 0.5)


FIN_OUTPUTS = ("scale", "shift", "running_mean", "running_var", "eval_scale", "eval_shift")


def finalize_case(tiles, C, dtype=F64, rows=FIN_ROWS):
    d = finalize_inputs(tiles, C, rows)
    out = bn_finalize(d["partial"], d["count"], d["gamma"], d["beta"], d["rm"], d["rv"], BN_MOMENTUM, BN_EPS, 1, dtype)
    ev = bn_finalize(None, d["count"], d["gamma"], d["beta"], d["rm"], d["rv"], BN_MOMENTUM, BN_EPS, 0, dtype)
    out["eval_scale"], out["eval_shift"] = ev["scale"], ev["shift"]
    return out


def finalize_f32_error(tiles, C, rows=FIN_ROWS):
    r64, r32 = finalize_case(tiles, C, F64, rows), finalize_case(tiles, C, F32, rows)
    return r64, {k: max_err(r32[k], r64[k]) for k in FIN_OUTPUTS}


def slab_inputs(tiles, C, groups):
    """slabs whose values are integer multiples of 2^-10 below 16 (sums of squares: non-negative): every float64 sum of them is
    exact in any order, and so is the product with 2^22"""
    g = gen(4, tiles, C, groups)
    k = torch.randint(-2 ** 14, 2 ** 14, (groups, tiles, 2, C), generator=g)
    k[:, :, 1] = k[:, :, 1].abs()
    return (k.double() * 2.0 ** -10).float(), torch.randint(-10 ** 6, 10 ** 6, (groups, 2, 2, C), generator=g)


# ---------------------------------------------------------------------------------------------- cross entropy, column sums

def ce_inputs(V):
    """logits [35, V] (every row kind with every placed target once) and the placed targets: 0, V-1, the first element of the scalar
    tail 4*(V/4), 1023, 1024, and -1 and V, which the kernel clamps"""
    g = gen(5, V)
    kinds = [CE_KINDS[i % 5] for i in range(35)]
    placed = [0, V - 1, min(4 * (V // 4), V - 1), 1023, 1024, -1, V]
    targets = torch.tensor([placed[i % 7] for i in range(35)], dtype=torch.int64)
    targets = torch.where((targets > V) & (targets != V), torch.tensor(V - 1), targets)     # 1023 / 1024 beyond a short row
    logits = torch.randn(35, V, generator=g) * 3
    for i, kind in enumerate(kinds):
        if kind == "equal":
            logits[i] = 1.25
        elif kind == "dominant":
            logits[i, (7 * i + 3) % V] = 40.0
        elif kind == "low":
            logits[i] = logits[i] / 3 - 80.0
        elif kind == "shifted":
            logits[i] += 60.0
    return logits, targets, kinds


def ce_rows(logits, targets, scale):
    """row losses lse - x[target], gradient (softmax - onehot) * scale, loss = sum(row loss * scale); scale a float or a per-row
    tensor (weighted form: a row of weight 0 has gradient 0 and no part in the loss, whatever its logits hold)"""
    V = logits.shape[1]
    t = targets.clamp(0, V - 1)
    lse = torch.logsumexp(logits, 1)
    row_loss = lse - logits.gather(1, t[:, None])[:, 0]
    onehot = torch.zeros_like(logits).scatter_(1, t[:, None], 1.0)
    if torch.is_tensor(scale):
        w = scale.to(logits.dtype)
        live = w != 0
        grad = torch.where(live[:, None], (torch.exp(logits - lse[:, None]) - onehot) * w[:, None], torch.zeros_like(logits))
        return dict(row_loss=row_loss, grad=grad, loss=torch.where(live, row_loss * w, torch.zeros_like(w)).sum())
    s = f32v(scale)
    return dict(row_loss=row_loss, grad=(torch.exp(logits - lse[:, None]) - onehot) * s, loss=row_loss.sum() * s)


CE_OUTPUTS = ("row_loss", "grad", "loss")


def ce_f32_error(logits, targets, scale):
    r64 = ce_rows(logits.double(), targets, scale)
    r32 = ce_rows(logits, targets, scale)
    return r64, {k: max_err(r32[k], r64[k]) for k in CE_OUTPUTS}


def ce_loss_inputs(N):
    g = gen(6, N)
    return torch.randn(N, CE_LOSS_V, generator=g) * 3, torch.randint(0, CE_LOSS_V, (N,), generator=g)


def ce_weighted_inputs():
    """B = 3 sampled captions of T = 4 steps over V = 1003 (register path, 3-element scalar tail): logits [T*B, V] of packed rows
    n = t*B + b, ids [B, T + 2] (stride 6), weights with zeros; the rows of weight 0 hold NaN logits; the tail targets 1000..1002"""
    g = gen(7)
    B, T, V = 3, 4, 1003
    logits = torch.randn(T * B, V, generator=g) * 3
    ids = torch.randint(0, V, (B, T + 2), generator=g)
    ids[0, 1], ids[1, 2], ids[2, 0] = 1000, 1002, 1001
    w = torch.randn(T * B, generator=g) * 0.1
    w[4] = 0.0
    w[11] = 0.0
    logits[4] = float("nan")
    logits[11] = float("nan")
    targets = torch.stack([ids[n % B, n // B] for n in range(T * B)])
    return dict(B=B, T=T, V=V, logits=logits, ids=ids, w=w, targets=targets)


def colsum_inputs(rows, cols):
    """values of the size of the logit gradients the kernel sums in the model (the existing test's 1e-7 belongs to that size)"""
    return torch.randn(rows, cols, generator=gen(8, rows, cols)) * 0.01


def colsum_f32_error(rows, cols):
    x = colsum_inputs(rows, cols)
    return x.double().sum(0), dict(out=max_err(x.sum(0), x.double().sum(0)))


# ---------------------------------------------------------------------------------------------- clamp + Adam

def clamp_adam_step(p, g, m, v, step, clip, lr, beta1, beta2, eps):
    """torch.optim.Adam's single-tensor arithmetic on the clamped gradient, in the dtype of p; returns (p, clamped g, m, v).  The
    bias corrections are python floats (float64) as in torch and in the launcher."""
    b1, b2, e, c = f32v(beta1), f32v(beta2), f32v(eps), f32v(clip)
    if c > 0:
        g = g.clamp(-c, c)
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + ((1.0 - b2) * g) * g
    step_size, bc2_sqrt = f32v(f32v(lr) / (1.0 - b1 ** step)), f32v(math.sqrt(1.0 - b2 ** step))
    return p - step_size * m / (v.sqrt() / bc2_sqrt + e), g, m, v


def adam_inputs(n):
    """parameters, non-zero starting moments (v >= 0) and the gradients of three steps"""
    g = gen(9, n)
    return dict(p=torch.randn(n, generator=g), m=torch.randn(n, generator=g) * 0.05, v=torch.rand(n, generator=g) * 0.01,
                grads=[torch.randn(n, generator=g) * 0.3 for _ in range(3)])


ADAM_OUTPUTS = ("p", "m", "v")


def adam_case(n, clip, dtype=F64):
    """the state after each of three steps: a list of dicts p, g, m, v"""
    d = adam_inputs(n)
    p, m, v = d["p"].to(dtype), d["m"].to(dtype), d["v"].to(dtype)
    out = []
    for step, gr in enumerate(d["grads"], 1):
        p, g, m, v = clamp_adam_step(p, gr.to(dtype), m, v, step, clip, **ADAM_HP)
        out.append(dict(p=p, g=g, m=m, v=v))
    return out


def adam_f32_error(n, clip):
    r64, r32 = adam_case(n, clip), adam_case(n, clip, F32)
    return r64, {k: max(max_err(a[k], b[k]) for a, b in zip(r32, r64)) for k in ADAM_OUTPUTS}


# ---------------------------------------------------------------------------------------------- BatchNorm1d head

def bn1d_inputs(B, Fd, E):
    g = gen(10, B, Fd, E)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(pooled=torch.rand(B, Fd, generator=g), w=r(E, Fd) * (2.0 / Fd ** 0.5), b=r(E) * 0.1, gamma=torch.rand(E, generator=g) + 0.5,
                beta=r(E) * 0.1, rm=r(E) * 0.2, rv=torch.rand(E, generator=g) + 0.5, dy=r(B, E))


def bn1d_fwd(pooled, w, b, gamma, beta, rm, rv, momentum, eps, training):
    """resnet.fc then BatchNorm1d: z = pooled w^T + b; training: batch mean / biased variance (the unbiased one, or the biased one at
    B = 1, into the running statistics); else the running statistics.  Returns feats, xhat, rstd, running_mean, running_var."""
    m, e = f32v(momentum), f32v(eps)
    z = pooled @ w.t() + b
    B = z.shape[0]
    if training:
        mean = z.mean(0)
        var = ((z - mean) ** 2).sum(0) / B
        unbiased = ((z - mean) ** 2).sum(0) / (B - 1) if B > 1 else var
        rm, rv = (1.0 - m) * rm + m * mean, (1.0 - m) * rv + m * unbiased
    else:
        mean, var = rm, rv
    rstd = 1.0 / torch.sqrt(var + e)
    xhat = (z - mean) * rstd
    return dict(feats=xhat * gamma + beta, xhat=xhat, rstd=rstd, running_mean=rm, running_var=rv)


def bn1d_bwd(dy, pooled, xhat, rstd, gamma):
    """the training-mode backward, from the tape (xhat, rstd) the forward left"""
    B = dy.shape[0]
    dgamma, dbeta = (dy * xhat).sum(0), dy.sum(0)
    dz = (gamma * rstd / B) * (B * dy - dbeta - xhat * dgamma)
    return dict(dgamma=dgamma, dbeta=dbeta, dw=dz.t() @ pooled, db=dz.sum(0))


BN1D_OUTPUTS = ("feats", "xhat", "rstd", "running_mean", "running_var", "dgamma", "dbeta", "dw", "db")


def bn1d_case(shape, training, dtype=F64):
    """forward in `dtype`; the backward from the FLOAT32 values of the float64 forward's tape, which is what the GPU test hands
    the backward kernel (so the backward is judged on its own operands)"""
    d = bn1d_inputs(*shape)
    c = lambda k: d[k].to(dtype)
    out = bn1d_fwd(c("pooled"), c("w"), c("b"), c("gamma"), c("beta"), c("rm"), c("rv"), BN1D_MOMENTUM, BN_EPS, training)
    tape = out if dtype == F64 else bn1d_case(shape, training)
    out.update(bn1d_bwd(c("dy"), c("pooled"), tape["xhat"].float().to(dtype), tape["rstd"].float().to(dtype), c("gamma")))
    return out


def bn1d_f32_error(shape, training):
    r64, r32 = bn1d_case(shape, training), bn1d_case(shape, training, F32)
    return r64, {k: max_err(r32[k], r64[k]) for k in BN1D_OUTPUTS}


# ---------------------------------------------------------------------------------------------- embedding

def batch_sizes(lengths):
    return [sum(1 for l in lengths if l > t) for t in range(int(lengths[0]))]


def embed_inputs(name):
    """lengths count the packed steps of the decoder input [features, embed(captions[:, :-1])]: step 0 is the feature row, step t the
    embedding of captions[b][t-1].  captions [B, Tmax + 1] (the last column only pack_targets reads)."""
    lengths, E, V, how = EMBED_CASES[name]
    g = gen(11, len(lengths), E, V)
    B, T = len(lengths), lengths[0]
    cap = torch.randint(0, V, (B, T + 1), generator=g)
    if how == "same":
        cap[:] = 3
    elif how == "bad":
        cap[0, 0], cap[1, 1], cap[2, 0] = -1, V, V + 5
    bs = batch_sizes(lengths)
    prefix = torch.tensor([0] + list(np.cumsum(bs)), dtype=torch.int32)
    N = int(prefix[-1])
    return dict(lengths=lengths, B=B, T=T, E=E, V=V, N=N, captions=cap, prefix=prefix, bs=bs,
                features=torch.randn(B, E, generator=g), embed=torch.randn(V, E, generator=g), dX=torch.randn(N, E, generator=g))


def packed_rows(bs):
    """(t, b) of every packed row"""
    return [(t, b) for t, n in enumerate(bs) for b in range(n)]


def embed_concat_fwd(features, embed, captions, bs):
    """X[row(t, b)] = features[b] at t = 0, embed[clamp(captions[b][t-1])] after"""
    V = embed.shape[0]
    return torch.stack([features[b] if t == 0 else embed[int(captions[b, t - 1].clamp(0, V - 1))] for t, b in packed_rows(bs)])


def embed_concat_bwd(dX, captions, bs, V, row_ordered_f32=False):
    """d_features = the step-0 rows; d_embed[v] = the sum of the rows of token v -- in float64, or (row_ordered_f32) in float32 one
    row after the other in ascending row order starting from the first, the order embed_concat_bwd_kernel documents"""
    B = bs[0]
    x = dX.numpy().astype(np.float32 if row_ordered_f32 else np.float64)
    table = np.zeros((V, x.shape[1]), dtype=x.dtype)
    seen = np.zeros(V, dtype=bool)
    for i, (t, b) in enumerate(packed_rows(bs)):
        if t == 0:
            continue
        v = int(captions[b, t - 1].clamp(0, V - 1))
        table[v] = table[v] + x[i] if seen[v] else x[i]
        seen[v] = True
    return torch.from_numpy(x[:B].copy()), torch.from_numpy(table)


def pack_targets(captions, bs):
    """targets[row(t, b)] = captions[b][t + 1]"""
    return torch.stack([captions[b, t + 1] for t, b in packed_rows(bs)])


def embed_f32_error(name):
    d = embed_inputs(name)
    _, t64 = embed_concat_bwd(d["dX"], d["captions"], d["bs"], d["V"])
    _, t32 = embed_concat_bwd(d["dX"], d["captions"], d["bs"], d["V"], row_ordered_f32=True)
    return t64, dict(d_embed=max_err(t32, t64))


# ---------------------------------------------------------------------------------------------- the tolerance table

def measure_all(large=True):
    """{key: tuple of max abs errors of the float32 restatement against float64}, every case of the sweep: what F32_ERR freezes"""
    out = {}
    for dn in ("f32", "bf16"):
        for form in GROUPED_FORMS:
            if form == "pool" and dn == "f32":
                continue                    # the f32 maxpool launcher has no grouped form
            out[("grouped", dn, form)] = tuple(grouped_f32_error(dn, form)[1].values())
        for shape in BN_SMALL[dn] + SLICE_SHAPES:
            out[("bn", dn, shape)] = tuple(bn_f32_error(dn, shape)[1].values())
        for shape in POOL_SHAPES + ([POOL_LARGE] if dn == "f32" and large else []):
            out[("pool", dn, shape)] = tuple(bn_f32_error(dn, shape, ("pool", "pool_derived"))[1].values())
        if large:
            for shape in BN_LARGE[dn]:
                out[("bn_large", dn, shape)] = tuple(bn_f32_error(dn, shape, ("relu", "add_b1"))[1].values())
        for N in AVG_N:
            for HW in AVG_HW:
                for C in AVG_C:
                    out[("avg", dn, N, HW, C)] = (avgpool_f32_error(dn, N, HW, C)[1]["out"],)
    for tiles in FIN_TILES:
        for C in FIN_C:
            out[("fin", tiles, C)] = tuple(finalize_f32_error(tiles, C)[1].values())
    for C in FIN_C:
        out[("fin_count1", C)] = tuple(finalize_f32_error(1, C, rows=1)[1].values())
    for V in CE_V:
        logits, targets, _ = ce_inputs(V)
        out[("ce", V)] = tuple(ce_f32_error(logits, targets, CE_INV)[1].values())
    for N in CE_LOSS_N:
        out[("ce_loss", N)] = tuple(ce_f32_error(*ce_loss_inputs(N), CE_INV)[1].values())
    d = ce_weighted_inputs()
    live = d["w"] != 0
    out[("ce_weighted",)] = tuple(ce_f32_error(d["logits"][live], d["targets"][live], d["w"][live])[1].values())
    for rows in COLSUM_ROWS:
        for cols in COLSUM_COLS:
            out[("colsum", rows, cols)] = (colsum_f32_error(rows, cols)[1]["out"],)
    for n in ADAM_N:
        if n < 10 ** 5 or large:
            for clip in ADAM_CLIP:
                out[("adam", n, clip)] = tuple(adam_f32_error(n, clip)[1].values())
    for shape in BN1D_SHAPES:
        for training in (1, 0):
            out[("bn1d", shape, training)] = tuple(bn1d_f32_error(shape, training)[1].values())
    for name in EMBED_CASES:
        out[("embed", name)] = (embed_f32_error(name)[1]["d_embed"],)
    return out


ERR_NAMES = {"bn": BN_OUTPUTS, "grouped": GROUPED_OUTPUTS, "pool": ("pool", "pool_derived"), "bn_large": ("relu", "add_b1"), "avg": ("out",), "fin": FIN_OUTPUTS,
             "fin_count1": FIN_OUTPUTS, "ce": CE_OUTPUTS, "ce_loss": CE_OUTPUTS, "ce_weighted": CE_OUTPUTS, "colsum": ("out",),
             "adam": ADAM_OUTPUTS, "bn1d": BN1D_OUTPUTS, "embed": ("d_embed",)}

# The float32 restatement's max abs error against float64 at every case of the sweep, as test_elementwise_reference_host.py measured
# it (`measure_all()`, 3 digits; torch 2.x CPU).  FROZEN: torch's float32 summation order depends on the host, so the GPU test reads
# its tolerance from here, not from the machine it happens to run on; the host test re-measures and compares.
F32_ERR = {
    ('grouped', 'f32', 'relu'): (1.3e-06, 3.13e-08, 1.42e-07),
    ('grouped', 'f32', 'add'): (1.96e-06, 3.13e-08, 1.42e-07),
    ('grouped', 'f32', 'slice'): (1.3e-06, 3.13e-08, 1.42e-07),
    ('bn', 'f32', (1, 1, 1, 8)): (9.78e-08, 9.78e-08, 1.96e-07, 4.62e-08, 2.26e-07, 3.36e-08, 8.59e-08, 6.44e-09, 3.63e-08),
    ('bn', 'f32', (3, 10, 10, 32)): (5.51e-07, 8.86e-07, 6.66e-07, 6.53e-07, 9e-07, 6.61e-08, 1.19e-07, 2.42e-08, 1.2e-07),
    ('bn', 'f32', (2, 5, 5, 24)): (4.28e-07, 5.86e-07, 5.08e-07, 7.85e-07, 7e-07, 6.83e-08, 1.78e-07, 2.21e-08, 7.12e-08),
    ('bn', 'f32', (2, 7, 7, 2048)): (9.08e-07, 1.13e-06, 1.36e-06, 1.34e-06, 1.74e-06, 1.8e-07, 2.75e-07, 5.18e-08, 1.43e-07),
    ('bn', 'f32', (2, 5, 5, 32)): (5.22e-07, 6.15e-07, 9.02e-07, 6.92e-07, 6.56e-07, 8.64e-08, 9.49e-08, 3.27e-08, 1.08e-07),
    ('pool', 'f32', (1, 1, 1, 8)): (9.78e-08, 4.62e-08),
    ('pool', 'f32', (1, 2, 2, 8)): (1.24e-07, 2.6e-07),
    ('pool', 'f32', (2, 5, 7, 8)): (6.56e-07, 5.39e-07),
    ('pool', 'f32', (1, 9, 12, 16)): (4.6e-07, 5.44e-07),
    ('pool', 'f32', (1, 10, 10, 32)): (5.12e-07, 1.22e-06),
    ('pool', 'f32', (4, 112, 112, 64)): (9.46e-07, 1.43e-06),
    ('bn_large', 'f32', (13, 56, 56, 64)): (9.03e-07, 1.32e-06),
    ('bn_large', 'f32', (17, 56, 56, 64)): (8.84e-07, 1.26e-06),
    ('bn_large', 'f32', (7, 56, 56, 40)): (8.8e-07, 1.3e-06),
    ('avg', 'f32', 1, 1, 8): (0,), ('avg', 'f32', 1, 1, 2048): (0,), ('avg', 'f32', 1, 3, 8): (3.97e-08,),
    ('avg', 'f32', 1, 3, 2048): (1.59e-07,), ('avg', 'f32', 1, 4, 8): (5.22e-08,), ('avg', 'f32', 1, 4, 2048): (1.49e-07,),
    ('avg', 'f32', 1, 49, 8): (4.32e-08,), ('avg', 'f32', 1, 49, 2048): (1.59e-07,), ('avg', 'f32', 1, 50, 8): (7.81e-08,),
    ('avg', 'f32', 1, 50, 2048): (1.34e-07,), ('avg', 'f32', 3, 1, 8): (0,), ('avg', 'f32', 3, 1, 2048): (0,),
    ('avg', 'f32', 3, 3, 8): (5.96e-08,), ('avg', 'f32', 3, 3, 2048): (1.99e-07,), ('avg', 'f32', 3, 4, 8): (7.45e-08,),
    ('avg', 'f32', 3, 4, 2048): (1.79e-07,), ('avg', 'f32', 3, 49, 8): (5.53e-08,), ('avg', 'f32', 3, 49, 2048): (1.47e-07,),
    ('avg', 'f32', 3, 50, 8): (7.21e-08,), ('avg', 'f32', 3, 50, 2048): (1.41e-07,),
    ('grouped', 'bf16', 'relu'): (7.17e-07, 2.08e-08, 1.24e-07),
    ('grouped', 'bf16', 'add'): (8.9e-07, 2.08e-08, 1.24e-07),
    ('grouped', 'bf16', 'slice'): (7.17e-07, 2.08e-08, 1.24e-07),
    ('grouped', 'bf16', 'pool'): (7.17e-07, 2.08e-08, 1.24e-07),
    ('bn', 'bf16', (1, 1, 1, 8)): (3.17e-08, 3.93e-08, 7.17e-08, 3.32e-08, 1.35e-07, 6.32e-08, 4.93e-08, 1.38e-08, 9.56e-08),
    ('bn', 'bf16', (3, 10, 10, 32)): (5.07e-07, 5.96e-07, 6.69e-07, 7.74e-07, 8.06e-07, 1.02e-07, 1.12e-07, 1.74e-08, 1.08e-07),
    ('bn', 'bf16', (2, 5, 5, 48)): (4.6e-07, 5.63e-07, 7.02e-07, 6.85e-07, 9.58e-07, 8.98e-08, 6.79e-08, 2.4e-08, 1.19e-07),
    ('bn', 'bf16', (2, 7, 7, 2048)): (9.42e-07, 9.42e-07, 1.33e-06, 1.57e-06, 1.65e-06, 1.59e-07, 3.39e-07, 4.84e-08, 1.44e-07),
    ('bn', 'bf16', (2, 5, 5, 32)): (4.58e-07, 8.2e-07, 7e-07, 5.47e-07, 5.95e-07, 6.83e-08, 9.71e-08, 2.25e-08, 8.25e-08),
    ('pool', 'bf16', (1, 1, 1, 8)): (3.17e-08, 3.32e-08),
    ('pool', 'bf16', (1, 2, 2, 8)): (4.14e-07, 3.25e-07),
    ('pool', 'bf16', (2, 5, 7, 8)): (4.62e-07, 7.71e-07),
    ('pool', 'bf16', (1, 9, 12, 16)): (3.78e-07, 5.64e-07),
    ('pool', 'bf16', (1, 10, 10, 32)): (4.45e-07, 7.93e-07),
    ('bn_large', 'bf16', (13, 56, 56, 128)): (9.42e-07, 1.38e-06),
    ('bn_large', 'bf16', (17, 56, 56, 128)): (9.46e-07, 1.41e-06),
    ('avg', 'bf16', 1, 1, 8): (0,), ('avg', 'bf16', 1, 1, 2048): (0,), ('avg', 'bf16', 1, 3, 8): (3.97e-08,),
    ('avg', 'bf16', 1, 3, 2048): (7.95e-08,), ('avg', 'bf16', 1, 4, 8): (0,), ('avg', 'bf16', 1, 4, 2048): (0,),
    ('avg', 'bf16', 1, 49, 8): (2.92e-08,), ('avg', 'bf16', 1, 49, 2048): (4.74e-08,), ('avg', 'bf16', 1, 50, 8): (1.31e-08,),
    ('avg', 'bf16', 1, 50, 2048): (4.53e-08,), ('avg', 'bf16', 3, 1, 8): (0,), ('avg', 'bf16', 3, 1, 2048): (0,),
    ('avg', 'bf16', 3, 3, 8): (3.97e-08,), ('avg', 'bf16', 3, 3, 2048): (7.95e-08,), ('avg', 'bf16', 3, 4, 8): (0,),
    ('avg', 'bf16', 3, 4, 2048): (0,), ('avg', 'bf16', 3, 49, 8): (2.8e-08,), ('avg', 'bf16', 3, 49, 2048): (5.72e-08,),
    ('avg', 'bf16', 3, 50, 8): (2.86e-08,), ('avg', 'bf16', 3, 50, 2048): (6.68e-08,),
    ('fin', 1, 4): (3.94e-06, 6.61e-06, 9.14e-09, 9.6e-08, 7.91e-08, 1.44e-08),
    ('fin', 1, 40): (1.03e-05, 4.75e-06, 3.66e-08, 9.31e-08, 9.12e-08, 4.44e-08),
    ('fin', 1, 64): (2.8e-06, 3.18e-06, 2.09e-08, 1.08e-07, 9.72e-08, 5.39e-08),
    ('fin', 31, 4): (1.12e-05, 8.88e-06, 1.42e-08, 3.96e-08, 7.18e-08, 1.08e-08),
    ('fin', 31, 40): (6.02e-06, 6.53e-06, 2.51e-08, 9.69e-08, 1.04e-07, 3.67e-08),
    ('fin', 31, 64): (1.09e-05, 1.08e-06, 2.74e-08, 1.2e-07, 1.29e-07, 3.79e-08),
    ('fin', 32, 4): (3.14e-06, 3.1e-06, 1.72e-08, 3.87e-08, 6.66e-08, 2.23e-08),
    ('fin', 32, 40): (4.69e-06, 3.7e-07, 2.21e-08, 1.32e-07, 1.53e-07, 3.31e-08),
    ('fin', 32, 64): (1.2e-05, 8.05e-06, 3.41e-08, 1.08e-07, 9.83e-08, 6.45e-08),
    ('fin', 33, 4): (5.95e-06, 1.21e-06, 3.37e-09, 5.75e-08, 7.74e-08, 1.28e-08),
    ('fin', 33, 40): (6.47e-06, 2.02e-06, 2.98e-08, 7.3e-08, 1.06e-07, 3.82e-08),
    ('fin', 33, 64): (4.05e-06, 4.24e-06, 2.82e-08, 1.21e-07, 9.49e-08, 3.59e-08),
    ('fin', 127, 4): (1.01e-05, 2.27e-06, 1.28e-08, 6.78e-08, 1.07e-07, 3.12e-08),
    ('fin', 127, 40): (1.62e-05, 1.53e-05, 2.13e-08, 1.32e-07, 1.13e-07, 3.89e-08),
    ('fin', 127, 64): (8.76e-06, 2.95e-06, 3e-08, 1.21e-07, 1.32e-07, 8.07e-08),
    ('fin', 128, 4): (1.63e-05, 8.04e-06, 5.17e-09, 3.41e-08, 7.76e-08, 7.76e-09),
    ('fin', 128, 40): (2.94e-06, 7.68e-06, 2.23e-08, 9.69e-08, 1.21e-07, 3.1e-08),
    ('fin', 128, 64): (3.66e-06, 1.07e-06, 1.85e-08, 1.21e-07, 9.62e-08, 5.09e-08),
    ('fin', 129, 4): (1.65e-06, 6.86e-08, 2.2e-08, 4.59e-08, 9.36e-08, 4.25e-08),
    ('fin', 129, 40): (1.34e-06, 3.08e-06, 2.75e-08, 9.68e-08, 9.53e-08, 4.29e-08),
    ('fin', 129, 64): (1.6e-05, 2.05e-06, 2.26e-08, 1.21e-07, 1.07e-07, 4.48e-08),
    ('fin', 300, 4): (5.44e-06, 6.1e-06, 6.77e-09, 4.95e-08, 5.53e-08, 1.4e-08),
    ('fin', 300, 40): (3.96e-07, 7.33e-06, 2.82e-08, 1.2e-07, 9.91e-08, 5.82e-08),
    ('fin', 300, 64): (9.83e-06, 8.53e-06, 2.71e-08, 1.09e-07, 1.22e-07, 4.45e-08),
    ('fin_count1', 4): (1.59e-05, 3.74e-05, 3e-08, 5.85e-08, 2.8e-08, 3.12e-08),
    ('fin_count1', 40): (1.67e-05, 7.53e-05, 3.26e-08, 8.15e-08, 1.27e-07, 5.77e-08),
    ('fin_count1', 64): (2.54e-05, 6.51e-05, 3.5e-08, 1.26e-07, 9.86e-08, 3.8e-08),
    ('ce', 1): (0, 0, 0),
    ('ce', 3): (3.8e-06, 6.04e-08, 3.68e-07),
    ('ce', 4): (3.77e-06, 4.63e-08, 3.26e-07),
    ('ce', 5): (3.56e-06, 4.54e-08, 3.91e-07),
    ('ce', 255): (3.51e-06, 3.85e-08, 1.29e-07),
    ('ce', 1003): (3.7e-06, 1.8e-08, 5.25e-07),
    ('ce', 1024): (3.08e-06, 4.15e-08, 4.23e-08),
    ('ce', 12288): (3.95e-06, 1.25e-08, 7.86e-07),
    ('ce', 12289): (3.94e-06, 2.1e-08, 4e-07),
    ('ce', 12292): (3.69e-06, 3.35e-08, 1.12e-07),
    ('ce_loss', 1): (4.19e-07, 5.14e-10, 1.97e-10),
    ('ce_loss', 255): (1.59e-06, 8.04e-09, 4.64e-06),
    ('ce_loss', 257): (1.29e-06, 8.25e-09, 3.22e-06),
    ('ce_weighted',): (6.71e-07, 1.2e-08, 1.48e-07),
    ('colsum', 1, 1): (0,), ('colsum', 1, 31): (0,), ('colsum', 1, 32): (0,), ('colsum', 1, 33): (0,), ('colsum', 1, 100): (0,),
    ('colsum', 7, 1): (9.31e-10,), ('colsum', 7, 31): (2.1e-09,), ('colsum', 7, 32): (3.26e-09,),
    ('colsum', 7, 33): (4.61e-09,), ('colsum', 7, 100): (4.19e-09,), ('colsum', 8, 1): (6.49e-10,),
    ('colsum', 8, 31): (5.26e-09,), ('colsum', 8, 32): (3.26e-09,), ('colsum', 8, 33): (2.62e-09,),
    ('colsum', 8, 100): (5.59e-09,), ('colsum', 9, 1): (1.4e-09,), ('colsum', 9, 31): (2.79e-09,),
    ('colsum', 9, 32): (9.78e-09,), ('colsum', 9, 33): (2.94e-09,), ('colsum', 9, 100): (7.1e-09,),
    ('colsum', 24, 1): (5.82e-11,), ('colsum', 24, 31): (6.78e-09,), ('colsum', 24, 32): (1.02e-08,),
    ('colsum', 24, 33): (7.8e-09,), ('colsum', 24, 100): (1.16e-08,), ('colsum', 25, 1): (5.41e-09,),
    ('colsum', 25, 31): (8.33e-09,), ('colsum', 25, 32): (1.45e-08,), ('colsum', 25, 33): (9.94e-09,),
    ('colsum', 25, 100): (8.96e-09,), ('colsum', 32, 1): (1.57e-09,), ('colsum', 32, 31): (1.06e-08,),
    ('colsum', 32, 32): (1.23e-08,), ('colsum', 32, 33): (1.13e-08,), ('colsum', 32, 100): (1.55e-08,),
    ('colsum', 33, 1): (1.4e-09,), ('colsum', 33, 31): (9.01e-09,), ('colsum', 33, 32): (1.7e-08,),
    ('colsum', 33, 33): (1.11e-08,), ('colsum', 33, 100): (1.99e-08,), ('colsum', 57, 1): (7.63e-09,),
    ('colsum', 57, 31): (1.22e-08,), ('colsum', 57, 32): (1.66e-08,), ('colsum', 57, 33): (2.19e-08,),
    ('colsum', 57, 100): (2.12e-08,),
    ('adam', 1, 0.0): (3.79e-09, 5.18e-10, 1.48e-10),
    ('adam', 1, 0.1): (2.56e-09, 1.41e-09, 4.27e-10),
    ('adam', 3, 0.0): (5.55e-08, 3.02e-09, 2.68e-10),
    ('adam', 3, 0.1): (2.06e-08, 1.59e-09, 5.17e-10),
    ('adam', 4, 0.0): (7.55e-08, 4.51e-09, 6.94e-10),
    ('adam', 4, 0.1): (8.76e-08, 1.59e-09, 7.96e-10),
    ('adam', 5, 0.0): (8.67e-08, 8.68e-09, 1.07e-09),
    ('adam', 5, 0.1): (8.67e-08, 2.68e-09, 9.14e-10),
    ('adam', 1023, 0.0): (2.72e-07, 1.35e-08, 1.66e-09),
    ('adam', 1023, 0.1): (3.02e-07, 1.25e-08, 1.86e-09),
    ('adam', 786439, 0.0): (6.53e-07, 2.58e-08, 2.39e-09),
    ('adam', 786439, 0.1): (6.02e-07, 1.91e-08, 2.37e-09),
    ('bn1d', (1, 8, 4), 1): (0, 0, 1.32e-05, 1.98e-08, 6.17e-08, 0, 0, 0, 0),
    ('bn1d', (1, 8, 4), 0): (1.41e-07, 2.03e-07, 2.88e-08, 0, 0, 3.27e-08, 0, 3.31e-07, 1.96e-07),
    ('bn1d', (2, 16, 32), 1): (4.53e-06, 5.24e-06, 0.000654, 2.53e-08, 1.07e-07, 1.66e-07, 1.19e-07, 6.75e-06, 7.63e-06),
    ('bn1d', (2, 16, 32), 0): (3.58e-07, 3.07e-07, 7.3e-08, 0, 0, 1.5e-07, 1.19e-07, 4.77e-07, 5.19e-07),
    ('bn1d', (7, 64, 33), 1): (1.01e-06, 1.14e-06, 8.58e-07, 2.36e-08, 1.01e-07, 4.05e-07, 6.41e-07, 1.15e-06, 8.54e-07),
    ('bn1d', (7, 64, 33), 0): (1.24e-06, 8.85e-07, 8.6e-08, 0, 0, 2.82e-07, 6.41e-07, 2.4e-06, 1.09e-06),
    ('bn1d', (8, 64, 31), 1): (1.77e-06, 1.26e-06, 9.56e-07, 2.17e-08, 1.13e-07, 4.35e-07, 5.44e-07, 1.22e-06, 1.2e-06),
    ('bn1d', (8, 64, 31), 0): (1.6e-06, 1.28e-06, 8.03e-08, 0, 0, 6.38e-07, 5.44e-07, 3.52e-06, 3.05e-06),
    ('bn1d', (9, 256, 40), 1): (8.69e-07, 9.11e-07, 7.58e-07, 1.86e-08, 8.21e-08, 1.23e-06, 7.67e-07, 1.75e-06, 1.66e-06),
    ('bn1d', (9, 256, 40), 0): (6.93e-07, 5.3e-07, 9.01e-08, 0, 0, 1.05e-06, 7.67e-07, 3.01e-06, 4.33e-06),
    ('bn1d', (12, 256, 32), 1): (2.56e-06, 2.15e-06, 8.64e-07, 1.91e-08, 9.86e-08, 1.4e-06, 8.42e-07, 1.72e-06, 1.42e-06),
    ('bn1d', (12, 256, 32), 0): (1.42e-06, 1.77e-06, 9.51e-08, 0, 0, 1.62e-06, 8.42e-07, 3.42e-06, 4.15e-06),
    ('embed', 't1'): (0,), ('embed', 'ragged_e1'): (2.98e-08,), ('embed', 'ragged_e255'): (1.19e-07,),
    ('embed', 'same_e256'): (1.12e-06,), ('embed', 'repeat_e257'): (7.45e-07,), ('embed', 'clamped'): (4.47e-08,),
}


def f32_err(*key):
    """the frozen errors of one case as a dict by output name"""
    return dict(zip(ERR_NAMES[key[0]], F32_ERR[key]))
