"""Plain CPU reference of the Show-Attend-Tell step kernels (csrc/sat_attend.hip, the LSTM epilogue of csrc/sat_skinny.hip,
`lstm_bwd_point_kernel`, the row utilities), written from the formulas in the kernel comments and `oracle/attend.py`.  A helper
module like alpha_reference.py: no GPU, no test in it.  Every function runs in the dtype of its inputs: the tests feed float64 for
the reference and float32 for the "restatement" whose error against float64 sets the tolerance of the GPU test at a shape
(tests/test_attend_step_reference_host.py computes it, tests/test_gpu_attend_edges.py allows 8 x that value).

The shape tables and the seeded inputs of the GPU sweep live here too, so that the host test measures exactly the cases the GPU
test runs."""
import numpy as np
import torch

# ---------------------------------------------------------------------------------------------- the cases of the GPU sweep

# (rows, P, C): what each reaches is in the table of tests/test_gpu_attend_edges.py
ATT_SHAPES = [(1, 1, 4), (3, 3, 4), (2, 5, 36), (7, 9, 68), (1, 197, 260), (600, 8, 64), (2, 1030, 8), (5, 196, 512)]
ATT_EX_SHAPES = [(2, 5, 36), (7, 9, 68), (1, 197, 260)]
ATT_VALUE_SHAPES = [(2, 5, 36), (5, 196, 512)]
ATT_VALUE_KINDS = ["zero_w", "large", "dominant"]
EX_SCALE = 0.37
LSTM_SHAPES = [(1, 4, 4), (5, 20, 20), (65, 36, 48), (64, 64, 64), (3, 1028, 8)]          # (B, In, H)
BWD_POINT_SHAPES = [(1, 4), (5, 20), (64, 64), (300, 12)]                                 # (n, H)
SPLITK_SHAPES = [(33, 20, 8, 2), (200, 72, 100, 3), (64, 64, 1024, 16)]                   # (M, N, K, ksplit)
TOL_FACTOR = 8.0           # GPU tolerance = TOL_FACTOR x the f32 restatement's error: the kernel sums in another order than torch


def attention_inputs(rows, P, C, kind="plain"):
    """Seeded float32 inputs of one attention step: ctx_enc, feats [rows,P,C], proj [rows,C], w_att [C], d_ctx [rows,C],
    extra [rows,P], and pre_dce / pre_dfe [rows,P,C], the random contents of the two buffers the backward accumulates INTO (a few
    2^-6, so that the rounding of the accumulation stays below the gradients' own error).  kind: "plain" (the distributions of
    test_attention_fwd_bwd_kernels_vs_fp64); "zero_w" (w_att = 0: uniform alpha); "large" (w_att scaled until the scores reach
    +-80); "dominant" (one position per row holds nearly all the weight)."""
    g = torch.Generator().manual_seed(1000 * rows + 10 * P + C)
    ce, fe = torch.randn(rows, P, C, generator=g) * 0.5, torch.randn(rows, P, C, generator=g).clamp(min=0)
    proj, w = torch.randn(rows, C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.1
    dctx, extra = torch.randn(rows, C, generator=g), torch.randn(rows, P, generator=g)
    pre_dce, pre_dfe = torch.randn(rows, P, C, generator=g) * 2.0 ** -6, torch.randn(rows, P, C, generator=g) * 2.0 ** -6
    if kind == "zero_w":
        w = torch.zeros(C)
    elif kind == "large":
        s = torch.tanh(ce.double() + proj.double()[:, None, :]) @ w.double()
        w = (w.double() * (80.0 / s.abs().max().item())).float()
    elif kind == "dominant":
        w = w * (40.0 / w.abs().sum().item())                     # the largest score any position can reach is 40
        for b in range(rows):
            ce[b, (3 * b + 1) % P] = 4.0 * torch.sign(w)           # tanh ~ sign(w): that position scores ~ 40, the others a few units
    else:
        assert kind == "plain"
    return dict(ce=ce, fe=fe, proj=proj, w=w, dctx=dctx, extra=extra, pre_dce=pre_dce, pre_dfe=pre_dfe)


def lstm_inputs(B, In, H):
    g = torch.Generator().manual_seed(77 * B + 5 * In + H)
    k = 1.0 / H ** 0.5
    u = lambda *s: torch.empty(*s).uniform_(-k, k, generator=g)
    return dict(x=torch.randn(B, In, generator=g), h=torch.randn(B, H, generator=g) * 0.5, c=torch.randn(B, H, generator=g),
                w_ih=u(4 * H, In), w_hh=u(4 * H, H), b_ih=u(4 * H), b_hh=u(4 * H))


def bwd_point_inputs(n, H):
    g = torch.Generator().manual_seed(31 * n + H)
    r = lambda *s: torch.randn(*s, generator=g)
    gates = torch.cat([torch.sigmoid(r(n, H)), torch.sigmoid(r(n, H)), torch.tanh(r(n, H)), torch.sigmoid(r(n, H))], 1)
    return dict(dh_out=r(n, H), dh_carry=r(n, H), gates=gates, c=r(n, H), c_prev=r(n, H), dc_state=r(n, H))


# ---------------------------------------------------------------------------------------------- attention step

def attention_step(ctx_enc, feats, proj, w_att):
    """h_att = tanh(ctx_enc + proj); scores = h_att . w_att; alpha = softmax over positions; context = MEAN_p alpha[p] feats[p]."""
    scores = torch.tanh(ctx_enc + proj[:, None, :]) @ w_att
    alpha = torch.softmax(scores, dim=1)
    context = (feats * alpha[:, :, None]).mean(1)
    return scores, alpha, context


def attention_step_grads(ctx_enc, feats, proj, w_att, d_ctx, extra=None, scale=0.0):
    """Forward and, through autograd, the backward of `attention_step` for upstream d_ctx on the context and (optionally)
    scale * extra on alpha.  d_w_att is summed over rows (the kernel returns per-row partials [rows, C])."""
    ce, fe, pj, w = (t.detach().clone().requires_grad_(True) for t in (ctx_enc, feats, proj, w_att))
    scores, alpha, context = attention_step(ce, fe, pj, w)
    loss = (context * d_ctx).sum()
    if extra is not None:
        loss = loss + scale * (extra * alpha).sum()
    loss.backward()
    return dict(scores=scores.detach(), alpha=alpha.detach(), context=context.detach(), d_ctx_enc=ce.grad, d_proj=pj.grad,
                d_w_att=w.grad, d_feats=fe.grad)


ATT_OUTPUTS = ("alpha", "context", "d_ctx_enc", "d_proj", "d_w_att", "d_feats", "acc_ctx_enc", "acc_feats")


def attention_case(rows, P, C, kind="plain", extra=False, dtype=torch.float64):
    """one case of the sweep in `dtype`: the results of `attention_step_grads` plus acc_ctx_enc / acc_feats, the accumulated
    buffers pre + gradient, which is what the kernel leaves in memory"""
    d = {k: v.to(dtype) for k, v in attention_inputs(rows, P, C, kind).items()}
    ex = dict(extra=d["extra"], scale=EX_SCALE) if extra else {}
    r = attention_step_grads(d["ce"], d["fe"], d["proj"], d["w"], d["dctx"], **ex)
    r["acc_ctx_enc"], r["acc_feats"] = d["pre_dce"] + r["d_ctx_enc"], d["pre_dfe"] + r["d_feats"]
    return r


def attention_f32_error(rows, P, C, kind="plain", extra=False):
    """(float64 results, {output: max abs error of the float32 restatement}) for one case of the sweep"""
    r64, r32 = attention_case(rows, P, C, kind, extra), attention_case(rows, P, C, kind, extra, torch.float32)
    return r64, {k: (r32[k].double() - r64[k]).abs().max().item() for k in ATT_OUTPUTS}


def coverage(alpha_packed, batch_sizes, coef):
    """cov[b,p] = sum of alpha over the steps image b is alive in; grad = 2 coef (cov - 1); penalty = coef sum (cov - 1)^2"""
    B, P = int(batch_sizes[0]), alpha_packed.shape[1]
    cov = torch.zeros(B, P, dtype=alpha_packed.dtype)
    r0 = 0
    for bs in batch_sizes:
        cov[:bs] += alpha_packed[r0:r0 + bs]
        r0 += bs
    return cov, 2 * coef * (cov - 1), coef * ((cov - 1) ** 2).sum()


# ---------------------------------------------------------------------------------------------- LSTM cell

def lstmcell_step(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """nn.LSTMCell: returns h', c' and the activated gates (i, f, g, o)"""
    z = x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
    H = h.shape[1]
    i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
    c2 = f * c + i * g
    return o * torch.tanh(c2), c2, (i, f, g, o)


def lstm_f32_error(B, In, H):
    d = lstm_inputs(B, In, H)
    keys = ("x", "h", "c", "w_ih", "w_hh", "b_ih", "b_hh")
    h64, c64, g64 = lstmcell_step(*[d[k].double() for k in keys])
    h32, c32, g32 = lstmcell_step(*[d[k] for k in keys])
    err = dict(h=(h32.double() - h64).abs().max().item(), c=(c32.double() - c64).abs().max().item(),
               gates=(torch.cat(g32, 1).double() - torch.cat(g64, 1)).abs().max().item())
    return (h64, c64, torch.cat(g64, 1)), err


def lstmcell_bwd_point(dh_out, dh_carry, n_carry, gates, c, c_prev, dc_state):
    """Pointwise backward of one LSTM step.  gates [n, 4H] activated (i, f, g, o); rows >= n_carry take neither dh_carry nor the
    old dc_state; c_prev None = zeros.  Returns DG [n, 4H] (gradient of the gate pre-activations) and the new dc_state = dc * f."""
    n, H = c.shape
    i, f, g, o = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:3 * H], gates[:, 3 * H:]
    dh, dcn = dh_out.clone(), torch.zeros_like(c)
    if n_carry > 0:
        dh[:n_carry] += dh_carry[:n_carry]
        dcn[:n_carry] = dc_state[:n_carry]
    cp = torch.zeros_like(c) if c_prev is None else c_prev
    tc = torch.tanh(c)
    dc = dh * o * (1 - tc * tc) + dcn
    DG = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    return DG, dc * f


def bwd_point_f32_error(n, H, n_carry, with_c_prev):
    d = bwd_point_inputs(n, H)
    keys = ("dh_out", "dh_carry", "gates", "c", "c_prev", "dc_state")

    def run(cast):
        a = {k: cast(d[k]) for k in keys}
        return lstmcell_bwd_point(a["dh_out"], a["dh_carry"], n_carry, a["gates"], a["c"], a["c_prev"] if with_c_prev else None, a["dc_state"])
    dg64, dc64 = run(lambda t: t.double())
    dg32, dc32 = run(lambda t: t)
    return (dg64, dc64), dict(DG=(dg32.double() - dg64).abs().max().item(), dc_state=(dc32.double() - dc64).abs().max().item())


# ---------------------------------------------------------------------------------------------- conv-stack backward helpers

def maxpool2_bwd_first_max(x, dy):
    """Backward of the 2x2 / stride 2 max-pool, NHWC: the gradient goes to the FIRST maximum of each window in the scan order
    (0,0), (0,1), (1,0), (1,1); every other element of dx is zero.  An explicit loop."""
    x, dy = np.asarray(x), np.asarray(dy)
    N, Hin, Win, C = x.shape
    dx = np.zeros_like(x)
    for n in range(N):
        for ho in range(Hin // 2):
            for wo in range(Win // 2):
                for c in range(C):
                    best, bv = (0, 0), x[n, 2 * ho, 2 * wo, c]
                    for dh, dw in ((0, 1), (1, 0), (1, 1)):
                        v = x[n, 2 * ho + dh, 2 * wo + dw, c]
                        if v > bv:
                            best, bv = (dh, dw), v
                    dx[n, 2 * ho + best[0], 2 * wo + best[1], c] = dy[n, ho, wo, c]
    return torch.from_numpy(dx)


def pad_nhwc(inp, y, pad):
    """zero-bordered copy of inp [N,H,W,C]; with y the ReLU mask on the way: out = y > 0 ? inp : 0 (0.0 and -0.0 both mask)"""
    N, H, W, C = inp.shape
    out = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=inp.dtype)
    out[:, pad:pad + H, pad:pad + W] = inp if y is None else torch.where(y > 0, inp, torch.zeros_like(inp))
    return out


def bcast_add(out, v, scale):
    """out[b,p,c] + scale * v[b,c]"""
    return out + scale * v[:, None, :]


# ---------------------------------------------------------------------------------------------- row utilities

def batch_sizes(lengths):
    return [sum(1 for l in lengths if l > t) for t in range(int(lengths[0]))]


def pack_tokens(captions, lengths, col0):
    """time-major packed ids of captions[:, col0:] (lengths sorted decreasing): row (t, b) = captions[b][t + col0]"""
    return torch.cat([captions[:bs, t + col0] for t, bs in enumerate(batch_sizes(lengths))])


def collate(flat, offsets, order, Tmax):
    """out[r][t] = t < len(order[r]) ? flat[offsets[order[r]] + t] : 0"""
    out = torch.zeros(len(order), Tmax, dtype=flat.dtype)
    for r, src in enumerate(order):
        o0, o1 = int(offsets[src]), int(offsets[src + 1])
        out[r, :o1 - o0] = flat[o0:o1]
    return out


def scatter_rows_add_rowordered_f32(rows, ids, V):
    """table[v] = the float32 sum of rows[i] over the i with ids[i] == v, added one by one in ascending i starting from the first
    such row (the order `scatter_rows_kernel` documents); ids no row carries stay exactly zero."""
    r, idn = rows.numpy().astype(np.float32), ids.numpy()
    table = np.zeros((V, r.shape[1]), dtype=np.float32)
    seen = np.zeros(V, dtype=bool)
    for i in range(r.shape[0]):
        v = int(idn[i])
        table[v] = table[v] + r[i] if seen[v] else r[i]
        seen[v] = True
    return torch.from_numpy(table)


# ---------------------------------------------------------------------------------------------- the tolerance table

# The float32 restatement's max abs error against float64 at every case of the sweep, as test_attend_step_reference_host.py
# measured it (3 digits; torch 2.x CPU, 16 threads).  FROZEN: torch's float32 summation order depends on the host, so the GPU test
# reads its tolerance from here, not from the machine it happens to run on; the host test re-measures and compares.
# ("att", shape, kind, extra): ATT_OUTPUTS order; ("lstm", shape): h, c, gates; ("bwd_point", shape, n_carry, c_prev): DG, dc_state
F32_ERR = {
    ("att", (1, 1, 4), "plain", False): (0, 0, 0, 0, 0, 0, 0, 1.02e-07),
    ("att", (3, 3, 4), "plain", False): (1.4e-08, 1.27e-08, 6.27e-10, 7.74e-10, 5.14e-09, 1.29e-08, 1.43e-09, 1.66e-08),
    ("att", (2, 5, 36), "plain", False): (1.8e-08, 2.29e-08, 3.86e-09, 6.61e-09, 4.7e-08, 1.31e-08, 4.1e-09, 1.47e-08),
    ("att", (7, 9, 68), "plain", False): (2.55e-08, 1.62e-08, 6.22e-09, 1.47e-08, 1.43e-07, 7.3e-09, 6.45e-09, 1.02e-08),
    ("att", (1, 197, 260), "plain", False): (2.8e-09, 4.28e-10, 6.45e-11, 4.44e-10, 2.19e-09, 4.78e-11, 2.06e-09, 3.24e-09),
    ("att", (600, 8, 64), "plain", False): (4.44e-08, 3.68e-08, 1.89e-08, 4.43e-08, 1.74e-06, 1.98e-08, 1.89e-08, 1.96e-08),
    ("att", (2, 1030, 8), "plain", False): (1.58e-10, 5.01e-11, 1.92e-13, 7.76e-12, 3.24e-11, 4.51e-13, 2.98e-09, 3.7e-09),
    ("att", (5, 196, 512), "plain", False): (2.26e-08, 5.92e-10, 4.51e-10, 6.45e-10, 1.25e-08, 4.04e-10, 3.55e-09, 3.62e-09),
    ("att", (2, 5, 36), "plain", True): (1.8e-08, 2.29e-08, 4.28e-09, 9.87e-09, 3.89e-08, 1.31e-08, 6.09e-09, 1.47e-08),
    ("att", (7, 9, 68), "plain", True): (2.55e-08, 1.62e-08, 1.43e-08, 3.51e-08, 2.19e-07, 7.3e-09, 1.46e-08, 1.02e-08),
    ("att", (1, 197, 260), "plain", True): (2.8e-09, 4.28e-10, 6.72e-10, 1.64e-09, 1.5e-08, 4.78e-11, 2.57e-09, 3.24e-09),
    ("att", (2, 5, 36), "zero_w", False): (2.98e-09, 2.03e-08, 0, 0, 5.45e-08, 4.47e-09, 0, 6.67e-09),
    ("att", (2, 5, 36), "large", False): (2.81e-11, 1.19e-08, 3.23e-10, 3.23e-10, 1.34e-11, 2.38e-08, 3.23e-10, 2.51e-08),
    ("att", (2, 5, 36), "dominant", False): (7.65e-24, 1.19e-08, 4.2e-23, 6.58e-23, 1.77e-23, 2.38e-08, 6.94e-18, 2.51e-08),
    ("att", (5, 196, 512), "zero_w", False): (1.05e-10, 4.86e-10, 0, 0, 1.04e-08, 6.35e-12, 0, 3.58e-09),
    ("att", (5, 196, 512), "large", False): (3.45e-07, 5.16e-09, 2.39e-07, 1.41e-07, 7.2e-08, 5.09e-09, 2.39e-07, 5.86e-09),
    ("att", (5, 196, 512), "dominant", False): (4.66e-15, 6.08e-10, 4.27e-19, 4.27e-19, 1.59e-16, 9.12e-10, 3.47e-18, 2.24e-09),
    ("lstm", (1, 4, 4)): (1.76e-08, 1.67e-07, 6.23e-08),
    ("lstm", (5, 20, 20)): (6.09e-08, 1.72e-07, 1.61e-07),
    ("lstm", (65, 36, 48)): (1.01e-07, 2.99e-07, 2.75e-07),
    ("lstm", (64, 64, 64)): (1.16e-07, 2.5e-07, 3.66e-07),
    ("lstm", (3, 1028, 8)): (2.28e-07, 6.23e-07, 7.34e-07),
    ("bwd_point", (1, 4), 0, False): (4.1e-08, 2.83e-08),
    ("bwd_point", (1, 4), 0, True): (4.1e-08, 2.83e-08),
    ("bwd_point", (1, 4), 1, False): (5.42e-08, 3.93e-08),
    ("bwd_point", (1, 4), 1, True): (5.42e-08, 3.93e-08),
    ("bwd_point", (5, 20), 0, False): (4.19e-08, 5.41e-08),
    ("bwd_point", (5, 20), 0, True): (4.19e-08, 5.41e-08),
    ("bwd_point", (5, 20), 2, False): (7.55e-08, 8.03e-08),
    ("bwd_point", (5, 20), 2, True): (1.39e-07, 8.03e-08),
    ("bwd_point", (5, 20), 5, False): (7.55e-08, 8.03e-08),
    ("bwd_point", (5, 20), 5, True): (1.39e-07, 8.03e-08),
    ("bwd_point", (64, 64), 0, False): (1.21e-07, 1.09e-07),
    ("bwd_point", (64, 64), 0, True): (1.21e-07, 1.09e-07),
    ("bwd_point", (64, 64), 32, False): (1.69e-07, 1.9e-07),
    ("bwd_point", (64, 64), 32, True): (1.71e-07, 1.9e-07),
    ("bwd_point", (64, 64), 64, False): (1.92e-07, 2.4e-07),
    ("bwd_point", (64, 64), 64, True): (1.92e-07, 2.4e-07),
    ("bwd_point", (300, 12), 0, False): (1.02e-07, 1.4e-07),
    ("bwd_point", (300, 12), 0, True): (1.02e-07, 1.4e-07),
    ("bwd_point", (300, 12), 150, False): (1.96e-07, 2.11e-07),
    ("bwd_point", (300, 12), 150, True): (2.06e-07, 2.11e-07),
    ("bwd_point", (300, 12), 300, False): (2.19e-07, 2.37e-07),
    ("bwd_point", (300, 12), 300, True): (2.19e-07, 2.37e-07),
}


def f32_err(*key):
    """the frozen errors of one case as a dict by output name"""
    names = {"att": ATT_OUTPUTS, "lstm": ("h", "c", "gates"), "bwd_point": ("DG", "dc_state")}[key[0]]
    return dict(zip(names, F32_ERR[key]))
