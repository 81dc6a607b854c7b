"""Plain CPU reference of token-level unlikelihood training (`sat_ce_rows_ul`, `sat_vocab_ce_fwd_bf16_ul`; the arithmetic is at their
declaration in include/sat_hip.h), a helper module like label_smoothing_reference.py: no GPU, no test in it.

`ul_autograd` is THE reference: the fairseq formulation (candidate_penalty_cross_entropy; Welleck et al. 2019, arXiv:1908.04319) in
float64 through torch autograd -- log_softmax, a 0/1 negative mask built by scatter from each row's earlier ground-truth targets with
the row's own target taken out, -log(clamp(1 - exp(lp), min=1e-5)), a sum.  `ul_rows` is the closed form of the same thing in the
dtype it is given: float64 to validate it against autograd (tests/test_unlikelihood_host.py), float32 as the restatement whose error
against the float64 reference sets the tolerance of the GPU test at a case (F32_ERR below, frozen from the host test's measurement;
tests/test_gpu_unlikelihood.py allows elementwise_reference.TOL_FACTOR x that value).

The cases of the GPU sweep live here, so that the host test can assert on the float64 reference what the GPU test relies on: no
candidate near the clamp (q in (5e-6, 2e-5)), amplification max w_c <= 10 in the tolerance sweeps, and q_c < 1e-6 for the
dedicated clamp rows."""
import numpy as np
import torch
import torch.nn.functional as F

import elementwise_reference as R

QMIN = 1e-5
UL_V = [3, 5, 255, 1003, 1024, 12288, 12289, 12292]
UL_SETTINGS = [(1.0, 0.0), (0.5, 0.1)]                        # (alpha, label smoothing)
UL_LENGTHS = [12, 12, 11, 9, 9, 7, 4, 3]                      # the pack of the sweep: 67 rows
UL_PACKS = {"one": [1], "ones": [1, 1, 1], "two": [2, 1], "full": [64, 64, 3]}
UL_PACK_V = {"one": [5, 1003], "ones": [5, 1003], "two": [5, 1003], "full": [255, 12289]}
UL_CLAMP_V = [1003, 12292]
UL_KINDS = ["random", "equal", "shifted", "low", "random"]
UL_OUTPUTS = ("row_loss", "row_nll", "row_ul", "grad", "loss", "nll", "ul")


def batch_sizes(lengths):
    return [sum(1 for l in lengths if l > t) for t in range(lengths[0])]


def prefix(lengths):
    p = [0]
    for n in batch_sizes(lengths):
        p.append(p[-1] + n)
    return p


def positions(lengths):
    """[(t, b)] of every packed row, time-major"""
    return [(t, b) for t, n in enumerate(batch_sizes(lengths)) for b in range(n)]


def candidate_sets(targets, lengths, V):
    """per row: the clamped targets of the earlier steps of its sequence in order of first occurrence, each once, without the row's own"""
    t = targets.clamp(0, V - 1).tolist()
    pre = prefix(lengths)
    sets = []
    for n, (step, b) in enumerate(positions(lengths)):
        seen = []
        for s in range(step):
            c = t[pre[s] + b]
            if c != t[n] and c not in seen:
                seen.append(c)
        sets.append(seen)
    return sets


def negative_mask(targets, lengths, V, dtype):
    """fairseq's negative_targets: zeros [N, V] with 1 scattered at every earlier target of the row's sequence, the row's own target
    zeroed afterwards"""
    N = targets.numel()
    t = targets.clamp(0, V - 1)
    pre = prefix(lengths)
    mask = torch.zeros(N, V, dtype=dtype)
    for n, (step, b) in enumerate(positions(lengths)):
        if step:
            mask[n].scatter_(0, torch.stack([t[pre[s] + b] for s in range(step)]), 1.0)
    mask.scatter_(1, t[:, None], 0.0)
    return mask


def ul_autograd(logits, targets, lengths, eps, alpha, scale):
    """the reference (module docstring), float64: every output of the kernels by name"""
    assert logits.dtype == torch.float64
    V = logits.shape[1]
    e, a, s = R.f32v(eps), R.f32v(alpha), R.f32v(scale)
    t = targets.clamp(0, V - 1)
    x = logits.clone().requires_grad_(True)
    lp = F.log_softmax(x, 1)
    row_nll = F.nll_loss(lp, t, reduction="none")
    row_ce = F.cross_entropy(x, t, reduction="none", label_smoothing=e)
    mask = negative_mask(targets, lengths, V, torch.float64)
    row_ul = (-torch.log(torch.clamp(1.0 - lp.exp(), min=QMIN)) * mask).sum(1)
    row_loss = row_ce + a * row_ul
    (row_loss.sum() * s).backward()
    return dict(row_loss=row_loss.detach(), row_nll=row_nll.detach(), row_ul=row_ul.detach(), grad=x.grad,
                loss=row_loss.detach().sum() * s, nll=row_nll.detach().sum() * s, ul=row_ul.detach().sum() * s)


def ul_rows(logits, targets, lengths, eps, alpha, scale):
    """the closed form, in the dtype of `logits`: with p = softmax(x), q = 1 - p over the candidate set C of the row
    row_ul = sum_C -log(max(q, 1e-5)); w = p / q where q > 1e-5 else 0; W = sum_C w;
    row_loss = (1 - eps) nll + eps (log s - mean(x - m)) + alpha row_ul;
    grad = (p (1 - alpha W) - (1 - eps) onehot - eps / V + alpha w [v in C]) * scale"""
    V = logits.shape[1]
    e, a, s = R.f32v(eps), R.f32v(alpha), R.f32v(scale)
    t = targets.clamp(0, V - 1)
    m = logits.max(1).values
    z = logits - m[:, None]
    logs = torch.log(torch.exp(z).sum(1))
    lse = m + logs
    row_nll = lse - logits.gather(1, t[:, None])[:, 0]
    row_ce = (1 - e) * row_nll + e * (logs - z.sum(1) / V)
    p = torch.exp(logits - lse[:, None])
    q = 1 - p
    mask = negative_mask(targets, lengths, V, logits.dtype)
    row_ul = (-torch.log(torch.clamp(q, min=QMIN)) * mask).sum(1)
    w = torch.where(q > QMIN, p / q, torch.zeros_like(p)) * mask
    W = w.sum(1)
    onehot = torch.zeros_like(logits).scatter_(1, t[:, None], 1.0)
    grad = (p * (1 - a * W)[:, None] - ((1 - e) * onehot + e / V) + a * w) * s
    row_loss = row_ce + a * row_ul
    return dict(row_loss=row_loss, row_nll=row_nll, row_ul=row_ul, grad=grad, loss=row_loss.sum() * s, nll=row_nll.sum() * s,
                ul=row_ul.sum() * s, w=w, q=q, mask=mask)


def ul_f32_error(logits, targets, lengths, eps, alpha, scale):
    """(float64 reference, {output: error of the float32 restatement}).  Arrays: the max abs error.  The three scalar sums: the larger
    of the observed error and the spread of a float32 sum of these rows,
        scale * (||row errors||_2 + sqrt(N) * ulp32(S) / 2) + ulp32(scale * S) / 2,      S = the float64 sum of the rows.
    The observed error of a sum is ONE draw: N row errors of either sign and N - 1 roundings of partial sums up to S, each up to half
    an ulp of S, plus the rounding of the product, add up as a random walk and can land arbitrarily close to 0 (2e-10 on a sum of
    3e-3 at V = 1024; 1.7e-7 on a loss of 13.05 whose own ulp is 9.5e-7).  Another summation order -- the kernels sum in a tree --
    draws again, so the spread is the restatement's error of the sum, not the draw.  At these cases 8 x the figure is 7e-7 to 5e-6 of
    the sum: at least a factor 2 below the 1e-5 relative tolerance the existing tests give a summed loss."""
    r64 = ul_autograd(logits.double(), targets, lengths, eps, alpha, scale)
    r32 = ul_rows(logits, targets, lengths, eps, alpha, scale)
    err = {k: R.max_err(r32[k], r64[k]) for k in UL_OUTPUTS}
    s, N = R.f32v(scale), logits.shape[0]
    for total, rows in (("loss", "row_loss"), ("nll", "row_nll"), ("ul", "row_ul")):
        S = float(r64[rows].sum())
        spread = s * (float((r32[rows].double() - r64[rows]).norm()) + N ** 0.5 * ulp32(S) / 2) + ulp32(s * S) / 2
        err[total] = max(err[total], spread) if S != 0 else err[total]
    return r64, err


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ---------------------------------------------------------------------------------------------- the cases of the GPU sweep

def edge_ids(V):
    """raw target ids the sweep draws from: column 0, V - 1, the first element of the scalar tail, a 16-byte chunk boundary (4) and
    its neighbour (3), -1 and V (clamped: they collide with 0 and V - 1), the middle; for long rows 4 + 2048 and 4 + 4096 as well"""
    ids = [0, V - 1, min(4 * (V // 4), V - 1), min(4, V - 1), min(3, V - 1), -1, V, V // 2]
    if V > 4100:
        ids += [2052, 4100]
    return ids


def shape_rows(logits, offset=0):
    """row n is UL_KINDS[(n + offset) % 5]: random (unit scale), equal, shifted by +60, low (-80), random"""
    for n in range(logits.shape[0]):
        kind = UL_KINDS[(n + offset) % 5]
        if kind == "equal":
            logits[n] = 1.25
        elif kind == "shifted":
            logits[n] += 60.0
        elif kind == "low":
            logits[n] -= 80.0
    return logits


def ul_inputs(V):
    """the sweep at one V: (logits [67, V], raw targets [67], UL_LENGTHS)"""
    g = R.gen(7, V)
    N = sum(UL_LENGTHS)
    ids = torch.tensor(edge_ids(V), dtype=torch.int64)
    targets = ids[torch.randint(0, len(ids), (N,), generator=g)]
    return shape_rows(torch.randn(N, V, generator=g)), targets, UL_LENGTHS


def ul_pack_inputs(name, V):
    """the other packs.  "full" = [64, 64, 3]: sequence 0 has all-distinct targets (63 candidates at its last step: every lane of the
    wave), sequence 1 one repeated id with another one at the last step (a set of one; before that the only candidate is the target
    itself: an empty set), sequence 2 the ids 5, 5, 6"""
    lengths = UL_PACKS[name]
    g = R.gen(8, V, len(lengths), lengths[0])
    N = sum(lengths)
    if name == "full":
        targets = torch.empty(N, dtype=torch.int64)
        pre = prefix(lengths)
        for n, (t, b) in enumerate(positions(lengths)):
            targets[n] = ((3 * t + 1) % V, 9 if t == 63 else 7, (5, 5, 6)[min(t, 2)])[b]
        assert len(set(targets[[pre[t] for t in range(64)]].tolist())) == 64
    else:
        ids = torch.tensor(edge_ids(V), dtype=torch.int64)
        targets = ids[torch.randint(0, len(ids), (N,), generator=g)]
    return shape_rows(torch.randn(N, V, generator=g), offset=1 if name == "full" else 0), targets, lengths


def ul_clamp_inputs(V):
    """the clamp rows: pack [4, 4, 4]; from step 1 on one candidate of the row (the target of step 0 of its sequence) has a logit 40
    above unit-scale noise: q_c < 1e-6, the term is -log(1e-5) and the weight 0"""
    lengths = [4, 4, 4]
    g = R.gen(9, V)
    targets = torch.tensor([0, V - 1, 4, 7, 8, 9, 7, 0, 11, 12, 13, 4], dtype=torch.int64).clamp(max=V - 1)
    logits = torch.randn(12, V, generator=g)
    for n, (t, b) in enumerate(positions(lengths)):
        if t:
            logits[n, targets[b]] = 40.0
    return logits, targets, lengths


def all_cases():
    """{key: (logits, targets, lengths, eps, alpha)} of every case with a frozen error"""
    out = {}
    for V in UL_V:
        for alpha, eps in UL_SETTINGS:
            out[("ul", V, alpha, eps)] = ul_inputs(V) + (eps, alpha)
    for name, Vs in UL_PACK_V.items():
        for V in Vs:
            out[("ul_pack", name, V)] = ul_pack_inputs(name, V) + (0.1, 1.0)
    for V in UL_CLAMP_V:
        out[("ul_clamp", V)] = ul_clamp_inputs(V) + (0.0, 1.0)
    return out


def measure_all():
    """{key: tuple of max abs errors of the float32 restatement against the float64 reference, in UL_OUTPUTS' order}"""
    return {key: tuple(ul_f32_error(lg, tg, ln, eps, alpha, R.CE_INV)[1].values()) for key, (lg, tg, ln, eps, alpha) in all_cases().items()}


# The float32 restatement's max abs error against float64 at every case, as test_unlikelihood_host.py measured it (`measure_all()`,
# 3 digits; torch 2.x CPU).  FROZEN, as label_smoothing_reference.F32_ERR is: the GPU test reads its tolerance from here.
F32_ERR = {
    ('ul', 3, 1.0, 0.0): (2e-05, 3.63e-06, 2.36e-05, 2.77e-07, 1.2e-06, 8.66e-07, 8.89e-07),
    ('ul', 3, 0.5, 0.1): (8.66e-06, 3.63e-06, 2.36e-05, 1.35e-07, 9.54e-07, 8.66e-07, 8.89e-07),
    ('ul', 5, 1.0, 0.0): (3.19e-06, 3.8e-06, 4.33e-06, 4.54e-08, 1.51e-06, 9.52e-07, 3.03e-07),
    ('ul', 5, 0.5, 0.1): (3.02e-06, 3.8e-06, 4.33e-06, 3.96e-08, 1.51e-06, 9.52e-07, 3.03e-07),
    ('ul', 255, 1.0, 0.0): (3.76e-06, 3.84e-06, 1.59e-07, 6.52e-09, 2.98e-06, 2.98e-06, 1.1e-08),
    ('ul', 255, 0.5, 0.1): (3.54e-06, 3.84e-06, 1.59e-07, 6.28e-09, 2.95e-06, 2.98e-06, 1.1e-08),
    ('ul', 1003, 1.0, 0.0): (4.13e-06, 4.04e-06, 7.59e-08, 3.24e-09, 3.23e-06, 3.23e-06, 6.31e-09),
    ('ul', 1003, 0.5, 0.1): (3.51e-06, 4.04e-06, 7.59e-08, 3.12e-09, 3.21e-06, 3.23e-06, 6.31e-09),
    ('ul', 1024, 1.0, 0.0): (4e-06, 4e-06, 6.96e-08, 1.52e-09, 3.23e-06, 3.23e-06, 5.14e-09),
    ('ul', 1024, 0.5, 0.1): (4.09e-06, 4e-06, 6.96e-08, 2.27e-09, 3.23e-06, 3.23e-06, 5.14e-09),
    ('ul', 12288, 1.0, 0.0): (3.8e-06, 3.83e-06, 9.94e-08, 1.23e-09, 5.69e-06, 5.69e-06, 8.71e-09),
    ('ul', 12288, 0.5, 0.1): (3.56e-06, 3.83e-06, 9.94e-08, 1.39e-09, 5.68e-06, 5.69e-06, 8.71e-09),
    ('ul', 12289, 1.0, 0.0): (3.9e-06, 3.91e-06, 7.11e-08, 1.28e-09, 5.73e-06, 5.72e-06, 1.34e-08),
    ('ul', 12289, 0.5, 0.1): (3.9e-06, 3.91e-06, 7.11e-08, 1.22e-09, 5.72e-06, 5.72e-06, 1.34e-08),
    ('ul', 12292, 1.0, 0.0): (3.71e-06, 3.81e-06, 7.65e-08, 1.27e-09, 5.72e-06, 5.72e-06, 1.1e-08),
    ('ul', 12292, 0.5, 0.1): (3.83e-06, 3.81e-06, 7.65e-08, 2.14e-09, 5.72e-06, 5.72e-06, 1.1e-08),
    ('ul_pack', 'one', 5): (1.07e-07, 6.44e-08, 0, 1.52e-09, 4.27e-09, 3.41e-09, 0),
    ('ul_pack', 'one', 1003): (3.19e-07, 5.74e-08, 0, 1.65e-10, 1.86e-08, 1.34e-08, 0),
    ('ul_pack', 'ones', 5): (1.46e-06, 1.57e-06, 0, 1.05e-08, 4.13e-08, 4.34e-08, 0),
    ('ul_pack', 'ones', 1003): (2.04e-06, 2.08e-06, 0, 2.11e-09, 9.02e-08, 9.1e-08, 0),
    ('ul_pack', 'two', 5): (1.34e-06, 1.8e-06, 2.9e-07, 1.25e-08, 4.29e-08, 5.18e-08, 6.18e-09),
    ('ul_pack', 'two', 1003): (2.51e-06, 2.4e-06, 2.53e-08, 7.68e-10, 9.93e-08, 9.73e-08, 5.09e-10),
    ('ul_pack', 'full', 255): (3.46e-06, 3.88e-06, 9.12e-07, 6.18e-09, 7.77e-06, 7.82e-06, 1.01e-07),
    ('ul_pack', 'full', 12289): (3.61e-06, 4.03e-06, 8.08e-07, 1.58e-09, 1.52e-05, 1.52e-05, 1.13e-07),
    ('ul_clamp', 1003): (2.46e-06, 1.85e-06, 3.17e-07, 9.7e-10, 1.61e-06, 1.36e-06, 3.42e-07),
    ('ul_clamp', 12292): (2.11e-06, 1.18e-06, 3.17e-07, 9.75e-10, 1.62e-06, 1.34e-06, 3.42e-07),
}


def f32_err(*key):
    """the frozen errors of one case as a dict by output name"""
    return dict(zip(UL_OUTPUTS, F32_ERR[key]))
