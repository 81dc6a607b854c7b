"""Plain CPU reference of the label-smoothed cross entropy (`sat_ce_rows_ls`, `sat_vocab_ce_fwd_bf16_ls`; formulas at their
declaration in include/sat_hip.h), a helper module like elementwise_reference.py: no GPU, no test in it.

`ls_rows` runs in the dtype it is given: float64 is the reference, float32 the restatement whose error against float64 sets the
second tolerance of the GPU test at a case (tests/test_label_smoothing_host.py measures it, F32_ERR keeps it,
tests/test_gpu_label_smoothing.py allows elementwise_reference.TOL_FACTOR x that value).  The smoothing term is formed from values
centred on the row maximum, log s - mean(x - m), as the kernels form it.  The inputs are elementwise_reference's: `ce_inputs(V)`
for the edge sweep, `ce_loss_inputs(N)` for the sums.  eps and the scale cross the C ABI as `float` and enter as those values."""
import torch

import elementwise_reference as R

LS_EPS = (0.1, 0.9)
LS_LOSS_EPS = 0.1
LS_OUTPUTS = ("row_loss", "row_nll", "grad", "loss", "nll")


def ls_rows(logits, targets, eps, scale):
    """row_nll = lse - x[t]; row_loss = (1 - eps) row_nll + eps (log s - mean(x - m)); grad = (softmax - (1 - eps) onehot - eps / V)
    * scale; loss = scale * sum(row_loss); nll = scale * sum(row_nll).  Targets are clamped into [0, V - 1] as the kernels clamp."""
    V = logits.shape[1]
    e, s = R.f32v(eps), R.f32v(scale)
    t = targets.clamp(0, V - 1)
    m = logits.max(1).values
    z = logits - m[:, None]
    logs = torch.log(torch.exp(z).sum(1))
    lse = m + logs
    row_nll = lse - logits.gather(1, t[:, None])[:, 0]
    row_loss = (1 - e) * row_nll + e * (logs - z.sum(1) / V)
    onehot = torch.zeros_like(logits).scatter_(1, t[:, None], 1.0)
    grad = (torch.exp(logits - lse[:, None]) - ((1 - e) * onehot + e / V)) * s
    return dict(row_loss=row_loss, row_nll=row_nll, grad=grad, loss=row_loss.sum() * s, nll=row_nll.sum() * s)


def ls_f32_error(logits, targets, eps, scale):
    r64 = ls_rows(logits.double(), targets, eps, scale)
    r32 = ls_rows(logits, targets, eps, scale)
    return r64, {k: R.max_err(r32[k], r64[k]) for k in LS_OUTPUTS}


def measure_all():
    """{key: tuple of max abs errors of the float32 restatement against float64, in LS_OUTPUTS' order}: what F32_ERR freezes"""
    out = {}
    for V in R.CE_V:
        logits, targets, _ = R.ce_inputs(V)
        for eps in LS_EPS:
            out[("ls", V, eps)] = tuple(ls_f32_error(logits, targets, eps, R.CE_INV)[1].values())
    for N in R.CE_LOSS_N:
        out[("ls_loss", N, LS_LOSS_EPS)] = tuple(ls_f32_error(*R.ce_loss_inputs(N), LS_LOSS_EPS, R.CE_INV)[1].values())
    return out


# The float32 restatement's max abs error against float64 at every case, as test_label_smoothing_host.py measured it
# (`measure_all()`, 3 digits; torch 2.x CPU).  FROZEN, as elementwise_reference.F32_ERR is: the GPU test reads its tolerance from here.
F32_ERR = {
    ('ls', 1, 0.1): (0, 0, 0, 0, 0),
    ('ls', 1, 0.9): (0, 0, 0, 0, 0),
    ('ls', 3, 0.1): (3.51e-06, 3.8e-06, 6.03e-08, 2.58e-07, 3.68e-07),
    ('ls', 3, 0.9): (1.99e-06, 3.8e-06, 6.01e-08, 1.64e-07, 3.68e-07),
    ('ls', 4, 0.1): (3.35e-06, 3.77e-06, 4.73e-08, 7.89e-08, 3.26e-07),
    ('ls', 4, 0.9): (1.43e-06, 3.77e-06, 4.62e-08, 5.11e-07, 3.26e-07),
    ('ls', 5, 0.1): (5.66e-06, 3.56e-06, 4.61e-08, 1.41e-07, 3.91e-07),
    ('ls', 5, 0.9): (2.8e-06, 3.56e-06, 4.48e-08, 5.26e-07, 3.91e-07),
    ('ls', 255, 0.1): (4.25e-06, 3.51e-06, 3.81e-08, 8.02e-07, 1.29e-07),
    ('ls', 255, 0.9): (2.03e-06, 3.51e-06, 3.81e-08, 6.34e-07, 1.29e-07),
    ('ls', 1003, 0.1): (3.66e-06, 3.7e-06, 1.8e-08, 3.1e-07, 5.25e-07),
    ('ls', 1003, 0.9): (3.48e-06, 3.7e-06, 1.76e-08, 4.58e-07, 5.25e-07),
    ('ls', 1024, 0.1): (3.21e-06, 3.08e-06, 4.13e-08, 3.11e-07, 4.23e-08),
    ('ls', 1024, 0.9): (4.23e-06, 3.08e-06, 4.21e-08, 2.83e-07, 4.23e-08),
    ('ls', 12288, 0.1): (4.09e-06, 3.95e-06, 1.28e-08, 3.36e-08, 7.86e-07),
    ('ls', 12288, 0.9): (2.45e-06, 3.95e-06, 1.27e-08, 1.04e-06, 7.86e-07),
    ('ls', 12289, 0.1): (6.06e-06, 3.94e-06, 2.13e-08, 5.1e-07, 4e-07),
    ('ls', 12289, 0.9): (4.45e-06, 3.94e-06, 2.13e-08, 1.58e-07, 4e-07),
    ('ls', 12292, 0.1): (4.49e-06, 3.69e-06, 3.41e-08, 6.42e-07, 1.12e-07),
    ('ls', 12292, 0.9): (3.87e-06, 3.69e-06, 3.38e-08, 1.06e-06, 1.12e-07),
    ('ls_loss', 1, 0.1): (5.55e-07, 4.19e-07, 3.34e-10, 1.23e-08, 1.97e-10),
    ('ls_loss', 255, 0.1): (1.91e-06, 1.59e-06, 8.92e-09, 3.79e-06, 4.64e-06),
    ('ls_loss', 257, 0.1): (2.37e-06, 1.29e-06, 8.35e-09, 6.79e-07, 3.22e-06),
}


def f32_err(*key):
    """the frozen errors of one case as a dict by output name"""
    return dict(zip(LS_OUTPUTS, F32_ERR[key]))
