"""numpy yardstick of the averaged weights (csrc/sat_optim.hip: sat_ema_update): one step of the rule, bit for bit.

The kernel's arithmetic is  w = f32(1 - f64(f32(decay)));  d = f32(p - e);  e' = fma(w, d, e), i.e. the exact value e + w d rounded
ONCE to float32.  Here: d in float32 (numpy's subtraction rounds to nearest even, as the kernel's does), then e + w d in float64.
The product w d is exact there (24 x 24 significand bits); the SUM rounds to float64 before it is rounded to float32 -- a double
rounding.  It can differ from the single rounding only when the float64 value lands on, or within its own rounding error of, the
midpoint between two float32 neighbours.  So: the expected result is the float32 rounding of the float64 value, and where that
value lies within a relative 2^-50 of such a midpoint the other neighbour passes as well.  That is the only slack, and it covers the
reference's double rounding, not the kernel."""
import numpy as np

F32, F64 = np.float32, np.float64
MIDPOINT_RTOL = 2.0 ** -50


def weight(decay):
    """the kernel's w: the decay as the C ABI receives it (a float32), 1 - decay in float64, rounded to float32"""
    return F32(1.0 - F64(F32(decay)))


def ema_decay_at(decay, t, warmup=False):
    """sat.ema_decay_at restated: python floats; t = the optimizer's step count after this step's increment"""
    return min(decay, (1 + t) / (10 + t)) if warmup else decay


def ema_step(e, p, decay):
    """(expected, other): float32 arrays; `other` equals `expected` except where the float64 value sits on a float32 midpoint"""
    e, p = np.asarray(e, dtype=F32), np.asarray(p, dtype=F32)
    w = weight(decay)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (p - e).astype(F32)
        v = e.astype(F64) + F64(w) * d.astype(F64)
        r = v.astype(F32)
        r64 = r.astype(F64)
        away = np.where(r64 > v, F32(-np.inf), F32(np.inf))
        other = np.nextafter(r, away).astype(F32)
        mid = 0.5 * (r64 + other.astype(F64))                       # exact in float64
        near = np.isfinite(mid) & (r64 != v) & (np.abs(v - mid) <= MIDPOINT_RTOL * np.abs(mid))
    return r, np.where(near, other, r)


def matches(got, expected, other):
    """elementwise: the bits of `got` are those of `expected` or of `other`"""
    g = np.asarray(got, dtype=F32).view(np.uint32)
    return (g == expected.view(np.uint32)) | (g == other.view(np.uint32))


def ema_step_f64(e, p, decay):
    """the rule in float64 with the decay as given (no float32 anywhere): what torch's swa_utils computes"""
    return e + (1.0 - decay) * (p - e)


SWEEP_N = (1, 3, 4, 5, 1023, 1024, 1025, 786437)         # 786437 = 768 * 256 * 4 + 5: a second grid-stride trip, and a tail
SWEEP_DECAY = (0.5, 0.999, 0.9999)


def sweep_inputs(n, decay):
    """(e, p) float32 [n].  decay 0.9999: magnitudes spread log-uniformly over 1e-30 .. 1e30, both signs; the others: unit scale"""
    g = np.random.default_rng(1000 + n % 997 + int(decay * 10000))
    if decay == 0.9999:
        e = (g.choice([-1.0, 1.0], n) * 10.0 ** g.uniform(-30, 30, n)).astype(F32)
        p = (g.choice([-1.0, 1.0], n) * 10.0 ** g.uniform(-30, 30, n)).astype(F32)
        k = n // 2
        p[:k] = (e[:k] * (1 + g.uniform(-1e-3, 1e-3, k))).astype(F32)      # half of them close to their average, as in training
        return e, p
    e = g.standard_normal(n).astype(F32)
    return e, (e + 0.01 * g.standard_normal(n)).astype(F32)
