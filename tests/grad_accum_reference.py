"""Plain numpy reference of sat_grad_accumulate (csrc/sat_optim.hip): one finished backward folded into the accumulated twin of the
flat gradient buffer.  A helper module like ema_reference.py: no GPU, no test in it.

Buffers hold n + 2 float32: n gradients, the loss slot, the fault word.  Elements 0 .. n: acc = weight * g on the first fold (the old
acc is not read), acc = fma(weight, g, acc) afterwards -- ONE rounding each.  Element n + 1: 1.0 when a fault word seen so far
(the old one only when the fold is not the first) is non-zero, 0.0 otherwise.

The fma is formed in float64: weight * g is exact there (24 x 24 bits), the sum is rounded once to float64 and once more to float32.
Double rounding can differ from the single rounding of a hardware fma only where the float64 sum lies within 2^-53 relative of a
float32 midpoint; `fold` returns the second candidate for that case (`matches`), as ema_reference does.  With weight == 1 (and with
any power of two that does not underflow) the float64 sum of two float32 values of comparable exponent is exact, and numpy's own
float32 `a + g` is the yardstick: the tests named "bitwise" compare against that, without the second candidate."""
import numpy as np

BLOCK, VEC, GRID_CAP = 256, 4, 768          # sat_optim.hip: OPT_BLOCK threads, 16-byte accesses (4 floats), OPT_GRID_CAP workgroups
SPAN = BLOCK * VEC                           # elements one workgroup covers in one trip of the grid-stride loop
SWEEP = GRID_CAP * SPAN                      # elements one trip of the whole grid covers
# the kernel covers n + 1 elements (gradients and loss slot) in 16-byte chunks: one workgroup's span is full at n + 1 == SPAN, and
# the second workgroup gets its first chunk at n + 1 == SPAN + 4; the last size wraps the grid-stride loop and leaves a tail
SIZES = [1, 3, 4, 5, SPAN - 2, SPAN - 1, SPAN, SPAN + 1, SPAN + 3, SWEEP + SPAN + 5]


def grid(n):
    """workgroups of a launch over n gradients"""
    return min(GRID_CAP, max(1, -(-((n + 1) // VEC) // BLOCK)))


def gen(*seed):
    return np.random.default_rng([int(s) for s in seed])


def inputs(n, k, seed=0):
    """k buffers of n + 2 float32: normal gradients of mixed magnitude, a loss of a few units, a zero fault word"""
    r = gen(31, n, seed)
    out = []
    for _ in range(k):
        g = (r.standard_normal(n + 2) * 10.0 ** r.uniform(-6, 2, n + 2)).astype(np.float32)
        g[n] = np.float32(r.uniform(1.0, 6.0))
        g[n + 1] = 0.0
        out.append(g)
    return out


def fault(first, acc_word, g_word):
    return np.float32(1.0 if ((not first and acc_word != 0) or g_word != 0) else 0.0)


def fold(acc, g, weight, first):
    """(expected, other): the accumulated buffer after one fold and the second candidate at float32 midpoints (equal elsewhere)"""
    n = len(g) - 2
    w = np.float64(np.float32(weight))
    with np.errstate(all="ignore"):
        exact = w * g[:n + 1].astype(np.float64)
        if not first:
            exact = exact + acc[:n + 1].astype(np.float64)
        out = exact.astype(np.float32)
        # the float32 neighbour on the other side of the float64 value, taken only where that value sits on the midpoint
        toward = np.where(exact > out.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        nb = np.nextafter(out, toward)
        mid = (out.astype(np.float64) + nb.astype(np.float64)) * 0.5
        other = np.where(np.isfinite(exact) & (exact != out.astype(np.float64)) & (mid == exact), nb, out).astype(np.float32)
    word = fault(first, None if first else acc[n + 1], g[n + 1])
    return np.append(out, word).astype(np.float32), np.append(other, word).astype(np.float32)


def matches(got, expected, other):
    g, e, o = (np.asarray(x, dtype=np.float32).view(np.uint32) for x in (got, expected, other))
    return (g == e) | (g == o)


def sum_f64(gs, weights):
    """(sum_k w_k g_k, sum_k |w_k g_k|) over elements 0 .. n in float64, the weights as the float32 values that cross the ABI"""
    n = len(gs[0]) - 2
    terms = [np.float64(np.float32(w)) * g[:n + 1].astype(np.float64) for g, w in zip(gs, weights)]
    return sum(terms), sum(np.abs(t) for t in terms)


def bound(k, abs_sum, result):
    """|err_i| <= K * 2^-24 * sum_k |w_k g_k[i]| + one ulp of the float32 result.  Each of the K folds rounds once, by at most 2^-24 of
    a partial sum whose magnitude is at most sum_k |w_k g_k|; the ulp covers the comparison of a float32 with the float64 sum"""
    r = np.abs(np.asarray(result, dtype=np.float32))
    ulp = np.nextafter(r, np.float32(np.inf)).astype(np.float64) - r.astype(np.float64)
    return k * 2.0 ** -24 * abs_sum + ulp
