"""numpy f64 restatement of the filtered draw (include/sat_hip.h, `sat_sample_filtered`): the total order of a row, the top-k and
nucleus prefix, the Gumbel-max draw among the kept columns and the log-probability of the drawn token -- what the tests recompute
the library's stochastic decode with."""
import numpy as np

import ss_reference as SS


def total_order(x):
    """The candidates of a row -- columns above -inf, NaN excluded -- by value descending, equal values by ascending column
    (+0.0 == -0.0 as floats compare)"""
    x = np.asarray(x, dtype=np.float64)
    cand = np.flatnonzero(x > -np.inf)                       # (NaN > -inf is False)
    return cand[np.argsort(-x[cand], kind="stable")]


def kept_prefix(x, tau, k, p):
    """(order, n, clearance): the total order [n_candidates] int64, the size n of the kept prefix after top-k (0 < k < candidates)
    and the nucleus (p < 1: the shortest prefix whose cumulative w = exp((x - max) / tau) reaches p * Z, Z over the top-k
    survivors, at least one token), and the clearance of the nucleus decision: the smaller distance of the two cumulative sums
    around the cut from p * Z, divided by Z (inf when the nucleus is off)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    tau, p = float(np.float32(tau)), float(np.float32(p))
    order = total_order(x)
    n = len(order)
    if 0 < k < n:
        n = int(k)
    clearance = np.inf
    if p < 1 and n > 0:
        w = np.exp((x[order[:n]] - x[order[0]]) / tau)
        cum = np.cumsum(w)
        Z = cum[-1]
        m = int(np.searchsorted(cum, p * Z, side="left")) + 1          # the first prefix with cum >= p * Z
        m = min(max(m, 1), n)
        below = cum[m - 2] if m >= 2 else 0.0
        clearance = min(abs(cum[m - 1] - p * Z), abs(p * Z - below)) / Z
        n = m
    return order, n, clearance


def draw(x, tau, kept, seed, rank, r, t):
    """(token, margin): the first arg-max over the columns `kept` of x / tau + G(r, t, v), and the gap to the runner-up (inf when
    one column is kept)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    kept = np.sort(np.asarray(kept, dtype=np.int64))
    g = SS.noise(seed, rank, r, t, len(x))
    s = x[kept] / float(np.float32(tau)) + g[kept]
    top = np.argsort(-s, kind="stable")
    margin = s[top[0]] - s[top[1]] if len(top) > 1 else np.inf
    return int(kept[top[0]]), float(margin)


def logp(x, tau, kept, token):
    """ln(w_token / sum of w over kept), f64"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    kept = np.asarray(kept, dtype=np.int64)
    tau = float(np.float32(tau))
    m = x[kept].max()
    w = np.exp((x[kept] - m) / tau)
    return float((x[token] - m) / tau - np.log(w.sum()))


def probabilities(x, tau, k, p):
    """the filtered softmax of a row, f64 [V]"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    order, n, _ = kept_prefix(x, tau, k, p)
    kept = order[:n]
    w = np.exp((x[kept] - x[kept].max()) / float(np.float32(tau)))
    out = np.zeros(len(x))
    out[kept] = w / w.sum()
    return out
