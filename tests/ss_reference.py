"""numpy restatement of the scheduled-sampling random numbers (include/sat_hip.h, `sat_ss_decoder_fwd`): Philox4x32-10, the uniform
and Gumbel maps, and the per-row decisions of one forward -- what the tests recompute the library's draws with."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123) on broadcastable uint32 arrays; returns the 4 output words as uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint32) for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint32(k0), np.uint32(k1)
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0 = np.uint32(k0 + W0)
                k1 = np.uint32(k1 + W1)
            p0 = M0 * c[0].astype(np.uint64)
            p1 = M1 * c[2].astype(np.uint64)
            c = [((p1 >> np.uint64(32)).astype(np.uint32) ^ c[1] ^ k0), (p1 & _LO).astype(np.uint32),
                 ((p0 >> np.uint64(32)).astype(np.uint32) ^ c[3] ^ k1), (p0 & _LO).astype(np.uint32)]
    return c


def seed_key(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def uniform(x):
    """u = ((x >> 8) + 0.5) * 2^-24 in float64 (exact)"""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def gumbel(x):
    """G = -log(-log u), float64"""
    return -np.log(-np.log(uniform(x)))


def noise(seed, rank, b, t, V):
    """G(b, t, v) for v < V, float64 [V]"""
    k0, k1 = seed_key(seed)
    v = np.arange(V)
    words = philox4x32_10(v >> 2, b, t, 2 * rank, k0, k1)
    x = np.choose(v & 3, words)
    return gumbel(x)


def mask_uniform(seed, rank, b, t):
    k0, k1 = seed_key(seed)
    return float(uniform(philox4x32_10(0, b, t, 2 * rank + 1, k0, k1)[0]))


def draws(logits, batch_sizes, captions, ss_prob, seed, rank=0):
    """Replay of one forward's decisions from its packed f32 logits [N, >= V] (float64 arithmetic).  captions: the teacher's
    inputs [B, >= T-1].  Returns (used [B, T-1] int64, mask [B, T-1] bool, margin [B, T-1] float64): margin is the gap
    between the best and second-best perturbed score of a drawn entry (inf elsewhere)."""
    T = len(batch_sizes)
    B = batch_sizes[0]
    prefix = np.concatenate([[0], np.cumsum(batch_sizes)])
    used = np.array(captions[:, :max(T - 1, 0)], dtype=np.int64, copy=True)
    mask = np.zeros(used.shape, dtype=bool)
    margin = np.full(used.shape, np.inf)
    V = logits.shape[1]
    p = np.float64(np.float32(ss_prob))
    for t in range(2, T):
        for b in range(batch_sizes[t]):
            if not mask_uniform(seed, rank, b, t) < p:
                continue
            mask[b, t - 1] = True
            s = logits[prefix[t - 1] + b].astype(np.float64) + noise(seed, rank, b, t, V)
            top = np.argsort(-s, kind="stable")[:2]
            used[b, t - 1] = int(np.argmax(s))
            margin[b, t - 1] = s[top[0]] - s[top[1]]
    assert B == used.shape[0]
    return used, mask, margin
