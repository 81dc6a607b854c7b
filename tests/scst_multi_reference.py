"""numpy float64 restatement of `sat_scst_weights_group` and `sat_group_sum_rows` (include/sat_hip.h): exactly the operations the
header states, in its order, one Python float (an IEEE double) at a time.  Rows are image-major: row r = b * S + s."""
import numpy as np

import scst_reference as S1


def weights_group(ids, reward, baseline_img=None, mode=0, end_id=2, denom=None):
    """ids [B, S, T]; reward [B * S]; baseline_img [B] or None (mode 0 only).  Returns (w f32 [T * R] with row t * R + r, len i32
    [R], M f64, advantage f64 [R], baseline_rows f64 [R])"""
    ids = np.asarray(ids)
    B, S, T = ids.shape
    R = B * S
    assert mode in (0, 1) and not (mode == 1 and (S < 2 or baseline_img is not None))
    ln = S1.lengths(ids.reshape(R, T), end_id)
    M = float(int(ln.astype(np.int64).sum())) if denom is None else float(denom)
    rw = [float(x) for x in np.asarray(reward, dtype=np.float64).reshape(R)]              # (f32 -> f64 is exact)
    adv, base = np.empty(R, dtype=np.float64), np.empty(R, dtype=np.float64)
    for r in range(R):
        b, s = divmod(r, S)
        if mode == 0:
            bl = 0.0 if baseline_img is None else float(np.asarray(baseline_img, dtype=np.float64).reshape(B)[b])
            a = rw[r] - bl
        else:
            da, sb = 0.0, 0.0
            for o in range(S):
                if o == s:
                    continue
                da = da + (rw[r] - rw[b * S + o])
                sb = sb + rw[b * S + o]
            a, bl = da / float(S - 1), sb / float(S - 1)
        adv[r], base[r] = a, bl
    w = np.zeros((T, R), dtype=np.float32)
    for r in range(R):
        w[:ln[r], r] = np.float32(np.float64(adv[r]) / np.float64(M))
    return w.reshape(-1), ln, np.float64(M), adv, base


def group_sum_rows(x, S):
    """x f32 [B * S, W] -> [B, W]: out[b] = ((x[b*S] + x[b*S+1]) + x[b*S+2]) + ..., every add rounded to float32"""
    x = np.asarray(x, dtype=np.float32)
    B = x.shape[0] // S
    out = x[0::S][:B].copy()
    for s in range(1, S):
        out = (out + x[s::S][:B]).astype(np.float32)
    return out


def group_ids(B, S, T, end_id, seed):
    """ids [B, S, T] over 3..8 with the edge rows the kernel's length rule has: a row ending at step 0, a row with no <end>, an
    <end> in the last column only, and <end> at every other position in turn"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.integers(3, 9, (B * S, T))
    for r in range(B * S):
        k = r % (T + 2)
        if k < T:
            ids[r, k] = end_id               # k = 0: ends at step 0; k = T - 1: <end> in the last column
        # k == T, T + 1: no <end>
    return ids.reshape(B, S, T)


def group_rewards(B, S, seed):
    """rewards [B * S] f64 with negatives, zeros, repeats within an image, and one image whose rewards are all equal (0.1)"""
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    rw = (rng.random((B, S)) * 4 - 1.5)
    rw[:, 0] = np.where(np.arange(B) % 3 == 0, 0.0, rw[:, 0])
    if S > 1:
        rw[:, S - 1] = np.where(np.arange(B) % 2 == 1, rw[:, 0], rw[:, S - 1])     # a repeat within the image
    rw[B // 2, :] = 0.1                                                              # every sample alike: exact zeros (mode 1)
    return rw.reshape(-1)


# Argument sets `sat_scst_weights_group` / `sat_group_sum_rows` must refuse before anything is enqueued, as overrides of a valid
# call.  "PTR" stands for some non-null device address the caller supplies; group-sum addresses are byte offsets from the caller's
# `in` (rows [B * S = 6][ld 8], W 8) and `out` ([2][8]) buffers.
WEIGHTS_GROUP_VALID = dict(stride=4, B=3, S=2, T=4, mode=0, baseline=None, denom=None)
WEIGHTS_GROUP_ARG_ERRORS = [dict(ids=None), dict(reward=None), dict(w=None), dict(len=None), dict(m=None), dict(adv=None),
                            dict(B=0), dict(S=0), dict(T=0), dict(B=-1), dict(mode=2), dict(mode=-1), dict(mode=1, S=1),
                            dict(mode=1, baseline="PTR"), dict(stride=3), dict(B=1 << 20, S=256, T=8, stride=8),
                            dict(B=1 << 30, S=4, T=1)]
WEIGHTS_GROUP_UNSUPPORTED = [dict(S=257), dict(S=257, mode=1), dict(S=1 << 20, B=1)]
GROUP_SUM_VALID = dict(ld_in=8, B=2, S=3, W=8, ld_out=8)
GROUP_SUM_ARG_ERRORS = [dict(inp=None), dict(out=None), dict(B=0), dict(S=0), dict(W=0), dict(W=-4), dict(ld_in=7), dict(ld_out=7),
                        dict(out="in+0"), dict(out="in+%d" % (4 * (5 * 8 + 7))), dict(out="in-%d" % (4 * (8 + 7)))]
