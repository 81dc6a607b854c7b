"""Plain references of the ensemble decode (sat_ensemble_logprobs, sat_beam_decode_ensemble, `sat.Ensemble`): numpy f64 / torch on
the CPU, one obvious line per rule, nothing shared with the code under test.

The combine.  lse_m = log-sum-exp of model m's row over all V columns; w_m = weight / sum(weights), rounded once to f32 (the value
the device is handed).  mode 0 ("prob"): out[v] = log sum_m w_m exp(x_m[v] - lse_m); -inf only where every model has -inf.
mode 1 ("logprob"): out[v] = sum_m w_m (x_m[v] - lse_m); -inf where any model has -inf; not renormalised.

Whole decodes.  The loops of tests/beam_constraints_reference.py (and, through `beam_groups_reference._grouped`, their grouped
form) are IMPORTED and driven with the combined log-probabilities in place of one model's logits: `_drive` wraps the loop's
`_select`, so the loop keeps the scores, prefixes, bans, gaps and back-pointers, while this module keeps the M members' own states
-- a plain torch-CPU LSTM per member -- and moves them by the parents the loop selected.  The selection takes log_softmax of the
combined row once more, as the step kernel does: an ensemble hypothesis's score is the sum of log_softmax(out)."""
import numpy as np
import torch

import beam_constraints_reference as BC
import beam_groups_reference as BG

GAP = 2e-4                                          # the whole-decode tests leave out images whose smallest key gap is <= GAP
END = 2


def pad4(n):
    return (n + 3) // 4 * 4


def weights32(weights, M):
    """the normalised weights as the device receives them: divided in f64, rounded once to f32 (returned as f64 values)"""
    w = np.ones(M, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    assert w.shape == (M,) and np.isfinite(w).all() and (w > 0).all()
    return (w / w.sum()).astype(np.float32).astype(np.float64)


def lse64(x):
    """log-sum-exp of every row of x in f64, [R, 1]"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    return m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def combine_ref(xs, weights=None, mode=0):
    """xs: M arrays [R, V] of logits -> the combined row [R, V] in f64"""
    w = weights32(weights, len(xs))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lp = np.stack([np.asarray(x, dtype=np.float64) - lse64(x) for x in xs])            # [M, R, V] log-probabilities
        if mode == 0:
            a = lp + np.log(w)[:, None, None]
            mx = a.max(axis=0)
            out = mx + np.log(np.exp(a - np.where(np.isfinite(mx), mx, 0.0)).sum(axis=0))
            return np.where(np.isneginf(mx), -np.inf, out)                                  # -inf only if every model has -inf
        out = (w[:, None, None] * np.where(np.isneginf(lp), 0.0, lp)).sum(axis=0)          # summed in model order
        return np.where(np.isneginf(lp).any(axis=0), -np.inf, out)                          # -inf if any model has -inf


# ---- inputs ----
def planted_rows(V, R, seed, nplants=6):
    """the rows of the beam step tests: a random background in [-1, 1) with min(V, nplants) plants 0.25 apart from 2.0 up, on random
    columns"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (R, V)).astype(np.float32)
    n = min(V, nplants)
    for r in range(R):
        x[r, rng.permutation(V)[:n]] = 2.0 + 0.25 * np.arange(n - 1, -1, -1)
    return x


def consensus_rows(M, R, V, rng, extra=0):
    """M matrices [R, V]: a background in [-1, 1); in every row member m has ITS OWN top column a_m at 4.0 (different per member)
    and all members share the runner-up column c at 3.5 -- every member alone picks a_m, the ensemble picks c.  extra: further
    shared plants 0.25 apart from 3.25 down (so that a beam has K distinct shared candidates per row).
    -> (xs, own [M, R], shared [R])"""
    assert V >= M + 1 + extra
    xs = [rng.uniform(-1.0, 1.0, (R, V)).astype(np.float32) for _ in range(M)]
    own, shared = np.zeros((M, R), dtype=np.int64), np.zeros(R, dtype=np.int64)
    for r in range(R):
        cols = rng.permutation(V)[:M + 1 + extra]
        shared[r] = cols[M]
        for m in range(M):
            own[m, r] = cols[m]
            xs[m][r, cols[m]] = 4.0
            xs[m][r, cols[M]] = 3.5
            for e in range(extra):
                xs[m][r, cols[M + 1 + e]] = 3.25 - 0.25 * e
    return xs, own, shared


def bases(B, K, stagger=0.0917):
    """the staggered start scores of the step tests"""
    return (-1.5 - 0.5 * np.arange(B, dtype=np.float32)[:, None] - np.float32(stagger) * np.arange(K, dtype=np.float32)[None, :])


# ---- whole decodes ----
def combine_torch(logits, w, mode):
    """the combine on torch tensors in their own dtype (the f32 restatement of the decode loops)"""
    lp = [torch.log_softmax(x, dim=1) for x in logits]
    if mode == 0:
        return torch.logsumexp(torch.stack([l + float(np.log(wm)) for l, wm in zip(lp, w)]), dim=0)
    out = torch.zeros_like(lp[0])
    for l, wm in zip(lp, w):
        out = out + float(wm) * l
    return out


def _drive(loop, logits_of, G, lam):
    """run `loop` (a call of one of BC's whole-decode loops) with `logits_of(previous order)` -- the combined log-probabilities of
    the step -- handed to its selection in place of the logits it computed itself; G > 1: under BG's grouped selection"""
    state = dict(order=None)

    def run():
        inner = BC._select

        def select(scores, logits, seqs, last, end_id, c, K):
            out = inner(scores, logits_of(state["order"]), seqs, last, end_id, c, K)
            state["order"] = out[0]
            return out

        BC._select = select
        try:
            return loop()
        finally:
            BC._select = inner

    return BG._grouped(run, G, lam) if G > 1 else run()


def lstm_step(p, l, x, h, c):
    """one nn.LSTM layer step, gate order i, f, g, o"""
    g = x @ p["lstm.weight_ih_l%d" % l].t() + p["lstm.bias_ih_l%d" % l] + h @ p["lstm.weight_hh_l%d" % l].t() + p["lstm.bias_hh_l%d" % l]
    i, f, gg, o = g.chunk(4, dim=1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def decoder_beam(members, feats, K, end_id, c=None, weights=None, mode=0, G=1, lam=0.0, steps=20):
    """members: [(params, num_layers)], feats: per member [B, E_m].  The beam search over the ensemble's distribution, in SEARCH
    order.  -> dict(ids [B,K,steps], scores [B,K], gap [B], nbans[, npen])"""
    M, B = len(members), feats[0].shape[0]
    V = members[0][0]["linear.weight"].shape[0]
    w = weights32(weights, M)
    xs = [f.repeat_interleave(K, 0) for f in feats]
    hs = [[torch.zeros(B * K, p["lstm.weight_hh_l%d" % l].shape[1]) for l in range(Lh)] for p, Lh in members]
    cs = [[torch.zeros_like(h) for h in hm] for hm in hs]

    def logits_of(order):
        if order is not None:                                    # follow the previous selection
            parent, token = order // V, order % V
            rows = (torch.arange(B).unsqueeze(1) * K + parent).reshape(-1)
            for m, (p, Lh) in enumerate(members):
                hs[m], cs[m] = [h[rows] for h in hs[m]], [cc[rows] for cc in cs[m]]
                xs[m] = p["embed.weight"][token.reshape(-1)]
        logits = []
        for m, (p, Lh) in enumerate(members):
            inp = xs[m]
            for l in range(Lh):
                hs[m][l], cs[m][l] = lstm_step(p, l, inp, hs[m][l], cs[m][l])
                inp = hs[m][l]
            logits.append(inp @ p["linear.weight"].t() + p["linear.bias"])
        return combine_torch(logits, w, mode)

    # the loop's own model has no layers and one-column weights: it only carries the search
    dummy = {"linear.weight": torch.zeros(V, 1), "linear.bias": torch.zeros(V), "embed.weight": torch.zeros(V, 1)}
    return _drive(lambda: BC.decoder_beam(dummy, torch.zeros(B, 1), K, 0, end_id, c or BC.Constraints(), steps=steps), logits_of, G, lam)


def attend_beam(ps, feats, K, end_id, c=None, weights=None, mode=0, G=1, lam=0.0, start_id=1, steps=20):
    """... for Show-Attend-Tell members (ps: their parameter dicts, feats: per member [B, P_m, C_m]), every member's step by the
    functions of oracle.attend.  The loop's own model is member 0 (it carries the search; its logits are not used)."""
    from oracle import attend as OA
    M, B = len(ps), feats[0].shape[0]
    V = ps[0]["classifier.weight"].shape[0]
    w = weights32(weights, M)
    fs = [f.repeat_interleave(K, 0) for f in feats]
    enc = [f @ p["image_att_w"] for p, f in zip(ps, fs)]
    hs = [torch.zeros(B * K, p["lstmcell.weight_hh"].shape[1]) for p in ps]
    cs = [torch.zeros_like(h) for h in hs]
    ctx, inp = [None] * M, [None] * M

    def logits_of(order):
        logits = []
        for m, p in enumerate(ps):
            if order is not None:
                parent, token = order // V, order % V
                rows = (torch.arange(B).unsqueeze(1) * K + parent).reshape(-1)
                hs[m], cs[m] = hs[m][rows], cs[m][rows]
                inp[m] = torch.cat([p["embedding.weight"][token.reshape(-1)], ctx[m][rows]], 1)
            ctx[m], _ = OA.attention_layer(p, fs[m], enc[m], hs[m])
            if order is None:
                inp[m] = torch.cat([p["embedding.weight"][torch.full((B * K,), start_id, dtype=torch.long)], ctx[m]], 1)
            hs[m], cs[m] = OA.lstmcell(p, inp[m], hs[m], cs[m])
            logits.append(OA.output_layer(p, ctx[m], hs[m]))
        return combine_torch(logits, w, mode)

    return _drive(lambda: BC.attend_beam(ps[0], feats[0], K, end_id, c or BC.Constraints(), None, start_id, steps), logits_of, G, lam)


# ---- the whole-decode cases of the GPU tests, fixed by a seed search against the references above only ----
def decoder_members(shapes, V, seed, scale=40.0):
    """[(params, num_layers)] for shapes [(E, H, num_layers)]: oracle initialisation, the projection scaled so that the
    distributions are peaked, <end> made likely enough to occur"""
    from oracle import decoder as OD
    gen = torch.Generator().manual_seed(seed)
    out = []
    for E, H, Lh in shapes:
        p = OD.init_decoder_params(E, H, V, Lh, generator=gen)
        p["linear.weight"] = p["linear.weight"] * scale
        p["linear.bias"][END] = 1.0
        out.append((p, Lh))
    return out


def first_seed(make, B, limit=60):
    """the convention of `build_case` in test_gpu_beam_groups.py: the first seed at which `make(seed)` -> dict with `ref` leaves
    no more than a quarter of the B images with a key gap <= GAP"""
    for seed in range(limit):
        case = make(seed)
        if int((case["ref"]["gap"] <= GAP).sum()) * 4 <= B:
            case["seed"] = seed
            return case
    raise AssertionError("no seed below %d leaves out at most a quarter of the images" % limit)


SHAPES = [(32, 64, 1), (48, 96, 2)]                 # two DecoderRNN members of different shape
V_DEC, B_DEC, K_DEC = 203, 5, 4
# the wide member path (one layer, >= 128 rows): B 32 makes R = 128.  "wide": the shapes above, so the one-layer member runs wide
# beside a narrow one, V odd (the exact-f32 projection); "wide_x3": two one-layer members, V % 4 == 0 (the split projection)
WIDE = dict(wide=(SHAPES, 203, 40.0), wide_x3=([(64, 256, 1), (32, 128, 1)], 1000, 20.0))
B_WIDE = 32


def decoder_case(kind):
    """kind: "plain" | "logprob" | "constrained" | "grouped" | "greedy" | "copies" | "wide" | "wide_x3"
    -> dict(members, feats, ref, kw, K, mode, seed, B, V)"""
    if kind in WIDE:
        shapes, V, scale = WIDE[kind]

        def make_wide(seed):
            members = decoder_members(shapes, V, seed, scale)
            gen = torch.Generator().manual_seed(1000 + seed)
            feats = [torch.randn(B_WIDE, p["embed.weight"].shape[1], generator=gen) for p, _ in members]
            ref = decoder_beam(members, feats, K_DEC, END)
            return dict(members=members, feats=feats, ref=ref, kw={}, K=K_DEC, mode=0, c=None, G=1, lam=0.0, B=B_WIDE, V=V)

        return first_seed(make_wide, B_WIDE)
    mode = 1 if kind == "logprob" else 0
    K = 1 if kind == "greedy" else K_DEC
    c, kw, G, lam = None, {}, 1, 0.0
    if kind == "constrained":
        c = BC.Constraints((), 3, 2, False, 0.7)
        kw = dict(no_repeat_ngram_size=2, min_length=3, length_penalty=0.7)
    if kind == "grouped":
        G, lam = 2, 0.6
        kw = dict(num_beam_groups=2, diversity_penalty=0.6)

    def make(seed):
        if kind == "copies":
            members = decoder_members(SHAPES[:1], V_DEC, seed) * 3
        else:
            members = decoder_members(SHAPES, V_DEC, seed)
        gen = torch.Generator().manual_seed(1000 + seed)
        feats = [torch.randn(B_DEC, p["embed.weight"].shape[1], generator=gen) for p, _ in members]
        if kind == "copies":
            feats = [feats[0]] * 3
        ref = decoder_beam(members, feats, K, END, c, None, mode, G, lam)
        return dict(members=members, feats=feats, ref=ref, kw=kw, K=K, mode=mode, c=c, G=G, lam=lam, B=B_DEC, V=V_DEC)

    return first_seed(make, B_DEC)


def attend_case(constrained):
    """two tiny Show-Attend-Tell members at the G6 golden's dimensions and features (the second member sees the features reversed
    along the batch's feature positions, as another encoder would give other features)"""
    import os
    from oracle import attend as OA
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G6_attend_small.npz"))
    hidden, context, vocab, embed, B, T, P, feat = [int(x) for x in z["dims"]]
    f0 = torch.from_numpy(z["features"])
    feats = [f0, f0.flip(1).contiguous()]
    c = BC.Constraints((), 3, 2, False, 0.0) if constrained else None
    kw = dict(no_repeat_ngram_size=2, min_length=3) if constrained else {}

    def make(seed):
        ps = []
        for m in range(2):
            p = OA.init_attend_params(hidden, context, vocab, embed, generator=torch.Generator().manual_seed(100 * seed + m), feat=feat)
            p["classifier.weight"] = p["classifier.weight"] * 8.0
            p["classifier.bias"] = p["classifier.bias"].clone()
            p["classifier.bias"][END] += 0.5
            ps.append(p)
        ref = attend_beam(ps, feats, 4, END, c)
        return dict(ps=ps, feats=feats, ref=ref, kw=kw, K=4, c=c, dims=(hidden, context, vocab, embed, B, P, feat))

    return first_seed(make, B, limit=20)
