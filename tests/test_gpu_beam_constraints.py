"""GPU: the constrained beam search -- sat_beam_step_ex (beam_row_ban_kernel<256> + beam_merge_kernel), sat_beam_rerank,
sat_beam_decode_ex and the `sample_beam` keywords -- against the plain references of tests/beam_constraints_reference.py.

Step level.  Logits are a random background in [-1, 1) with K + 4 plants per row 0.25 apart from 2.0 up, the highest of every row
on a column the case bans; bases are staggered per row.  A case is built from the first seed at which the f64 reference's best
K + 1 candidates of every image lie more than MARGIN = 1e-3 apart (asserted before anything runs), so parents and tokens are
compared exactly; scores to atol 1e-5, the tolerance test_beam_step_ties_dead_and_finished_hypotheses grants the same expression.
Which row path runs follows from (V, ldl): the register path for ldl % 4 == 0 and 4 <= V <= 12291, the long path otherwise.

Whole decode.  The f32 CPU restatement reports, per image, the smallest gap between consecutive candidates among the best K + 1
over all steps; ids are compared exactly and scores to 1e-4 on the images whose gap exceeds 2e-4 (twice the 1e-4 the existing beam
tests grant device against oracle), and at most a quarter of the images may be left out."""
import functools
import importlib
import math
import os

import numpy as np
import pytest
import torch

import beam_constraints_reference as BC

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
MARGIN, ATOL = 1e-3, 1e-5
GAP, DECODE_ATOL = 2e-4, 1e-4
STAGGER = 0.0917


def pad4(n):
    return (n + 3) // 4 * 4


def make_struct(c, dev="cuda"):
    """(sat_beam_constraints, the tensor it points to) of a reference `Constraints`"""
    t = torch.tensor(list(c.suppress_ids), dtype=torch.int64, device=dev) if c.suppress_ids else None
    return L.SatBeamConstraints(t.data_ptr() if t is not None else None, len(c.suppress_ids), c.min_length, c.no_repeat_ngram,
                                int(c.block_repeat), c.length_penalty), t


def device_step(x, ldl, scores, last, end_id, K, c="plain", parents=None, tokens=None, i=0, T=20, fill=0.0):
    """one step on the device: c == "plain": sat_beam_step; None: sat_beam_step_ex with a NULL struct; else a `Constraints`"""
    lib = L.load()
    R, V = x.shape
    B = R // K
    buf = np.full((R, ldl), fill, dtype=np.float32)
    buf[:, :V] = x
    logits = torch.from_numpy(buf).cuda()
    sc = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)).cuda()
    lt = None if last is None else torch.from_numpy(np.ascontiguousarray(last, dtype=np.int64).reshape(-1)).cuda()
    parent = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    token = torch.full((R,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((R,), float("nan"), device="cuda")
    ws = torch.empty(lib.sat_beam_step_ex_ws_bytes(B, K, V, T), dtype=torch.uint8, device="cuda")
    if isinstance(c, str):
        L.check(lib.sat_beam_step(logits.data_ptr(), ldl, sc.data_ptr(), L.ptr(lt), end_id, B, K, V, parent.data_ptr(), token.data_ptr(),
                                  out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "sat_beam_step")
    else:
        pr = None if parents is None else torch.from_numpy(np.ascontiguousarray(parents, dtype=np.int32)).cuda()
        tk = None if tokens is None else torch.from_numpy(np.ascontiguousarray(tokens, dtype=np.int64)).cuda()
        s, keep = make_struct(c) if c is not None else (None, None)
        L.check(lib.sat_beam_step_ex(logits.data_ptr(), ldl, sc.data_ptr(), L.ptr(lt), end_id, B, K, V, s, L.ptr(pr), L.ptr(tk), i, T,
                                     parent.data_ptr(), token.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()),
                "sat_beam_step_ex")
    torch.cuda.synchronize()
    return parent.cpu().numpy().astype(np.int64).reshape(B, K), token.cpu().numpy().reshape(B, K), out.cpu().numpy().reshape(B, K)


def bases(B, K):
    return (-1.5 - 0.5 * np.arange(B, dtype=np.float32)[:, None] - np.float32(STAGGER) * np.arange(K, dtype=np.float32)[None, :])


def planted_rows(V, R, K, edge, rng):
    """background + min(V, K + 4) plants per row; the row's HIGHEST plant sits on edge[r % len(edge)]"""
    x = rng.uniform(-1.0, 1.0, (R, V)).astype(np.float32)
    npl = min(V, K + 4)
    for r in range(R):
        cols = [int(edge[r % len(edge)])]
        for col in rng.permutation(V):
            if len(cols) >= npl:
                break
            if int(col) not in cols:
                cols.append(int(col))
        x[r, cols] = 2.0 + 0.25 * np.arange(npl - 1, -1, -1)
    return x


def well_formed(ref, K):
    for b in range(ref["cand"].shape[0]):
        top = -np.sort(-ref["cand"][b])[:K + 1]
        top = top[np.isfinite(top)]
        if top.size > 1 and not ((top[:-1] - top[1:]) > MARGIN).all():
            return False
    return True


def build_case(make, limit=200):
    """the first seed at which `make(rng)` -> (inputs, ref) is well formed; the search sees the f64 reference only"""
    for seed in range(limit):
        inputs, ref, K = make(np.random.default_rng(seed))
        if well_formed(ref, K):
            return inputs, ref
    raise AssertionError("no well-formed case below seed %d" % limit)


def check_exact(got, ref, K, V, tag):
    parent, token, out = got
    for b in range(parent.shape[0]):
        n = int(ref["live"][b])
        assert parent[b, :n].tolist() == ref["parent"][b, :n].tolist() and token[b, :n].tolist() == ref["token"][b, :n].tolist(), \
            (tag, b, parent[b].tolist(), token[b].tolist(), ref["parent"][b].tolist(), ref["token"][b].tolist())
        err = np.abs(out[b, :n].astype(np.float64) - ref["scores"][b, :n]).max() if n else 0.0
        print("%s image %d: %d live, score error %.3g (atol %.3g)" % (tag, b, n, err, ATOL))
        assert err <= ATOL, (tag, b)
        # fewer than K candidates: -inf / parent 0 / token 0 in the surplus slots
        assert np.isneginf(out[b, n:]).all() and (parent[b, n:] == 0).all() and (token[b, n:] == 0).all(), (tag, b)


# ---- step level: ban placement over the shapes ----
def edge_columns(V):
    nq = V >> 2
    tails = list(range(4 * nq, V)) if V >= 7 else []
    return sorted({0, V - 1} | set(tails) | {v for v in (31, 32, 63, 64) if v < V})


@pytest.mark.parametrize("V", [3, 7, 203, 700, 4100, 12292, 12300])
def test_banned_columns_over_shapes(V):
    """suppressed columns at 0, V - 1, every V % 4 tail column, the bitmap word edges 31 / 32 / 63 / 64, every row's arg-max, and
    two ids in the pad columns of ldl (no effect); end_id held back by min_length (V >= 7).  V 3: no whole chunk; 7, 203: a tail;
    203 / 700: one chunk per thread at most; 4100: several; 12292 / 12300: the long path.  ldl == pad4(V) and ldl > V"""
    edge = edge_columns(V)
    end_id = 1 if V >= 7 else -1
    c = BC.Constraints(suppress_ids=edge + [V, V + 1], min_length=1 if V >= 7 else 0)
    for K, B in ((1, 5), (3, 2), (8, 1)):
        def make(rng, K=K, B=B):
            x = planted_rows(V, B * K, K, edge, rng)
            sc = bases(B, K)
            return (x, sc), BC.step_ref(x, sc, None, end_id, K, [[[]] * K] * B, c), K
        (x, sc), ref = build_case(make)
        plain = BC.step_ref(x, sc, None, end_id, K, [[[]] * K] * B, BC.Constraints())
        assert ref["nbans"] >= B * K * len(edge) and (plain["token"][:, 0] != ref["token"][:, 0]).all()     # the ban changes the winner
        assert np.isin(plain["token"][:, 0], edge).all()
        for ldl, fill in ((pad4(V), 0.0), (pad4(V) + 4, np.inf)):
            got = device_step(x, ldl, sc, None, end_id, K, c, i=0, fill=fill)
            check_exact(got, ref, K, V, "V%d K%d B%d ldl%d" % (V, K, B, ldl))
            assert not np.isin(got[1][np.isfinite(got[2])], edge + ([end_id] if end_id >= 0 else [])).any()


def test_scores_are_not_renormalised():
    """a row with 90 % of its mass on a banned column: the survivors keep base + x - lse over ALL columns"""
    K, V, base = 2, 700, -0.75
    x = np.zeros((K, V), dtype=np.float32)
    x[:, 64] = np.float32(math.log(9 * (V - 1)))
    x[0, 5], x[1, 9] = 1.0, 0.5
    sc = np.array([[base, base]], dtype=np.float32)
    lse0 = math.log((V - 2) + math.exp(float(x[0, 64])) + math.exp(1.0))
    lse1 = math.log((V - 2) + math.exp(float(x[1, 64])) + math.exp(0.5))
    parent, token, out = device_step(x, V, sc, None, -1, K, BC.Constraints(suppress_ids=[64]), i=0)
    assert parent.tolist() == [[0, 1]] and token.tolist() == [[5, 9]]
    np.testing.assert_allclose(out[0], [base + 1.0 - lse0, base + 0.5 - lse1], rtol=0, atol=ATOL)
    renorm = base + 1.0 - math.log((V - 2) + math.exp(1.0))                     # what a renormalising implementation would return
    assert abs(renorm - (base + 1.0 - lse0)) > 2.0


# ---- step level: the prefix walk ----
def shuffling_parents(rng, T, B, K):
    """parents [T, B, K]: at every step, in every image, a permutation of the slots that is not the identity"""
    out = np.zeros((T, B, K), dtype=np.int32)
    for t in range(T):
        for b in range(B):
            while K > 1 and (out[t, b] == np.arange(K)).all() or out[t, b].sum() != K * (K - 1) // 2:
                out[t, b] = rng.permutation(K)
    return out


@pytest.mark.parametrize("V,ldl,K", [(203, 204, 3), (12292, 12292, 8)])
def test_ngram_and_repeat_bans_follow_the_parent_chain(V, ldl, K):
    """T = 20 records whose parents permute the slots at every step and whose tokens come from three columns, so n-grams recur;
    steps i in {0, 1, n - 1, n, 19} for n = 1, 2, 3, with and without block_repeat.  Rows >= i of the records are traps: they name
    the best unbanned column, so a walk that read them would change the winner"""
    T, B = 20, 2
    alphabet = [5, 31, 32, 64, V - 1]
    rec = np.random.default_rng(V)
    parents = shuffling_parents(rec, T, B, K)
    tokens = rec.choice(alphabet[:3], (T, B, K)).astype(np.int64)             # three symbols: trigrams recur within 19 tokens
    fired, by_n = 0, {1: 0, 2: 0, 3: 0}
    for n in (1, 2, 3):
        for block in (False, True):
            for i in sorted({0, 1, n - 1, n, 19}):
                c = BC.Constraints(no_repeat_ngram=n, block_repeat=block)
                prefixes = BC.prefixes_ref(parents, tokens, i)

                def make(rng):
                    x = planted_rows(V, B * K, K, alphabet, rng)
                    x[:, alphabet] = x[:, alphabet] + 3.0 + 0.3 * rng.permutation(len(alphabet))       # the alphabet leads every row
                    sc = bases(B, K)
                    return (x, sc), BC.step_ref(x, sc, None, -1, K, prefixes, c), K
                (x, sc), ref = build_case(make)
                fired += ref["nbans"]
                assert ref["nbans"] == 0 or i >= n or (block and i >= 1), (n, block, i)
                assert ref["nbans"] > 0 or not (i >= 1 and (n == 1 or block)), (n, block, i)
                by_n[n] += ref["nbans"] if not block else 0
                trap_par, trap_tok = parents.copy(), tokens.copy()
                trap_par[i:] = 0
                trap_tok[i:] = ref["token"][0, 0]
                last = tokens[i - 1] if i > 0 else None
                got = device_step(x, ldl, sc, last, -1, K, c, trap_par.reshape(T, B * K), trap_tok.reshape(T, B * K), i, T)
                check_exact(got, ref, K, V, "n%d block%d i%d" % (n, block, i))
    assert fired > 100 and all(v > 0 for v in by_n.values())          # every n banned something on its own


def test_finished_and_dead_rows_are_untouched_by_every_constraint():
    """finished rows (last token == end_id) beside live and dead ones, every constraint on, end_id itself held back by min_length:
    a finished row still continues with end_id at its unchanged score, a dead row has no candidate"""
    T, B, K, V, i, end_id = 20, 2, 4, 700, 5, 9
    rec = np.random.default_rng(3)
    parents = shuffling_parents(rec, T, B, K)
    tokens = rec.choice([5, 31, 64, 300], (T, B, K)).astype(np.int64)
    tokens[i - 1, 0, 1] = tokens[i - 1, 1, 3] = tokens[i - 1, 1, 0] = end_id                        # finished slots
    c = BC.Constraints(suppress_ids=[0, 31, V - 1], min_length=10, no_repeat_ngram=1, block_repeat=True)
    prefixes = BC.prefixes_ref(parents, tokens, i)

    def make(rng):
        x = planted_rows(V, B * K, K, [31, 5, 64, 300], rng)
        x[:, end_id] = 6.0                                                                          # <end> is every row's arg-max
        sc = bases(B, K)
        sc[0, 1] = -0.25                                                                            # a finished row in front
        sc[0, 2] = sc[1, 0] = -np.inf                                                               # dead (one of them finished too)
        return (x, sc), BC.step_ref(x, sc, tokens[i - 1], end_id, K, prefixes, c), K
    (x, sc), ref = build_case(make)
    got = device_step(x, V, sc, tokens[i - 1], end_id, K, c, parents.reshape(T, B * K), tokens.reshape(T, B * K), i, T)
    check_exact(got, ref, K, V, "finished-dead")
    parent, token, out = got
    assert (parent[0, 0], token[0, 0]) == (1, end_id) and out[0, 0] == np.float32(-0.25)           # unchanged, bit for bit
    live_rows = [(b, k) for b in range(B) for k in range(K) if np.isfinite(sc[b, k]) and tokens[i - 1, b, k] != end_id]
    for b in range(B):
        for p, t, s in zip(parent[b], token[b], out[b]):
            if np.isfinite(s) and (b, int(p)) in live_rows:
                assert t != end_id and t not in (0, 31, V - 1) and t not in prefixes[b][int(p)], (b, p, t)
            assert not (b, int(p)) in ((0, 2), (1, 0)) or not np.isfinite(s)


@pytest.mark.parametrize("V,ldl", [(700, 700), (12300, 12300), (7, 7), (203, 204)])
def test_constraints_off_is_sat_beam_step_bit_for_bit(V, ldl):
    """c == NULL, every field off, and fields that ban nothing at this step: parent, token and scores `torch.equal` to sat_beam_step
    (the same launches), on the register and the long path"""
    T, B, K, i, end_id = 20, 2, 5, 2, 2
    rng = np.random.default_rng(V)
    x = np.clip(rng.normal(0.0, 2.0, (B * K, V)), -8, 8).astype(np.float32)
    sc = bases(B, K)
    sc[1, 4] = -np.inf
    parents = rng.integers(0, K, (T, B * K)).astype(np.int32)
    tokens = rng.integers(0, V, (T, B * K)).astype(np.int64)
    last = tokens[i - 1].copy()
    last[3] = end_id
    want = device_step(x, ldl, sc, last, end_id, K, "plain")
    for name, c, at in (("NULL", None, i), ("all off", BC.Constraints(), i), ("penalty only", BC.Constraints(length_penalty=0.7), i),
                        ("nothing banned yet", BC.Constraints(min_length=2, no_repeat_ngram=3), i),
                        ("block_repeat at 0", BC.Constraints(block_repeat=True), 0)):
        got = device_step(x, ldl, sc, last, end_id, K, c, parents, tokens, at, T)
        for a, w in zip(got, want):
            assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, w.view(np.int32) if w.dtype == np.float32 else w), name


# ---- sat_beam_rerank ----
def device_rerank(ids, scores, end_id, alpha):
    lib = L.load()
    B, K, T = ids.shape
    i_d, s_d = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
    ids_out = torch.full((B, K, T), -7, dtype=torch.int64, device="cuda")
    sc_out, norm = torch.full((B, K), float("nan"), device="cuda"), torch.full((B, K), float("nan"), device="cuda")
    order = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    L.check(lib.sat_beam_rerank(i_d.data_ptr(), s_d.data_ptr(), B, K, T, end_id, alpha, ids_out.data_ptr(), sc_out.data_ptr(),
                                norm.data_ptr(), order.data_ptr(), L.stream()), "sat_beam_rerank")
    torch.cuda.synchronize()
    return ids_out.cpu().numpy(), sc_out.cpu().numpy(), norm.cpu().numpy(), order.cpu().numpy().astype(np.int64)


def test_rerank_hand_made_rows():
    """L counts the <end>; a row without one has L = T; equal norms keep the previous rank; -inf stays last; alpha 0: identity"""
    ids = np.array([[[5, 2, 2, 2], [5, 6, 7, 2], [5, 6, 7, 8], [2, 2, 2, 2]],
                    [[5, 2, 7, 7], [5, 6, 7, 2], [9, 9, 9, 9], [4, 2, 4, 4]]])
    scores = np.array([[-2.0, -3.0, -3.5, -np.inf], [-2.0, -4.0, -np.inf, -np.inf]], dtype=np.float32)
    ids_out, sc_out, norm, order = device_rerank(ids, scores, 2, 1.0)
    assert order.tolist() == [[1, 2, 0, 3], [0, 1, 2, 3]]                      # image 1: -2 / 2 == -4 / 4 keeps 0 in front of 1
    assert norm[0, :3].tolist() == [-0.75, -0.875, -1.0] and np.isneginf(norm[0, 3])
    assert norm[1, :2].tolist() == [-1.0, -1.0] and np.isneginf(norm[1, 2:]).all()
    assert sc_out[0].tolist()[:3] == [-3.0, -3.5, -2.0] and np.isneginf(sc_out[0, 3])
    assert np.array_equal(ids_out, np.take_along_axis(ids, order[:, :, None], 1))
    ids_out, sc_out, norm, order = device_rerank(ids, scores, 2, 0.0)
    assert order.tolist() == [[0, 1, 2, 3]] * 2 and np.array_equal(ids_out, ids)
    assert np.array_equal(sc_out.view(np.int32), scores.view(np.int32)) and np.array_equal(norm.view(np.int32), scores.view(np.int32))


@pytest.mark.parametrize("K,T,alpha", [(1, 1, 0.7), (5, 20, 0.7), (8, 20, 2.0), (8, 70, 0.3), (3, 64, 1.0)])
def test_rerank_random_rows_against_f64(K, T, alpha):
    """norm within 1e-6 relative of the f64 reference; the order exact on the images whose reference norms differ by more than
    1e-5 relative (most of them: asserted)"""
    B, end_id = 9, 2
    rng = np.random.default_rng([K, T])
    ids = rng.integers(3, 50, (B, K, T))
    for b in range(B):
        for k in range(K):
            if rng.random() < 0.7:
                ids[b, k, rng.integers(0, T):] = end_id
    scores = -np.sort(rng.uniform(0.5, 30.0, (B, K)), axis=1).astype(np.float32)
    scores[1, K - 1:] = -np.inf
    ref = BC.rerank_ref(ids, scores, end_id, np.float32(alpha))
    ids_out, sc_out, norm, order = device_rerank(ids, scores, end_id, alpha)
    exact = 0
    for b in range(B):
        fin = np.isfinite(ref["norm"][b])
        rel = np.abs(norm[b][fin] - ref["norm"][b][fin]) / np.abs(ref["norm"][b][fin])
        # the device's norm is in ITS order: compare per hypothesis through the order it reports
        by_hyp = np.empty(K)
        by_hyp[order[b]] = norm[b]
        ref_by_hyp = np.empty(K)
        ref_by_hyp[ref["order"][b]] = ref["norm"][b]
        f = np.isfinite(ref_by_hyp)
        assert np.array_equal(np.isfinite(by_hyp), f)
        rel = np.abs(by_hyp[f] - ref_by_hyp[f]) / np.abs(ref_by_hyp[f])
        assert rel.size == 0 or rel.max() <= 1e-6, (b, rel.max())
        assert sorted(order[b].tolist()) == list(range(K))
        assert np.array_equal(ids_out[b], ids[b][order[b]]) and np.array_equal(sc_out[b], scores[b][order[b]])
        rn = ref["norm"][b][fin]
        if rn.size < 2 or (np.abs(rn[:-1] - rn[1:]) / np.abs(rn[:-1]) > 1e-5).all():
            exact += 1
            assert order[b].tolist() == ref["order"][b].tolist(), b
    assert exact >= B - 2


# ---- whole decode ----
END, SUPPRESS, MINLEN = 2, [3, 0, 1], 6


def _decoder_case(E, H, V, B, K, Lh, seed, scale, n, block):
    from oracle import decoder as OD
    gen = torch.Generator().manual_seed(seed)
    params = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    params["linear.weight"] = params["linear.weight"] * scale
    params["linear.bias"][END] = 1.0                                # so that <end> occurs
    feats = torch.randn(B, E, generator=gen)
    c = BC.Constraints(SUPPRESS, MINLEN, n, block)
    ref = BC.decoder_beam(params, feats, K, Lh, END, c)
    plain = OD.beam_search(params, feats, K, Lh, end_id=END)
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    dec.cuda().eval()
    kw = dict(suppress_ids=SUPPRESS, min_length=MINLEN, no_repeat_ngram_size=n, block_repeat=block)
    ids, scores = dec.sample_beam(feats.cuda(), beam_size=K, end_id=END, return_all=True, **kw)
    return dict(dec=dec, params=params, feats=feats, c=c, ref=ref, plain=plain, K=K, kw=kw, ids=ids, scores=scores,
                norm=dec.last_beam_norm_scores, order=dec.last_beam_order)


@functools.lru_cache(maxsize=None)
def wide_case():
    return _decoder_case(64, 256, 1000, 32, 5, 1, 99, 20.0, 2, True)


@functools.lru_cache(maxsize=None)
def narrow_case():
    return _decoder_case(32, 64, 203, 8, 3, 2, 11, 40.0, 3, False)


def check_decode(ids, scores, ref, plain_ids, B, tag):
    keep = (ref["gap"] > GAP).numpy()
    print("%s: %d of %d images left out (gap <= %.0e); smallest kept gap %.3g; %d bans" %
          (tag, int((~keep).sum()), B, GAP, float(ref["gap"][torch.from_numpy(keep)].min()), ref["nbans"]))
    assert (~keep).sum() * 4 <= B                                   # at most a quarter left out
    assert ref["nbans"] > 0 and (ref["ids"] != plain_ids).any()     # the constraints fired and changed the result
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    assert np.array_equal(ids[keep], ref["ids"].numpy()[keep])
    err = np.abs(scores[keep] - ref["scores"].numpy()[keep]).max()
    print("%s: score error %.3g (atol %.0e)" % (tag, err, DECODE_ATOL))
    assert err <= DECODE_ATOL


def test_wide_constrained_decode_matches_the_cpu_restatement():
    """the wide path (160 rows, one layer, the projection on the bf16 pipe): bigram blocking, no immediate repeat, three
    suppressed ids, <end> not before position 6"""
    w = wide_case()
    assert tuple(w["ids"].shape) == (32, 5, 20)
    check_decode(w["ids"], w["scores"], w["ref"], w["plain"][0], 32, "wide")
    assert (w["ref"]["ids"] != w["plain"][0]).any(2).all() and (w["ref"]["ids"] == END).any(2).all()
    # without a penalty the norm is the score and the order the identity
    assert torch.equal(w["norm"], w["scores"]) and torch.equal(w["order"].cpu(), torch.arange(5, dtype=torch.int32).expand(32, 5))
    assert torch.equal(w["dec"].sample_beam(w["feats"].cuda(), beam_size=5, end_id=END, **w["kw"]), w["ids"][:, 0])


def test_narrow_constrained_decode_matches_the_cpu_restatement():
    """the narrow path, two LSTM layers: trigram blocking"""
    n = narrow_case()
    check_decode(n["ids"], n["scores"], n["ref"], n["plain"][0], 8, "narrow")


def test_every_returned_hypothesis_obeys_the_constraints():
    """wide case, every live hypothesis up to its <end>: no suppressed id, no <end> before position min_length, no bigram twice,
    no token twice in a row -- checked directly, not through the reference's banned sets"""
    w = wide_case()
    ids, scores = w["ids"].cpu().numpy(), w["scores"].cpu().numpy()
    checked = 0
    for b in range(ids.shape[0]):
        for k in range(ids.shape[1]):
            if not np.isfinite(scores[b, k]):
                continue
            row = ids[b, k].tolist()
            n = row.index(END) + 1 if END in row else len(row)
            row = row[:n]
            assert not set(row) & set(SUPPRESS), row
            assert END not in row[:MINLEN], row
            grams = list(zip(row, row[1:]))
            assert len(set(grams)) == len(grams), row
            assert all(a != b_ for a, b_ in grams), row
            checked += 1
    assert checked >= 150


def test_length_penalty_permutes_the_unpenalised_result():
    """length_penalty 0.7, then 2.0 (at 0.7 the reference re-orders no image of this case -- the lengths are 7 and 8 -- at 2.0 it
    re-orders most): ids and raw scores are the alpha = 0 result permuted by last_beam_order, the norms do not increase"""
    w = wide_case()
    dec = w["dec"]
    for alpha, reorders in ((0.7, False), (2.0, True)):
        ids, scores = dec.sample_beam(w["feats"].cuda(), beam_size=5, end_id=END, return_all=True, length_penalty=alpha, **w["kw"])
        order, norm = dec.last_beam_order.long(), dec.last_beam_norm_scores
        assert tuple(order.shape) == tuple(norm.shape) == (32, 5)
        assert torch.equal(torch.sort(order, 1)[0], torch.arange(5, device="cuda").expand(32, 5))
        assert torch.equal(ids, torch.gather(w["ids"], 1, order[:, :, None].expand(-1, -1, 20)))
        assert torch.equal(scores, torch.gather(w["scores"], 1, order))               # the raw sums, in the returned order
        assert (norm[:, :-1] >= norm[:, 1:]).all()
        ref = BC.rerank_ref(w["ids"].cpu().numpy(), w["scores"].cpu().numpy(), END, np.float32(alpha))
        rel = np.abs(norm.cpu().numpy() - ref["norm"]) / np.abs(ref["norm"])
        assert np.nanmax(rel) <= 1e-6
        moved = (ref["order"] != np.arange(5)).any(1)
        assert moved.any() == reorders and (not reorders or moved.sum() >= 8)         # (the reference's own statement of the case)
        rn = ref["norm"]
        clear = (np.abs(rn[:, :-1] - rn[:, 1:]) / np.abs(rn[:, :-1]) > 1e-5).all(1)
        assert clear.sum() >= 24 and np.array_equal(order.cpu().numpy()[clear], ref["order"][clear])
    # the penalty alone (no step constraint) re-orders the plain decode
    pid, psc = dec.sample_beam(w["feats"].cuda(), beam_size=5, end_id=END, return_all=True)
    assert dec.last_beam_order is None and dec.last_beam_norm_scores is None
    qid, qsc = dec.sample_beam(w["feats"].cuda(), beam_size=5, end_id=END, return_all=True, length_penalty=0.7)
    o = dec.last_beam_order.long()
    assert torch.equal(qid, torch.gather(pid, 1, o[:, :, None].expand(-1, -1, 20))) and torch.equal(qsc, torch.gather(psc, 1, o))


def test_beam_width_one_with_constraints_is_the_constrained_greedy_decode():
    n = narrow_case()
    ref = BC.decoder_beam(n["params"], n["feats"], 1, 2, END, n["c"])
    ids, sc = n["dec"].sample_beam(n["feats"].cuda(), beam_size=1, end_id=END, return_all=True, **n["kw"])
    keep = (ref["gap"] > GAP).numpy()
    assert (~keep).sum() * 4 <= 8 and ref["nbans"] > 0
    assert np.array_equal(ids.cpu().numpy()[keep], ref["ids"].numpy()[keep])
    assert np.abs(sc.cpu().numpy()[keep] - ref["scores"].numpy()[keep]).max() <= DECODE_ATOL


def test_defaults_are_the_calls_without_the_keywords():
    """every method with the new keywords at their off values returns tensors `torch.equal` to the call without them"""
    off = dict(suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0)
    n = narrow_case()
    dec, feats = n["dec"], n["feats"].cuda()
    a, b = dec.sample_beam(feats, 3, END, return_all=True), dec.sample_beam(feats, 3, END, return_all=True, **off)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and sat_beam_decode_ex with a NULL struct is sat_beam_decode
    lib = L.load()
    B, K, E, H, V = 8, 3, 32, 64, 203
    wsb = lib.sat_beam_decode_ex_ws_bytes(B, K, E, H, V, 2, 20)
    ws, ws_ptr = L.workspace256(wsb, feats.device)
    ids, sc = torch.empty(B, K, 20, dtype=torch.int64, device="cuda"), torch.empty(B, K, device="cuda")
    norm, order = torch.empty(B, K, device="cuda"), torch.empty(B, K, dtype=torch.int32, device="cuda")
    for s in (None, L.SatBeamConstraints()):
        L.check(lib.sat_beam_decode_ex(feats.data_ptr(), dec.embed.weight.data_ptr(), dec._lstm_ptrs(), 2, dec.linear.weight.data_ptr(),
                                       dec.linear.bias.data_ptr(), B, K, E, H, V, 20, END, s, ids.data_ptr(), sc.data_ptr(),
                                       norm.data_ptr(), order.data_ptr(), ws_ptr, wsb, L.stream()), "sat_beam_decode_ex")
        assert torch.equal(ids, a[0]) and torch.equal(sc, a[1]) and torch.equal(norm, a[1])
        assert torch.equal(order.cpu(), torch.arange(3, dtype=torch.int32).expand(8, 3))
    # ShowAndTell and validation_step
    arch = dict(layers=(1, 1, 1, 1), width=8)
    model = sat.ShowAndTell(32, 64, 203, 2, arch=arch, compute_dtype="f32").cuda().eval()
    model.decoder.load_state_dict(n["params"])
    images = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    assert torch.equal(model.sample_beam(images, 3, END), model.sample_beam(images, 3, END, **off))
    caps = torch.randint(4, 203, (4, 7), generator=torch.Generator().manual_seed(6)).cuda()
    ev = importlib.import_module("show-and-tell_amd.evaluate")
    v0 = ev.validation_step(model, images, caps, [7] * 4, beam_size=3)
    v1 = ev.validation_step(model, images, caps, [7] * 4, beam_size=3, **off)
    assert torch.equal(v0["ids"], v1["ids"]) and torch.equal(v0["kept"], v1["kept"])
    v2 = ev.validation_step(model, images, caps, [7] * 4, beam_size=3, suppress_ids=SUPPRESS, min_length=MINLEN, no_repeat_ngram_size=2)
    assert torch.equal(v2["ids"], model.sample_beam(images, 3, END, suppress_ids=SUPPRESS, min_length=MINLEN, no_repeat_ngram_size=2))
    assert not torch.isin(v2["ids"], torch.tensor(SUPPRESS, device="cuda")).any()


# ---- ShowAttendTellModel ----
@functools.lru_cache(maxsize=None)
def attend_case():
    from oracle import attend as OA
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G6_attend_small.npz"))
    hidden, context, vocab, embed, B, T, P, feat = [int(x) for x in z["dims"]]
    params = OA.init_attend_params(hidden, context, vocab, embed, generator=torch.Generator().manual_seed(int(z["seed"])), feat=feat)
    params["classifier.weight"] = params["classifier.weight"] * 8.0
    params["classifier.bias"] = params["classifier.bias"].clone()
    params["classifier.bias"][END] += 0.5
    model = sat.ShowAttendTellModel(hidden, context, vocab, embed, None, feature_size=(P, feat), compute_dtype="f32", vgg_cfg=[8, "M", feat])
    model.load_state_dict(params, strict=False)
    return model.cuda().eval(), params, torch.from_numpy(z["features"]), B, P


def test_attend_constrained_beam_matches_the_restatement_and_permutes_its_maps():
    from oracle import attend as OA
    model, params, feats, B, P = attend_case()
    K = 3
    c = BC.Constraints(SUPPRESS, MINLEN, 2, True)
    kw = dict(suppress_ids=SUPPRESS, min_length=MINLEN, no_repeat_ngram_size=2, block_repeat=True)
    ref = BC.attend_beam(params, feats, K, END, c)
    plain = OA.attend_beam_search(params, feats, K, None, end_id=END)
    ids, sc, al = model.sample_beam_features(feats.cuda(), K, None, END, return_all=True, return_alphas=True, **kw)
    check_decode(ids, sc, ref, plain[0], B, "attend")
    keep = (ref["gap"] > GAP).numpy()
    assert np.abs(al.cpu().numpy()[keep] - ref["alphas"].numpy()[keep]).max() <= 2e-5        # (test_gpu_alpha.py's tolerance for the maps)
    assert torch.equal(model.last_beam_order.cpu(), torch.arange(K, dtype=torch.int32).expand(B, K))
    assert torch.equal(model.last_beam_norm_scores, sc)
    # with a length penalty: ids, scores and maps are the alpha = 0 ones permuted by last_beam_order
    ids2, sc2, al2 = model.sample_beam_features(feats.cuda(), K, None, END, return_all=True, return_alphas=True, length_penalty=0.7, **kw)
    o = model.last_beam_order.long()
    assert torch.equal(torch.sort(o, 1)[0], torch.arange(K, device="cuda").expand(B, K))
    assert torch.equal(ids2, torch.gather(ids, 1, o[:, :, None].expand(-1, -1, 20))) and torch.equal(sc2, torch.gather(sc, 1, o))
    assert torch.equal(al2, torch.gather(al, 1, o[:, :, None, None].expand(-1, -1, 20, P)))
    norm = model.last_beam_norm_scores
    assert (norm[:, :-1] >= norm[:, 1:]).all()
    best_ids, best_al = model.sample_beam_features(feats.cuda(), K, None, END, return_alphas=True, length_penalty=0.7, **kw)
    assert torch.equal(best_ids, ids2[:, 0]) and torch.equal(best_al, al2[:, 0])


def test_attend_defaults_are_the_calls_without_the_keywords():
    off = dict(suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0)
    model, params, feats, B, P = attend_case()
    a = model.sample_beam_features(feats.cuda(), 3, None, END, return_all=True, return_alphas=True)
    b = model.sample_beam_features(feats.cuda(), 3, None, END, return_all=True, return_alphas=True, **off)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and model.last_beam_order is None
    images = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(7)).cuda()
    assert torch.equal(model.sample_beam(images, 2, None, END), model.sample_beam(images, 2, None, END, **off))
    with pytest.raises(ValueError, match="end_id"):
        model.sample_beam(images, 2, None, END, suppress_ids=[END])
