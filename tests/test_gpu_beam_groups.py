"""GPU: the diverse beam search -- sat_beam_step_groups (the row kernels + beam_merge_groups_kernel), sat_beam_decode_groups and the
`num_beam_groups` / `diversity_penalty` keywords -- against the plain references of tests/beam_groups_reference.py.

Step level, by the conventions of the constrained step tests.  Logits are a random background in [-1, 1) with plants 0.25 apart
from 2.0 up, the highest of every row on the SAME column so that the groups clash; bases are staggered per row.  A case is built
from the first seed at which the f64 reference's keys among each group's best Kg + 1 lie more than MARGIN = 1e-3 apart (asserted
before anything runs), so parents and tokens are compared exactly -- the surplus slots' too -- and scores to atol 1e-5.  Which row
path runs follows from (V, ldl): the register path for ldl % 4 == 0 and 4 <= V <= 12291, the long path otherwise.

Whole decode.  The f32 CPU restatement reports, per image, the smallest gap between consecutive keys among each group's best
Kg + 1 over all steps; ids are compared exactly and scores to 1e-4 on the images whose gap exceeds 2e-4, and at most a quarter of
the images may be left out.  Device and restatement are compared in SEARCH order (the device's result taken back through
`last_beam_order`); the final order is checked on the device's own scores."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import beam_constraints_reference as BC
import beam_groups_reference as BG

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
ARG, UNSUPPORTED = 1001, 1003
MARGIN, ATOL = 1e-3, 1e-5
GAP, DECODE_ATOL = 2e-4, 1e-4
STAGGER = 0.0917
LAM = 0.6                                   # no multiple of the plants' 0.25: a penalised plant never meets another one exactly
KG_PAIRS = [(2, 2), (4, 2), (6, 3), (8, 2), (8, 4), (8, 8)]


def pad4(n):
    return (n + 3) // 4 * 4


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def bases(B, K):
    return (-1.5 - 0.5 * np.arange(B, dtype=np.float32)[:, None] - np.float32(STAGGER) * np.arange(K, dtype=np.float32)[None, :])


def planted_rows(V, R, nplants, top, rng):
    """background + min(V, nplants) plants per row 0.25 apart, the row's HIGHEST on column `top`, the others on random columns"""
    x = rng.uniform(-1.0, 1.0, (R, V)).astype(np.float32)
    npl = min(V, nplants)
    for r in range(R):
        cols = [int(top)]
        for col in rng.permutation(V):
            if len(cols) >= npl:
                break
            if int(col) not in cols:
                cols.append(int(col))
        x[r, cols] = 2.0 + 0.25 * np.arange(npl - 1, -1, -1)
    return x


def device_step(x, ldl, scores, last, end_id, K, G=1, lam=0.0, entry="groups", c=None, parents=None, tokens=None, i=0, T=20, fill=0.0,
                expect=0):
    """one step on the device.  entry "groups": sat_beam_step_groups; "ex": sat_beam_step_ex; "plain": sat_beam_step.
    expect != 0: the call must return that code and leave the outputs' fill pattern alone"""
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
    ws = torch.empty(max(lib.sat_beam_step_ex_ws_bytes(B, min(K, 8), V, T), 64), dtype=torch.uint8, device="cuda")
    pr = None if parents is None else torch.from_numpy(np.ascontiguousarray(parents, dtype=np.int32)).cuda()
    tk = None if tokens is None else torch.from_numpy(np.ascontiguousarray(tokens, dtype=np.int64)).cuda()
    s = keep = None
    if c is not None:
        keep = torch.tensor(list(c.suppress_ids), dtype=torch.int64, device="cuda") if c.suppress_ids else None
        s = L.SatBeamConstraints(keep.data_ptr() if keep is not None else None, len(c.suppress_ids), c.min_length, c.no_repeat_ngram,
                                 int(c.block_repeat), c.length_penalty)
    if entry == "plain":
        rc = lib.sat_beam_step(logits.data_ptr(), ldl, sc.data_ptr(), L.ptr(lt), end_id, B, K, V, parent.data_ptr(), token.data_ptr(),
                               out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
    elif entry == "ex":
        rc = lib.sat_beam_step_ex(logits.data_ptr(), ldl, sc.data_ptr(), L.ptr(lt), end_id, B, K, V, s, L.ptr(pr), L.ptr(tk), i, T,
                                  parent.data_ptr(), token.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
    else:
        rc = lib.sat_beam_step_groups(logits.data_ptr(), ldl, sc.data_ptr(), L.ptr(lt), end_id, B, K, V, s, L.ptr(pr), L.ptr(tk), i, T, G,
                                      lam, parent.data_ptr(), token.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, (entry, rc, expect)
    if expect:
        assert (parent == -7).all() and (token == -7).all() and torch.isnan(out).all()
        return None
    return parent.cpu().numpy().astype(np.int64).reshape(B, K), token.cpu().numpy().reshape(B, K), out.cpu().numpy().reshape(B, K)


def build_case(make, limit=200):
    """the first seed at which `make(rng)` -> (inputs, ref) has every image's key gap above MARGIN; the search sees the f64
    reference only"""
    for seed in range(limit):
        inputs, ref = make(np.random.default_rng(seed))
        if (ref["gap"] > MARGIN).all():
            return inputs, ref
    raise AssertionError("no well-formed case below seed %d" % limit)


def check_exact(got, ref, tag):
    parent, token, out = got
    assert parent.tolist() == ref["parent"].tolist() and token.tolist() == ref["token"].tolist(), \
        (tag, parent.tolist(), token.tolist(), ref["parent"].tolist(), ref["token"].tolist())
    fin = np.isfinite(ref["scores"])
    assert np.array_equal(np.isneginf(out), ~fin), tag                 # surplus slots: -inf (parent g*Kg, token 0 compared above)
    err = np.abs(out[fin].astype(np.float64) - ref["scores"][fin]).max() if fin.any() else 0.0
    print("%s: score error %.3g (atol %.3g), smallest key gap %.3g, %d penalised winners" % (tag, err, ATOL, ref["gap"].min(), ref["npen"]))
    assert err <= ATOL, tag


# ---- step level ----
@pytest.mark.parametrize("V", [3, 203, 1000, 12292])
def test_grouped_step_over_shapes(V):
    """both row paths through (V, ldl): ldl = pad4(V) and, for the odd V, the unpadded odd ldl (the long path); B in {1, 2, 5};
    every row's arg-max on one column, so every group behind the first meets the penalty"""
    top = V - 1
    for (K, G), B in (((6, 3), 1), ((8, 4), 2), ((4, 2), 5), ((8, 8), 2)):
        def make(rng, K=K, G=G, B=B):
            x = planted_rows(V, B * K, K + 4, top, rng)
            sc = bases(B, K)
            return (x, sc), BG.step_ref(x, sc, None, -1, K, G, LAM)
        (x, sc), ref = build_case(make)
        plain = BG.step_ref(x, sc, None, -1, K, G, 0.0)
        assert (plain["token"] != ref["token"]).any(1).all()           # the penalty changed every image's winners
        for ldl in [pad4(V)] + ([V] if V % 2 else []):
            got = device_step(x, ldl, sc, None, -1, K, G, LAM, fill=0.0 if ldl == V else np.inf)
            check_exact(got, ref, "V%d ldl%d K%d G%d B%d" % (V, ldl, K, G, B))
            assert (got[0] // (K // G) == np.arange(K) // (K // G)).all()


@pytest.mark.parametrize("V", [203, 12292])
def test_depth_edge_of_the_lemma(V):
    """K 8, G 8, identical logits and bases in every row, lambda 10: group g must emit the row's (g + 1)-th best token, so group
    7's winner is the LAST entry of its row's top-8 list"""
    K = 8
    rng = np.random.default_rng(V)
    row = planted_rows(V, 1, K + 4, 5, rng)
    x = np.repeat(row, 2 * K, 0)
    sc = np.full((2, K), -0.75, dtype=np.float32)
    ranked = np.argsort(-row[0], kind="stable")
    ref = BG.step_ref(x, sc, None, -1, K, K, 10.0)
    assert (ref["gap"] > MARGIN).all() and ref["token"].tolist() == [ranked[:K].tolist()] * 2
    got = device_step(x, pad4(V), sc, None, -1, K, K, 10.0)
    check_exact(got, ref, "depth V%d" % V)
    assert got[1][:, 7].tolist() == [ranked[7]] * 2 and got[0].tolist() == [list(range(K))] * 2


def test_multiplicity_two_clashes_displace_what_one_does_not():
    """(K, G) = (6, 3): both slots of group 0 choose v; lambda 1.0 with v 1.5 ahead of w: 3 - 2 < 1.5 displaces v in group 1.  The
    control with one live row in group 0 (one clash on v, one on w): v stays"""
    K, G, V, v, w = 6, 3, 203, 77, 130
    rng = np.random.default_rng(1)
    row = rng.uniform(-1.0, 1.0, (1, V)).astype(np.float32)
    row[0, v], row[0, w] = 3.0, 1.5
    x = np.repeat(row, K, 0)
    sc = bases(1, K)
    two = BG.step_ref(x, sc, None, -1, K, G, 1.0)
    assert (two["gap"] > MARGIN).all() and two["token"][0, :2].tolist() == [v, v] and two["token"][0, 2] == w
    got = device_step(x, pad4(V), sc, None, -1, K, G, 1.0)
    check_exact(got, two, "two clashes")
    assert got[1][0, :3].tolist() == [v, v, w]
    sc1 = sc.copy()
    sc1[0, 1] = -np.inf
    one = BG.step_ref(x, sc1, None, -1, K, G, 1.0)
    assert (one["gap"] > MARGIN).all() and one["token"][0, :3].tolist() == [v, w, v] and one["npen"] > 0
    got = device_step(x, pad4(V), sc1, None, -1, K, G, 1.0)
    check_exact(got, one, "one clash")
    assert got[1][0, 2] == v


def test_tokens_of_one_group_do_not_penalise_each_other():
    """two rows of one group choose the same token unpenalised under lambda 1000; the group behind is driven off it"""
    K, G, V, v = 4, 2, 1000, 421

    def make(rng):
        x = planted_rows(V, 2 * K, K + 4, v, rng)
        sc = bases(2, K)
        return (x, sc), BG.step_ref(x, sc, None, -1, K, G, 1000.0)
    (x, sc), ref = build_case(make)
    assert ref["token"][:, :2].tolist() == [[v, v]] * 2 and ref["parent"][:, :2].tolist() == [[0, 1]] * 2
    got = device_step(x, pad4(V), sc, None, -1, K, G, 1000.0)
    check_exact(got, ref, "same group")
    assert (got[1][:, :2] == v).all() and (got[1][:, 2:] != v).all()
    assert np.array_equal(bits(got[2][:, :2]), bits(device_step(x, pad4(V), sc, None, -1, K, G, 0.0)[2][:, :2]))     # scores stay raw


def test_finished_dead_and_starved_rows():
    """end_id is every live row's arg-max.  Image 0: group 0 holds a finished and a live row, group 1 a finished row in front of a
    live one, group 2 a dead row and a row with ONE finite logit (a surplus slot).  Image 1: group 0 finished only -- nothing
    counts, group 1 takes end_id unpenalised -- and group 2 all dead"""
    K, G, V, end_id = 6, 3, 203, 2

    def make(rng):
        x = planted_rows(V, 2 * K, K + 4, end_id, rng)
        x[5, :] = -np.inf
        x[5, 9] = 0.5                                                  # image 0, slot 5: one candidate
        sc = bases(2, K)
        sc[0, 4] = -np.inf
        sc[1, 4:] = -np.inf
        sc[0, 2] = -0.25                                               # a finished row in front of its group
        last = np.full((2, K), 7, dtype=np.int64)
        last[0, 0] = last[0, 2] = last[1, 0] = last[1, 1] = end_id
        return (x, sc, last), BG.step_ref(x, sc, last, end_id, K, G, 1000.0)
    (x, sc, last), ref = build_case(make)
    got = device_step(x, pad4(V), sc, last, end_id, K, G, 1000.0, i=3)
    check_exact(got, ref, "finished-dead-starved")
    parent, token, out = got
    # image 0, group 0: the live row's end_id counts; group 1: the finished row's end_id is not penalised, bit for bit unchanged
    assert (parent[0, 2], token[0, 2]) == (2, end_id) and out[0, 2] == np.float32(-0.25)
    assert token[0, 3] != end_id                                       # the live row of group 1 is driven off end_id
    assert (parent[0, 4], token[0, 4]) == (5, 9) and (parent[0, 5], token[0, 5]) == (4, 0) and np.isneginf(out[0, 5])
    # image 1: finished rows do not count, so group 1's live rows take end_id freely; group 2 is all surplus
    assert token[1, :2].tolist() == [end_id, end_id] and np.array_equal(bits(out[1, :2]), bits(sc[1, :2]))
    assert token[1, 2] == end_id and parent[1, 4:].tolist() == [4, 4] and token[1, 4:].tolist() == [0, 0] and np.isneginf(out[1, 4:]).all()


def test_ties_in_the_key_resolve_by_lower_flat_index():
    """identical rows and bases inside a group: equal keys, the lower flat index k * V + v first"""
    K, G, V = 4, 2, 700
    rng = np.random.default_rng(2)
    row = planted_rows(V, 1, K + 4, 33, rng)
    x = np.repeat(row, K, 0)
    sc = np.array([[-1.0, -1.0, -1.25, -1.25]], dtype=np.float32)
    ranked = np.argsort(-row[0], kind="stable")
    ref = BG.step_ref(x, sc, None, -1, K, G, LAM)
    got = device_step(x, pad4(V), sc, None, -1, K, G, LAM)
    # group 0: the best token from row 0, then the same from row 1.  group 1: n(best) = 2, the second best from row 2, then row 3
    assert got[0].tolist() == [[0, 1, 2, 3]] == ref["parent"].tolist()
    assert got[1].tolist() == [[ranked[0], ranked[0], ranked[1], ranked[1]]] == ref["token"].tolist()
    assert got[2][0, 0] == got[2][0, 1] and got[2][0, 2] == got[2][0, 3]
    assert np.abs(got[2] - ref["scores"]).max() <= ATOL


@pytest.mark.parametrize("V,ldl", [(1000, 1000), (203, 203), (12292, 12292)])
def test_lambda_zero_is_the_plain_step_on_every_group_alone(V, ldl):
    """lambda = 0 with G > 1: every group is bit for bit sat_beam_step on that group's Kg rows alone, parents offset by g * Kg"""
    end_id = 2
    for K, G in KG_PAIRS:
        B, Kg = 2, K // G
        rng = np.random.default_rng([V, K, G])
        x = np.clip(rng.normal(0.0, 2.0, (B * K, V)), -8, 8).astype(np.float32)
        sc = bases(B, K)
        sc[1, K - 1] = -np.inf
        last = rng.integers(3, V, (B, K)).astype(np.int64)
        last[0, 0] = end_id
        got = device_step(x, ldl, sc, last, end_id, K, G, 0.0, i=2)
        want = device_step(x, ldl, sc.reshape(B * G, Kg), last.reshape(B * G, Kg), end_id, Kg, entry="plain")
        offset = (np.arange(B * G) % G * Kg)[:, None]
        assert np.array_equal(got[0].reshape(B * G, Kg), want[0] + offset), (K, G)
        assert np.array_equal(got[1].reshape(B * G, Kg), want[1]) and np.array_equal(bits(got[2].reshape(B * G, Kg)), bits(want[2])), (K, G)


def test_one_group_is_sat_beam_step_ex_bit_for_bit():
    """G = 1, with and without constraints; lambda is not read (NaN passes)"""
    T, B, K, V, i, end_id = 20, 2, 5, 700, 2, 2
    rng = np.random.default_rng(7)
    x = np.clip(rng.normal(0.0, 2.0, (B * K, V)), -8, 8).astype(np.float32)
    sc = bases(B, K)
    sc[1, 4] = -np.inf
    parents = rng.integers(0, K, (T, B * K)).astype(np.int32)
    tokens = rng.integers(0, 40, (T, B * K)).astype(np.int64)
    last = tokens[i - 1].copy()
    last[3] = end_id
    for c in (None, BC.Constraints(suppress_ids=[5, 9], min_length=4, no_repeat_ngram=1, block_repeat=True)):
        want = device_step(x, V, sc, last, end_id, K, entry="ex", c=c, parents=parents, tokens=tokens, i=i, T=T)
        for lam in (0.0, float("nan")):
            got = device_step(x, V, sc, last, end_id, K, 1, lam, c=c, parents=parents, tokens=tokens, i=i, T=T)
            assert all(np.array_equal(bits(a), bits(w)) for a, w in zip(got, want))


@pytest.mark.parametrize("K,G", KG_PAIRS)
def test_parents_stay_in_their_group_and_a_huge_penalty_separates_the_groups(K, G):
    """random logits, every row live, constraints on: every parent lies in its slot's group; with lambda 1000 the tokens of
    different groups are disjoint; group 0 is the lambda = 0 group 0 bit for bit"""
    B, V, Kg, T, i = 5, 1000, K // G, 20, 3
    rng = np.random.default_rng([K, G])
    x = np.clip(rng.normal(0.0, 2.0, (B * K, V)), -8, 8).astype(np.float32)
    x[:, 17] += 6.0                                                    # one token every row wants
    sc = bases(B, K)
    parents = np.tile(np.arange(K, dtype=np.int32), (T, B))
    tokens = rng.integers(0, V, (T, B * K)).astype(np.int64)
    c = BC.Constraints(suppress_ids=[4], block_repeat=True)
    base = device_step(x, V, sc, tokens[i - 1], -1, K, G, 0.0, c=c, parents=parents, tokens=tokens, i=i, T=T)
    for lam in (0.5, 1000.0):
        parent, token, out = device_step(x, V, sc, tokens[i - 1], -1, K, G, lam, c=c, parents=parents, tokens=tokens, i=i, T=T)
        assert (parent // Kg == np.arange(K) // Kg).all() and np.isfinite(out).all()
        assert all(np.array_equal(bits(a[:, :Kg]), bits(w[:, :Kg])) for a, w in zip((parent, token, out), base))
        assert (token != 4).all() and (token != tokens[i - 1].reshape(B, K)[np.arange(B)[:, None], parent]).all()
    for b in range(B):
        seen = [set(token[b, g * Kg:(g + 1) * Kg].tolist()) for g in range(G)]
        assert all(not (seen[g] & seen[h]) for g in range(G) for h in range(g)), (b, token[b].tolist())


def test_argument_errors_leave_the_outputs_alone():
    K, V = 6, 203
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (2 * K, V)).astype(np.float32)
    sc, last = bases(2, K), np.full((2, K), 7, dtype=np.int64)
    for G in (0, -1, 4, 12):
        device_step(x, V, sc, last, 2, K, G, 0.5, i=1, expect=ARG)
    for lam in (-0.5, float("nan"), float("inf")):
        device_step(x, V, sc, last, 2, K, 3, lam, i=1, expect=ARG)
    device_step(x, V, sc, None, 2, K, 3, 0.5, i=1, expect=ARG)         # G > 1, an end_id, i > 0: the last tokens are needed
    assert device_step(x, V, sc, None, 2, K, 3, 0.5, i=0) is not None  # ... not at step 0
    assert device_step(x, V, sc, None, -1, K, 3, 0.5, i=1) is not None  # ... and not without an end_id
    x9 = rng.uniform(-1, 1, (9, V)).astype(np.float32)
    device_step(x9, V, bases(1, 9), None, -1, 9, 3, 0.5, expect=UNSUPPORTED)
    device_step(x, V, sc, last, 2, K, 3, 0.5, i=1, c=BC.Constraints(min_length=-1), expect=ARG)


# ---- whole decode ----
END, SUPPRESS, MINLEN = 2, [3, 0, 1], 6


def search_order(ids, scores, order):
    """the public (re-ranked) result taken back to search order: slot order[b, r] held what is now at rank r"""
    o = order.long()
    ids_s, sc_s = torch.empty_like(ids), torch.empty_like(scores)
    ids_s.scatter_(1, o[:, :, None].expand_as(ids), ids)
    sc_s.scatter_(1, o, scores)
    return ids_s, sc_s


@functools.lru_cache(maxsize=None)
def decoder_case(E, H, V, B, K, G, lam, Lh, seed, scale, n=0, block=False, constrained=False):
    from oracle import decoder as OD
    gen = torch.Generator().manual_seed(seed)
    params = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    params["linear.weight"] = params["linear.weight"] * scale
    params["linear.bias"][END] = 1.0                                # so that <end> occurs
    feats = torch.randn(B, E, generator=gen)
    c = BC.Constraints(SUPPRESS if constrained else (), MINLEN if constrained else 0, n, block)
    kw = dict(no_repeat_ngram_size=n, block_repeat=block)
    if constrained:
        kw.update(suppress_ids=SUPPRESS, min_length=MINLEN)
    ref = BG.decoder_beam(params, feats, K, G, lam, Lh, END, c)
    ref0 = BG.decoder_beam(params, feats, K, G, 0.0, Lh, END, c)
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    dec.cuda().eval()
    return dict(dec=dec, params=params, feats=feats, c=c, kw=kw, ref=ref, ref0=ref0, K=K, G=G, lam=lam, B=B)


def run_grouped(w, lam=None, **extra):
    kw = dict(w["kw"], num_beam_groups=w["G"], diversity_penalty=w["lam"] if lam is None else lam, **extra)
    ids, scores = w["dec"].sample_beam(w["feats"].cuda(), beam_size=w["K"], end_id=END, return_all=True, **kw)
    dec = w["dec"]
    return ids, scores, dec.last_beam_order, dec.last_beam_norm_scores, dec.last_beam_groups


def check_final_order(ids, scores, order, norm, groups, K, G):
    """order is a permutation of the slots, sorted by (score desc, search slot asc) at length_penalty 0; groups = order // Kg"""
    B = ids.shape[0]
    assert torch.equal(torch.sort(order.long(), 1)[0], torch.arange(K, device="cuda").expand(B, K))
    assert groups.dtype == torch.int32 and torch.equal(groups, order // (K // G))
    assert torch.equal(norm, scores) and (scores[:, :-1] >= scores[:, 1:]).all()
    _, sc_s = search_order(ids, scores, order)
    assert torch.equal(order.long(), torch.sort(sc_s, dim=1, descending=True, stable=True)[1])


def check_decode(w, left_out, tag):
    ref, ref0, B, K, G = w["ref"], w["ref0"], w["B"], w["K"], w["G"]
    keep = (ref["gap"] > GAP).numpy()
    print("%s: %d of %d images left out (gap <= %.0e); smallest kept gap %.3g; %d penalised winners, %d bans" %
          (tag, int((~keep).sum()), B, GAP, float(ref["gap"][torch.from_numpy(keep)].min()), ref["npen"], ref["nbans"]))
    assert int((~keep).sum()) == left_out and left_out * 4 <= B     # what the case was chosen for; at most a quarter left out
    assert ref["npen"] > 0 and (ref["ids"] != ref0["ids"]).any(2).any(1).all()      # the penalty fired and changed every image
    ids, scores, order, norm, groups = run_grouped(w)
    assert tuple(ids.shape) == (B, K, 20)
    check_final_order(ids, scores, order, norm, groups, K, G)
    ids_s, sc_s = search_order(ids, scores, order)
    ids_s, sc_s = ids_s.cpu().numpy(), sc_s.cpu().numpy()
    assert np.array_equal(ids_s[keep], ref["ids"].numpy()[keep])
    fin = np.isfinite(ref["scores"].numpy()[keep])
    assert np.array_equal(np.isfinite(sc_s[keep]), fin)
    err = np.abs(sc_s[keep][fin] - ref["scores"].numpy()[keep][fin]).max()
    print("%s: score error %.3g (atol %.0e)" % (tag, err, DECODE_ATOL))
    assert err <= DECODE_ATOL
    return ids, scores, order, keep


def wide63():
    return decoder_case(64, 256, 1000, 32, 6, 3, 0.5, 1, 99, 20.0)


def test_wide_grouped_decode_matches_the_cpu_restatement():
    """the wide path (192 rows, one layer, the projection on the bf16 pipe), three groups of two"""
    check_decode(wide63(), 1, "wide 6/3")


def test_wide_grouped_constrained_decode_matches_the_cpu_restatement():
    """... under three suppressed ids, <end> not before position 6, bigram blocking and no immediate repeat"""
    w = decoder_case(64, 256, 1000, 32, 6, 3, 0.5, 1, 99, 20.0, 2, True, True)
    ids, scores, _, _ = check_decode(w, 0, "wide 6/3 constrained")
    live = torch.isfinite(scores).cpu().numpy()
    assert BC.check_properties(ids.cpu().numpy()[live][:, None, :], END, w["c"]) >= 150


def test_wide_eight_groups_of_one_match_the_cpu_restatement():
    check_decode(decoder_case(64, 256, 1000, 32, 8, 8, 1.0, 1, 99, 20.0), 4, "wide 8/8")


def test_narrow_grouped_decode_matches_the_cpu_restatement():
    """the narrow path, two LSTM layers, two groups of two"""
    check_decode(decoder_case(32, 64, 203, 8, 4, 2, 0.5, 2, 11, 40.0), 1, "narrow 4/2")


def test_narrow_grouped_decode_with_trigram_blocking_matches_the_cpu_restatement():
    check_decode(decoder_case(32, 64, 203, 8, 4, 2, 0.5, 2, 11, 40.0, 3), 0, "narrow 4/2 trigram")


def test_grouped_decode_properties():
    """no tolerance: a huge penalty separates the groups at every step; group 0 does not depend on lambda; without return_all the
    result is row 0; the order and group records are consistent"""
    w = wide63()
    K, G, Kg, B = 6, 3, 2, 32
    keep = torch.from_numpy((w["ref"]["gap"] > GAP).numpy()).cuda()
    ids0, sc0, order0, _, _ = run_grouped(w, 0.0)
    s_ids0, s_sc0 = search_order(ids0, sc0, order0)
    for lam in (0.5, 1000.0):
        ids, sc, order, norm, groups = run_grouped(w, lam)
        check_final_order(ids, sc, order, norm, groups, K, G)
        s_ids, s_sc = search_order(ids, sc, order)
        assert torch.equal(s_ids[keep][:, :Kg], s_ids0[keep][:, :Kg]) and torch.equal(s_sc[keep][:, :Kg], s_sc0[keep][:, :Kg])
        best = w["dec"].sample_beam(w["feats"].cuda(), beam_size=K, end_id=END, num_beam_groups=G, diversity_penalty=lam)
        assert torch.equal(best, ids[:, 0])
    # lambda 1000: at every step the tokens of live, unfinished slots of different groups are disjoint.  The final hypotheses
    # never left their groups, so at step t they sat in distinct live slots of their groups
    s_ids, s_sc = s_ids.cpu().numpy(), s_sc.cpu().numpy()
    checked = 0
    for b in range(B):
        for t in range(20):
            seen = []
            for g in range(G):
                toks = set()
                for k in range(g * Kg, (g + 1) * Kg):
                    if np.isfinite(s_sc[b, k]) and END not in s_ids[b, k, :t].tolist():
                        toks.add(int(s_ids[b, k, t]))
                assert all(not (toks & other) for other in seen), (b, t)
                seen.append(toks)
                checked += len(toks)
    assert checked >= 2 * B * G                                       # every group of every image, at steps 0 and 1 at least
    assert BG.distinct_captions(s_ids, s_sc, END) > BG.distinct_captions(s_ids0.cpu().numpy(), s_sc0.cpu().numpy(), END)


def test_defaults_are_the_calls_without_the_keywords_and_validation_step_follows_sample_beam():
    off = dict(num_beam_groups=1, diversity_penalty=0.0)
    w = decoder_case(32, 64, 203, 8, 4, 2, 0.5, 2, 11, 40.0)
    dec, feats = w["dec"], w["feats"].cuda()
    run_grouped(w)
    assert dec.last_beam_groups is not None
    a, b = dec.sample_beam(feats, 4, END, return_all=True), dec.sample_beam(feats, 4, END, return_all=True, **off)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and dec.last_beam_groups is None and dec.last_beam_order is None
    cons = dict(suppress_ids=SUPPRESS, min_length=MINLEN, no_repeat_ngram_size=2, length_penalty=0.7)
    a, b = dec.sample_beam(feats, 4, END, return_all=True, **cons), dec.sample_beam(feats, 4, END, return_all=True, **cons, **off)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and dec.last_beam_groups is None and dec.last_beam_order is not None
    # sat_beam_decode_groups with one group is sat_beam_decode_ex
    lib = L.load()
    B, K, E, H, V = 8, 4, 32, 64, 203
    wsb = lib.sat_beam_decode_groups_ws_bytes(B, K, E, H, V, 2, 20)
    ws, ws_ptr = L.workspace256(wsb, feats.device)
    plain = dec.sample_beam(feats, 4, END, return_all=True)
    ids, sc = torch.empty(B, K, 20, dtype=torch.int64, device="cuda"), torch.empty(B, K, device="cuda")
    L.check(lib.sat_beam_decode_groups(feats.data_ptr(), dec.embed.weight.data_ptr(), dec._lstm_ptrs(), 2, dec.linear.weight.data_ptr(),
                                       dec.linear.bias.data_ptr(), B, K, E, H, V, 20, END, None, 1, float("nan"), ids.data_ptr(),
                                       sc.data_ptr(), None, None, ws_ptr, wsb, L.stream()), "sat_beam_decode_groups")
    assert torch.equal(ids, plain[0]) and torch.equal(sc, plain[1])
    # ShowAndTell and validation_step
    arch = dict(layers=(1, 1, 1, 1), width=8)
    model = sat.ShowAndTell(32, 64, 203, 2, arch=arch, compute_dtype="f32").cuda().eval()
    model.decoder.load_state_dict(w["params"])
    images = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    assert torch.equal(model.sample_beam(images, 4, END), model.sample_beam(images, 4, END, **off)) and model.last_beam_groups is None
    grouped = model.sample_beam(images, 4, END, return_all=True, num_beam_groups=2, diversity_penalty=0.5)
    assert torch.equal(model.last_beam_groups, model.last_beam_order // 2) and tuple(grouped[0].shape) == (4, 4, 20)
    caps = torch.randint(4, 203, (4, 7), generator=torch.Generator().manual_seed(6)).cuda()
    ev = importlib.import_module("show-and-tell_amd.evaluate")
    v0 = ev.validation_step(model, images, caps, [7] * 4, beam_size=4)
    v1 = ev.validation_step(model, images, caps, [7] * 4, beam_size=4, **off)
    assert torch.equal(v0["ids"], v1["ids"]) and torch.equal(v0["kept"], v1["kept"])
    v2 = ev.validation_step(model, images, caps, [7] * 4, beam_size=4, num_beam_groups=2, diversity_penalty=0.5)
    assert torch.equal(v2["ids"], model.sample_beam(images, beam_size=4, end_id=END, num_beam_groups=2, diversity_penalty=0.5))
    assert torch.equal(v2["ids"], grouped[0][:, 0])


# ---- ShowAttendTellModel ----
@functools.lru_cache(maxsize=None)
def attend_case():
    """the G6 dimensions and features, K 4, G 2, lambda 0.5: the first parameter seed at which the restatement leaves out at most a
    quarter of the images (the search sees the restatement only)"""
    from oracle import attend as OA
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G6_attend_small.npz"))
    hidden, context, vocab, embed, B, T, P, feat = [int(x) for x in z["dims"]]
    feats = torch.from_numpy(z["features"])
    for seed in range(20):
        params = OA.init_attend_params(hidden, context, vocab, embed, generator=torch.Generator().manual_seed(seed), feat=feat)
        params["classifier.weight"] = params["classifier.weight"] * 8.0
        params["classifier.bias"] = params["classifier.bias"].clone()
        params["classifier.bias"][END] += 0.5
        ref = BG.attend_beam(params, feats, 4, 2, 0.5, END)
        if int((ref["gap"] <= GAP).sum()) * 4 <= B and ref["npen"] > 0:
            break
    else:
        raise AssertionError("no seed below 20 leaves out at most a quarter")
    model = sat.ShowAttendTellModel(hidden, context, vocab, embed, None, feature_size=(P, feat), compute_dtype="f32", vgg_cfg=[8, "M", feat])
    model.load_state_dict(params, strict=False)
    return model.cuda().eval(), params, feats, B, P, ref


def test_attend_grouped_beam_matches_the_restatement_and_permutes_its_maps():
    model, params, feats, B, P, ref = attend_case()
    K, G = 4, 2
    keep = (ref["gap"] > GAP).numpy()
    ref0 = BG.attend_beam(params, feats, K, G, 0.0, END)
    assert (~keep).sum() * 4 <= B and ref["npen"] > 0 and (ref["ids"] != ref0["ids"]).any()
    kw = dict(num_beam_groups=G, diversity_penalty=0.5)
    ids, sc, al = model.sample_beam_features(feats.cuda(), K, None, END, return_all=True, return_alphas=True, **kw)
    order, norm, groups = model.last_beam_order, model.last_beam_norm_scores, model.last_beam_groups
    check_final_order(ids, sc, order, norm, groups, K, G)
    ids_s, sc_s = search_order(ids, sc, order)
    al_s = torch.empty_like(al)
    al_s.scatter_(1, order.long()[:, :, None, None].expand_as(al), al)
    assert np.array_equal(ids_s.cpu().numpy()[keep], ref["ids"].numpy()[keep])
    fin = np.isfinite(ref["scores"].numpy()[keep])
    err = np.abs(sc_s.cpu().numpy()[keep][fin] - ref["scores"].numpy()[keep][fin]).max()
    print("attend 4/2: %d of %d left out, score error %.3g (atol %.0e), %d penalised winners" % ((~keep).sum(), B, err, DECODE_ATOL, ref["npen"]))
    assert err <= DECODE_ATOL
    live = np.isfinite(ref["scores"].numpy())[keep]
    assert np.abs(al_s.cpu().numpy()[keep][live] - ref["alphas"].numpy()[keep][live]).max() <= 2e-5     # (test_gpu_alpha.py's tolerance)
    # the returned maps are the search-order maps permuted by last_beam_order: a length penalty re-orders ids, scores and maps alike
    ids2, sc2, al2 = model.sample_beam_features(feats.cuda(), K, None, END, return_all=True, return_alphas=True, length_penalty=2.0, **kw)
    o2 = model.last_beam_order.long()
    assert torch.equal(model.last_beam_groups, model.last_beam_order // (K // G))
    assert torch.equal(ids2, torch.gather(ids_s, 1, o2[:, :, None].expand(-1, -1, 20))) and torch.equal(sc2, torch.gather(sc_s, 1, o2))
    assert torch.equal(al2, torch.gather(al_s, 1, o2[:, :, None, None].expand(-1, -1, 20, P)))
    n2 = model.last_beam_norm_scores
    assert (n2[:, :-1] >= n2[:, 1:]).all()
    best_ids, best_al = model.sample_beam_features(feats.cuda(), K, None, END, return_alphas=True, **kw)
    assert torch.equal(best_ids, ids[:, 0]) and torch.equal(best_al, al[:, 0])


def test_attend_defaults_are_the_calls_without_the_keywords():
    off = dict(num_beam_groups=1, diversity_penalty=0.0)
    model, params, feats, B, P, _ = attend_case()
    model.sample_beam_features(feats.cuda(), 4, None, END, num_beam_groups=2)
    assert model.last_beam_groups is not None
    a = model.sample_beam_features(feats.cuda(), 4, None, END, return_all=True, return_alphas=True)
    b = model.sample_beam_features(feats.cuda(), 4, None, END, return_all=True, return_alphas=True, **off)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and model.last_beam_groups is None and model.last_beam_order is None
    images = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(7)).cuda()
    assert torch.equal(model.sample_beam(images, 2, None, END), model.sample_beam(images, 2, None, END, **off))
    ids = model.sample_beam(images, 4, None, END, return_all=True, num_beam_groups=2, diversity_penalty=0.5)[0]
    assert tuple(ids.shape) == (2, 4, 20) and torch.equal(model.last_beam_groups, model.last_beam_order // 2)
