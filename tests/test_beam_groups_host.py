"""CPU: the diverse beam search's host side -- the f64 reference of tests/beam_groups_reference.py on hand-made rows, the lemma
that lets the selection kernel work from the row kernels' top-K lists (by brute force), the four new symbols in the header, the
built library and the ctypes table, the two keywords on every public method, the Python refusals, and the argument errors the
library returns before it touches a device."""
import ctypes as C
import importlib
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import beam_groups_reference as BG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
M = importlib.import_module("show-and-tell_amd.models")

ARG, WORKSPACE, UNSUPPORTED = 1001, 1002, 1003
NEW = ("sat_beam_step_groups", "sat_beam_step_groups_ws_bytes", "sat_beam_decode_groups_ws_bytes", "sat_beam_decode_groups")
NINF = -np.inf


def uniform_rows(K, V, best):
    """logits whose log-softmax is easy by hand: every row zero except the columns of `best`: {v: logit}"""
    x = np.zeros((K, V))
    for v, val in best.items():
        x[:, v] = val
    return x


# ---- the reference on hand-made rows ----
def test_reference_multiplicity_two():
    """(K, G) = (6, 3) from the start scores: group 0's live row picks 7 then 3; group 1 pays lambda for 7 and for 3; group 2 pays for
    what groups 0 and 1 chose, twice for 7.  Then two live rows of group 0 that both choose 7, and the control with one"""
    K, G, V = 6, 3, 10
    x = uniform_rows(K, V, {7: 3.0, 3: 2.0, 5: 1.0, 1: 0.5})
    scores = BG.group_start(1, K, G, torch.float64).numpy()
    r = BG.step_ref(x, scores, None, -1, K, G, 1.25)
    # group 0: 7, 3 unpenalised.  group 1: 7 -> 3 - 1.25 = 1.75, 3 -> 0.75, 5 -> 1.0, 1 -> 0.5: winners 7 (penalised), 5
    # group 2: n(7) = 2 -> 0.5, n(3) = 1 -> 0.75, n(5) = 1 -> -0.25, 1 -> 0.5 ahead of 7 by index: winners 3, 1
    assert r["token"].tolist() == [[7, 3, 7, 5, 3, 1]] and r["parent"].tolist() == [[0, 0, 2, 2, 4, 4]]
    assert r["npen"] == 2 and r["counted"] == [[7, 3, 7, 5, 3, 1]]
    lse = math.log(V - 4 + math.exp(3.0) + math.exp(2.0) + math.exp(1.0) + math.exp(0.5))
    np.testing.assert_allclose(r["scores"][0], np.array([3.0, 2.0, 3.0, 1.0, 2.0, 0.5]) - lse, atol=1e-12)      # raw, not the key
    # two clashes displace what one does not: rows 0 and 1 of group 0 BOTH live, both choose 7 (staggered bases, ties aside)
    scores = np.array([[0.0, -0.01, 0.0, NINF, NINF, NINF]])
    x = uniform_rows(K, V, {7: 3.0, 5: 1.5})
    two = BG.step_ref(x, scores, None, -1, K, 3, 1.0)
    assert two["token"][0, :2].tolist() == [7, 7] and two["counted"][0][:2] == [7, 7]
    assert two["token"][0, 2] == 5                                    # 3 - 2 * 1.0 < 1.5
    scores[0, 1] = NINF                                               # the control: one clash, 3 - 1.0 > 1.5, 7 stays
    one = BG.step_ref(x, scores, None, -1, K, 3, 1.0)
    assert one["token"][0, 0] == 7 and one["token"][0, 2] == 7 and one["npen"] >= 1


def test_reference_finished_rows_are_exempt_and_uncounted():
    K, G, V, end_id = 4, 2, 8, 2
    x = uniform_rows(K, V, {2: 4.0, 6: 1.0})                          # <end> is every live row's arg-max
    scores = np.array([[-1.0, -3.0, -0.5, -2.0]])
    last = np.array([[2, 5, 2, 5]])                                   # slots 0 and 2 are finished
    r = BG.step_ref(x, scores, last, end_id, K, G, 100.0)
    # group 0: the finished row's end_id at -1.0 (uncounted), then the live row's end_id (counts).  group 1: the finished row's
    # end_id is NOT penalised although group 0's live row chose end_id; the live row's end_id is, and it falls behind 6
    assert r["token"].tolist() == [[2, 2, 2, 6]] and r["parent"].tolist() == [[0, 1, 2, 3]]
    assert r["scores"][0, 0] == -1.0 and r["scores"][0, 2] == -0.5
    assert r["counted"] == [[2, 6]] and r["npen"] == 0
    # nothing counts from finished rows alone: with group 0 all finished, group 1 chooses end_id freely
    last = np.array([[2, 2, 5, 5]])
    r = BG.step_ref(x, scores, last, end_id, K, G, 100.0)
    assert r["token"][0, 2] == 2 and r["counted"][0][0] == 2 and len(r["counted"][0]) == 2


def test_reference_surplus_slots_and_dead_rows():
    K, G, V = 6, 3, 3
    x = uniform_rows(K, V, {0: 1.0})
    x[2:4, 1:] = NINF                                                 # group 1's rows have ONE finite logit each
    scores = np.array([[0.0, NINF, -1.0, NINF, NINF, NINF]])          # group 1: one live row -> one candidate; group 2: all dead
    r = BG.step_ref(x, scores, None, -1, K, G, 0.5)
    assert r["live"].tolist() == [[2, 1, 0]]
    assert r["parent"].tolist() == [[0, 0, 2, 2, 4, 4]] and r["token"][0, 3:].tolist() == [0, 0, 0]
    assert np.isneginf(r["scores"][0, 3:]).all() and r["scores"][0, 2] == -1.0
    assert r["counted"] == [[0, 1, 0]]                                # (row 0: token 0, then 1 in front of 2 by index)
    assert r["npen"] == 1                                             # group 1's only candidate is token 0, which group 0 chose


def test_reference_groups_of_one_are_the_plain_step():
    import beam_reference as R
    rng = np.random.default_rng(0)
    x = rng.normal(0, 2, (2 * 5, 40))
    scores = -rng.uniform(0, 3, (2, 5))
    scores[1, 3] = NINF
    plain, one = R.beam_step_ref(x, scores, None, -1, 5), BG.step_ref(x, scores, None, -1, 5, 1, 0.0)
    assert np.array_equal(plain["parent"], one["parent"]) and np.array_equal(plain["token"], one["token"])
    assert np.array_equal(plain["scores"], one["scores"])


# ---- the lemma, by brute force ----
def select_from_row_lists(cand, finished, G, lam):
    """the selection as the device runs it: every row reduced to its K best raw candidates under (s desc, index asc) first"""
    K, V = cand.shape
    short = np.full_like(cand, NINF)
    for k in range(K):
        keep = np.argsort(-cand[k], kind="stable")[:K]
        short[k, keep] = cand[k, keep]
    return BG.select_groups(short, finished, G, lam)


@pytest.mark.parametrize("K", range(1, 9))
def test_lemma_row_top_k_lists_are_deep_enough(K):
    """selection over the full K * V candidates == selection over per-row raw top-K lists: every divisor G of K, logits drawn from a
    handful of values (many exact duplicates, so the index tie rule is exercised), finished and dead rows, lambda from 0 to huge"""
    rng = np.random.default_rng(K)
    for G in [g for g in range(1, K + 1) if K % g == 0]:
        penalised = 0
        for trial in range(30):
            V = int(rng.integers(K, 24))
            cand = rng.choice(np.arange(-6.0, 0.0, 0.5), (K, V)) + rng.choice([0.0, -0.5, -1.0], (K, 1))
            finished = rng.random(K) < 0.15
            for k in range(K):
                if finished[k]:
                    only = cand[k, 2 % V]
                    cand[k] = NINF
                    cand[k, 2 % V] = only
                elif rng.random() < 0.1:
                    cand[k] = NINF
                elif rng.random() < 0.3:
                    cand[k, rng.random(V) < 0.5] = NINF
            lam = float(rng.choice([0.0, 0.25, 0.5, 1.0, 10.0, 1000.0]))
            full, short = BG.select_groups(cand, finished, G, lam), select_from_row_lists(cand, finished, G, lam)
            assert np.array_equal(full["parent"], short["parent"]) and np.array_equal(full["token"], short["token"]), (K, G, trial)
            assert np.array_equal(full["scores"], short["scores"])
            Kg = K // G
            for slot in range(K):                                     # a hypothesis never leaves its group
                assert full["parent"][slot] // Kg == slot // Kg
            penalised += full["npen"]
        assert G == 1 or penalised > 0, (K, G)


# ---- the interface ----
def test_new_symbols_are_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name), name
    assert lib.sat_version() == L.ABI_VERSION == 18
    assert len(L.SIGNATURES["sat_beam_step_groups"][1]) == len(L.SIGNATURES["sat_beam_step_ex"][1]) + 2
    assert len(L.SIGNATURES["sat_beam_decode_groups"][1]) == len(L.SIGNATURES["sat_beam_decode_ex"][1]) + 2
    assert lib.sat_beam_step_groups_ws_bytes(4, 6, 1000, 20) == lib.sat_beam_step_ex_ws_bytes(4, 6, 1000, 20) > 0
    assert lib.sat_beam_decode_groups_ws_bytes(4, 6, 32, 64, 203, 2, 20) == lib.sat_beam_decode_ex_ws_bytes(4, 6, 32, 64, 203, 2, 20) > 0
    assert lib.sat_beam_decode_groups_ws_bytes(4, 9, 32, 64, 203, 2, 20) == 0


@pytest.mark.parametrize("owner,method", [("DecoderRNN", "sample_beam"), ("ShowAndTell", "sample_beam"),
                                          ("ShowAttendTellModel", "sample_beam_features"), ("ShowAttendTellModel", "sample_beam"),
                                          (None, "validation_step")])
def test_every_method_takes_the_two_keywords(owner, method):
    fn = getattr(getattr(sat, owner), method) if owner else importlib.import_module("show-and-tell_amd.evaluate").validation_step
    p = inspect.signature(fn).parameters
    for name, default in (("num_beam_groups", 1), ("diversity_penalty", 0.0)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, (method, name)
    if owner:
        assert getattr(sat, owner).last_beam_groups is None


def test_validator_accepts_and_refuses():
    assert M.check_beam_groups(5) == (1, 0.0) and M.check_beam_groups(6, 3, 0.5) == (3, 0.5)
    assert M.check_beam_groups(8, 8, 0) == (8, 0.0) and M.check_beam_groups(6, 2, 0.1) == (2, float(np.float32(0.1)))
    for kw, match in ((dict(beam_size=6, num_beam_groups=4), "divisible"), (dict(beam_size=4, num_beam_groups=8), "divisible"),
                      (dict(beam_size=4, num_beam_groups=0), "num_beam_groups"), (dict(beam_size=4, num_beam_groups=2.0), "num_beam_groups"),
                      (dict(beam_size=4, num_beam_groups=True), "num_beam_groups"),
                      (dict(beam_size=4, num_beam_groups=2, diversity_penalty=-0.5), "diversity_penalty"),
                      (dict(beam_size=4, num_beam_groups=2, diversity_penalty=float("nan")), "diversity_penalty"),
                      (dict(beam_size=4, num_beam_groups=2, diversity_penalty=float("inf")), "diversity_penalty"),
                      (dict(beam_size=4, num_beam_groups=2, diversity_penalty=1e39), "diversity_penalty"),
                      (dict(beam_size=4, num_beam_groups=2, diversity_penalty="a"), "diversity_penalty"),
                      (dict(beam_size=4, diversity_penalty=0.5), "num_beam_groups > 1")):
        with pytest.raises(ValueError, match=match):
            M.check_beam_groups(**kw)


def test_methods_refuse_bad_groups_before_any_device_call():
    """host tensors: anything that reached the library or a device would fail another way"""
    bad = ((dict(num_beam_groups=3), "divisible"), (dict(num_beam_groups=2, diversity_penalty=-1.0), "diversity_penalty"),
           (dict(num_beam_groups=2, diversity_penalty=float("inf")), "diversity_penalty"), (dict(diversity_penalty=0.5), "num_beam_groups > 1"))
    dec = sat.DecoderRNN(8, 16, 50, 1)
    model = sat.ShowAndTell(8, 16, 50, 1, arch=dict(layers=(1, 1, 1, 1), width=8), compute_dtype="f32")
    att = sat.ShowAttendTellModel(16, 8, 50, 8, None, feature_size=(4, 8), compute_dtype="f32", vgg_cfg=[8, "M", 8])
    ev = importlib.import_module("show-and-tell_amd.evaluate")
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            dec.sample_beam(torch.zeros(2, 8), 4, end_id=2, **kw)
        with pytest.raises(ValueError, match=match):
            model.sample_beam(torch.zeros(2, 3, 64, 64), 4, 2, **kw)
        with pytest.raises(ValueError, match=match):
            att.sample_beam_features(torch.zeros(2, 4, 8), 4, None, 2, **kw)
        with pytest.raises(ValueError, match=match):
            att.sample_beam(torch.zeros(2, 3, 8, 8), 4, None, 2, **kw)
        with pytest.raises(ValueError, match=match):
            ev.validation_step(model, torch.zeros(2, 3, 64, 64), torch.zeros(2, 5, dtype=torch.int64), [5, 5], beam_size=4, **kw)
    with pytest.raises(TypeError):
        dec.sample_beam(torch.zeros(2, 8), 4, 2, 20, False, None, 0, 0, False, 0.0, 2)          # keyword-only


def test_grouped_entry_points_argument_errors_need_no_device():
    """every refusal comes before anything is enqueued: the 'buffers' are host bytes nothing ever reads"""
    lib = L.load()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    B, K, V, T = 2, 6, 8, 20
    ws = lib.sat_beam_step_groups_ws_bytes(B, K, V, T)

    def step(G=3, lam=0.5, K=K, i=1, last=p, end_id=2, logits=p, ws_bytes=ws, c=None):
        return lib.sat_beam_step_groups(logits, V, p, last, end_id, B, K, V, c, p, p, i, T, G, lam, p, p, p, p, ws_bytes, None)

    assert step(G=0) == ARG and step(G=-2) == ARG and step(G=4) == ARG and step(G=12) == ARG
    assert step(lam=-0.5) == ARG and step(lam=float("nan")) == ARG and step(lam=float("inf")) == ARG
    assert step(last=None) == ARG                                     # G > 1 with an end_id at i > 0 needs the rows' last tokens
    assert step(logits=None) == ARG and step(i=T) == ARG
    assert step(K=9, G=3) == UNSUPPORTED and step(K=16, G=2) == UNSUPPORTED
    assert step(ws_bytes=ws - 1) == WORKSPACE
    assert step(c=C.byref(L.SatBeamConstraints(min_length=-1))) == ARG

    E, H, steps = 8, 16, 20
    w = (C.c_void_p * 4)(p, p, p, p)
    need = lib.sat_beam_decode_groups_ws_bytes(B, K, E, H, V, 1, steps)

    def decode(G=3, lam=0.5, K=K, ws_bytes=need, ids=p, c=None):
        return lib.sat_beam_decode_groups(p, p, w, 1, p, p, B, K, E, H, V, steps, 2, c, G, lam, ids, p, None, None, 256 * 16, ws_bytes, None)

    assert decode(G=0) == ARG and decode(G=4) == ARG and decode(lam=-1.0) == ARG and decode(lam=float("nan")) == ARG
    assert decode(lam=float("inf")) == ARG and decode(ids=None) == ARG
    assert decode(K=9, G=3) == ARG                                    # (no workspace size exists for K > 8)
    assert decode(ws_bytes=need - 1) == WORKSPACE
    assert decode(c=C.byref(L.SatBeamConstraints(length_penalty=-1.0))) == ARG
