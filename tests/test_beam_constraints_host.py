"""CPU: the constrained beam search's host side -- the ctypes mirror of `sat_beam_constraints` against the C header, the Python
validator's refusals, the argument errors the library returns before it touches a device, the keyword-only arguments of the five
methods, and the f64 reference of tests/beam_constraints_reference.py on hand-worked prefixes."""
import ctypes as C
import importlib
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

import beam_constraints_reference as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
M = importlib.import_module("show-and-tell_amd.models")

ARG, WORKSPACE, UNSUPPORTED = 1001, 1002, 1003
KEYWORDS = dict(suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False, length_penalty=0.0)


def test_constraints_struct_layout_matches_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "sat_hip.h"
#define O(f) offsetof(sat_beam_constraints, f)
int main(){printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(sat_beam_constraints), O(suppress_ids), O(n_suppress), O(min_length),
 O(no_repeat_ngram), O(block_repeat), O(length_penalty));return 0;}
'''
    d = os.path.join(ROOT, "tests", "_build")
    os.makedirs(d, exist_ok=True)
    src, exe = os.path.join(d, "beam_constraints_layout.c"), os.path.join(d, "beam_constraints_layout")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = L.SatBeamConstraints
    assert out == [C.sizeof(S), S.suppress_ids.offset, S.n_suppress.offset, S.min_length.offset, S.no_repeat_ngram.offset,
                   S.block_repeat.offset, S.length_penalty.offset]
    assert [n for n, _ in S._fields_] == ["suppress_ids", "n_suppress", "min_length", "no_repeat_ngram", "block_repeat", "length_penalty"]


def test_new_symbols_are_declared_bound_and_listed():
    lib = L.load()
    for name in ("sat_beam_step_ex", "sat_beam_step_ex_ws_bytes", "sat_beam_rerank", "sat_beam_decode_ex_ws_bytes", "sat_beam_decode_ex"):
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name), name
    assert lib.sat_version() == L.ABI_VERSION == 18
    assert lib.sat_beam_step_ex_ws_bytes(4, 5, 1000, 20) == lib.sat_beam_step_ws_bytes(4, 5)       # stateless: no history
    assert lib.sat_beam_step_ex_ws_bytes(4, 5, 1000, 0) == 0
    base = lib.sat_beam_decode_ws_bytes(4, 5, 32, 64, 203, 2, 20)
    assert lib.sat_beam_decode_ex_ws_bytes(4, 5, 32, 64, 203, 2, 20) > base > 0
    assert lib.sat_beam_decode_ex_ws_bytes(4, 9, 32, 64, 203, 2, 20) == 0


@pytest.mark.parametrize("owner,method", [("DecoderRNN", "sample_beam"), ("ShowAndTell", "sample_beam"),
                                          ("ShowAttendTellModel", "sample_beam_features"), ("ShowAttendTellModel", "sample_beam"),
                                          (None, "validation_step")])
def test_the_five_methods_take_the_same_keyword_only_constraints(owner, method):
    fn = getattr(getattr(sat, owner), method) if owner else importlib.import_module("show-and-tell_amd.evaluate").validation_step
    p = inspect.signature(fn).parameters
    for name, default in KEYWORDS.items():
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, (method, name)


def test_validator_accepts_and_reports():
    c = M.check_beam_constraints()
    assert not c.active
    c = M.check_beam_constraints([3, 0, 1], 6, 2, True, 0.7, end_id=2, vocab_size=1000, steps=20)
    assert c.active and c.suppress_ids == [3, 0, 1] and (c.min_length, c.no_repeat_ngram_size, c.block_repeat) == (6, 2, True)
    assert c.length_penalty == pytest.approx(0.7, rel=1e-7) and c.length_penalty == float(np.float32(0.7))
    assert M.check_beam_constraints(length_penalty=0.5).active                  # the rerank alone is a constraint too
    assert M.check_beam_constraints(np.array([4, 5]), end_id=2).suppress_ids == [4, 5]
    assert M.check_beam_constraints(suppress_ids=list(range(256)), end_id=300).active


@pytest.mark.parametrize("kw,match", [
    (dict(suppress_ids=[2, 5], end_id=2), "end_id"),
    (dict(suppress_ids=[-1]), "suppress_ids"),
    (dict(suppress_ids=[1000], vocab_size=1000), "suppress_ids"),
    (dict(suppress_ids=[1.5]), "suppress_ids"),
    (dict(suppress_ids=[True]), "suppress_ids"),
    (dict(suppress_ids=5), "suppress_ids"),
    (dict(suppress_ids=list(range(257))), "256"),
    (dict(min_length=-1, end_id=2), "min_length"),
    (dict(min_length=2.0, end_id=2), "min_length"),
    (dict(min_length=3), "end_id"),
    (dict(min_length=3, end_id=-1), "end_id"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=True), "no_repeat_ngram_size"),
    (dict(block_repeat=2), "block_repeat"),
    (dict(block_repeat="yes"), "block_repeat"),
    (dict(length_penalty=-0.1), "length_penalty"),
    (dict(length_penalty=float("nan")), "length_penalty"),
    (dict(length_penalty=float("inf")), "length_penalty"),
    (dict(length_penalty=1e39), "length_penalty"),
    (dict(length_penalty="a"), "length_penalty"),
    (dict(no_repeat_ngram_size=2, steps=65), "64"),
    (dict(block_repeat=True, vocab_size=65537), "65536"),
])
def test_validator_refuses(kw, match):
    with pytest.raises(ValueError, match=match):
        M.check_beam_constraints(**kw)


def test_validator_bounds_bind_only_step_constraints():
    """the rerank has no T or V bound: a length penalty alone passes where a step constraint is refused"""
    assert M.check_beam_constraints(length_penalty=1.0, steps=100, vocab_size=100000).active


def test_methods_refuse_bad_constraints_before_any_device_work():
    dec = sat.DecoderRNN(8, 16, 50, 1)
    import torch
    with pytest.raises(ValueError, match="end_id"):
        dec.sample_beam(torch.zeros(2, 8), 3, end_id=2, suppress_ids=[2])
    with pytest.raises(ValueError, match="suppress_ids"):
        dec.sample_beam(torch.zeros(2, 8), 3, end_id=2, suppress_ids=[50])
    with pytest.raises(TypeError):
        dec.sample_beam(torch.zeros(2, 8), 3, 2, 20, False, [3])                  # keyword-only


def _cons(**kw):
    return L.SatBeamConstraints(**kw)


def test_step_ex_and_rerank_argument_errors_need_no_device():
    """every refusal comes before anything is enqueued: the 'buffers' are host bytes nothing ever reads"""
    lib = L.load()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    B, K, V, T = 2, 3, 8, 20
    ws = lib.sat_beam_step_ex_ws_bytes(B, K, V, T)
    ok = _cons(suppress_ids=p, n_suppress=2, min_length=3, no_repeat_ngram=2, block_repeat=1, length_penalty=0.5)

    def step(c=ok, end_id=2, i=1, T=T, K=K, V=V, ldl=V, logits=p, parents=p, tokens=p, out=p, ws_bytes=ws):
        return lib.sat_beam_step_ex(logits, ldl, p, p, end_id, B, K, V, C.byref(c) if c is not None else None, parents, tokens, i, T,
                                    p, p, out, p, ws_bytes, None)

    assert step(logits=None) == ARG and step(out=None) == ARG and step(ldl=V - 1) == ARG
    assert step(i=-1) == ARG and step(i=T) == ARG and step(T=0, i=0) == ARG
    assert step(c=None, i=T) == ARG                                             # the step index is checked with or without constraints
    for bad in (dict(n_suppress=-1), dict(min_length=-1), dict(no_repeat_ngram=-1), dict(block_repeat=-1), dict(block_repeat=2),
                dict(n_suppress=257, suppress_ids=p), dict(n_suppress=1), dict(length_penalty=-1.0),
                dict(length_penalty=float("nan")), dict(length_penalty=float("inf"))):
        assert step(c=_cons(**bad)) == ARG, bad
    assert step(c=_cons(min_length=1), end_id=-1) == ARG
    assert step(parents=None) == ARG and step(tokens=None) == ARG               # active constraints at i > 0 walk the records
    assert step(K=9) == UNSUPPORTED
    assert step(T=65) == UNSUPPORTED and step(V=65537, ldl=65537) == UNSUPPORTED
    assert step(ws_bytes=ws - 1) == WORKSPACE

    def rerank(ids=p, scores=p, B=2, K=3, T=5, alpha=0.5, ids_out=p + 2048, scores_out=p + 1024):
        return lib.sat_beam_rerank(ids, scores, B, K, T, 2, alpha, ids_out, scores_out, None, None, None)

    assert rerank(ids=None) == ARG and rerank(scores=None) == ARG and rerank(ids_out=None) == ARG and rerank(scores_out=None) == ARG
    assert rerank(ids_out=p) == ARG and rerank(scores_out=p) == ARG             # in place
    assert rerank(B=0) == ARG and rerank(K=0) == ARG and rerank(T=0) == ARG
    assert rerank(alpha=-0.5) == ARG and rerank(alpha=float("nan")) == ARG and rerank(alpha=float("inf")) == ARG
    assert rerank(K=9) == UNSUPPORTED


def test_decode_ex_argument_errors_need_no_device():
    lib = L.load()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    B, K, E, H, V, steps = 2, 3, 8, 16, 50, 20
    w = (C.c_void_p * 4)(p, p, p, p)
    need = lib.sat_beam_decode_ex_ws_bytes(B, K, E, H, V, 1, steps)

    def call(c, end_id=2, steps=steps, V=V, ws=256 * 16, ws_bytes=need, ids=p):
        return lib.sat_beam_decode_ex(p, p, w, 1, p, p, B, K, E, H, V, steps, end_id, C.byref(c) if c is not None else None, ids, p, None,
                                      None, ws, ws_bytes, None)

    assert call(_cons(min_length=-1)) == ARG and call(_cons(n_suppress=300, suppress_ids=p)) == ARG
    assert call(_cons(min_length=2), end_id=-1) == ARG and call(_cons(length_penalty=-1.0)) == ARG
    assert call(_cons(block_repeat=1), ids=None) == ARG
    assert call(_cons(no_repeat_ngram=2), steps=65, ws_bytes=1 << 40) == UNSUPPORTED
    assert call(_cons(block_repeat=1), V=65537, ws_bytes=1 << 40) == UNSUPPORTED
    assert call(_cons(block_repeat=1), ws_bytes=need - 1) == WORKSPACE
    assert call(None, ws_bytes=lib.sat_beam_decode_ws_bytes(B, K, E, H, V, 1, steps)) == WORKSPACE      # _ex always sizes for the rerank


# ---- the reference itself, on prefixes worked by hand ----
def test_reference_ngram_rule_on_hand_worked_prefixes():
    ban = BC.banned_tokens
    # i < n: nothing yet
    assert ban([7], no_repeat_ngram=2) == set() and ban([7, 8], no_repeat_ngram=3) == set() and ban([], no_repeat_ngram=1) == set()
    # i == n: the one earlier n-gram is the prefix itself; it bans its last token only when its head equals the tail
    assert ban([7, 8], no_repeat_ngram=2) == set()                   # tail (8): bigram (7, 8) starts with 7
    assert ban([7, 7], no_repeat_ngram=2) == {7}                     # tail (7): bigram (7, 7) -> a third 7 would repeat it
    assert ban([5, 6, 5], no_repeat_ngram=3) == set() and ban([5, 5, 5], no_repeat_ngram=3) == {5}
    # n = 1: every token already emitted
    assert ban([4, 9, 4, 2], no_repeat_ngram=1) == {4, 9, 2}
    # bigrams: after a b a, b is banned (a b exists); after a b a b c a: b again, from the FIRST two occurrences
    assert ban([1, 2, 1], no_repeat_ngram=2) == {2}
    assert ban([1, 2, 1, 3, 1], no_repeat_ngram=2) == {2, 3}
    # overlapping: x x x with n = 2 -- the bigram (x, x) at j = 0 and j = 1 (the latter overlaps the tail) both ban x
    assert ban([6, 6, 6], no_repeat_ngram=2) == {6}
    # trigrams: 1 2 3 1 2 -> 3; 1 2 3 2 1 -> nothing
    assert ban([1, 2, 3, 1, 2], no_repeat_ngram=3) == {3} and ban([1, 2, 3, 2, 1], no_repeat_ngram=3) == set()
    # a trigram that overlaps the tail: 4 4 4 4 -> tail (4, 4), trigrams at j = 0, 1 -> 4
    assert ban([4, 4, 4, 4], no_repeat_ngram=3) == {4}


def test_reference_other_rules_on_hand_worked_prefixes():
    ban = BC.banned_tokens
    assert ban([], block_repeat=True) == set()                       # step 0: nothing to repeat
    assert ban([3], block_repeat=True) == {3} and ban([3, 9], block_repeat=True) == {9}
    assert ban([], end_id=2, min_length=1) == {2} and ban([5], end_id=2, min_length=1) == set()
    assert ban([5] * 5, end_id=2, min_length=6) == {2} and ban([5] * 6, end_id=2, min_length=6) == set()
    assert ban([5], end_id=None, min_length=6) == set()
    assert ban([8], end_id=2, suppress_ids=(3, 0, 1), min_length=6, no_repeat_ngram=1, block_repeat=True) == {3, 0, 1, 2, 8}


def test_reference_step_does_not_renormalise_and_skips_finished_and_dead_rows():
    K, V = 4, 6
    x = np.zeros((K, V), dtype=np.float32)
    x[:, 1] = math.log(9 * (V - 1))                                  # 90 % of every row's mass sits on column 1
    scores = np.array([[-1.0, -2.0, -np.inf, -0.5]])
    last = np.array([[5, 2, 5, 5]])                                  # row 1 is finished (end_id 2), row 2 dead
    c = BC.Constraints(suppress_ids=(1,))
    r = BC.step_ref(x, scores, last, 2, K, [[[5]] * K], c)
    lse = math.log((V - 1) + math.exp(float(x[0, 1])))            # (the f32 logit as stored: ~log(50))
    assert r["nbans"] == 2                                           # rows 0 and 3: the finished and the dead row are skipped
    cand = r["cand"].reshape(K, V)
    assert np.isneginf(cand[0, 1]) and np.isneginf(cand[3, 1])
    np.testing.assert_allclose(cand[0, [0, 2, 3, 4, 5]], -1.0 - lse, rtol=0, atol=1e-12)        # NOT -1 - log(V - 1)
    assert cand[1, 2] == -2.0 and np.isneginf(np.delete(cand[1], 2)).all()
    assert np.isneginf(cand[2]).all()
    assert r["parent"][0].tolist() == [1, 3, 3, 3] and r["token"][0].tolist() == [2, 0, 2, 3]


def test_reference_prefixes_and_rerank():
    parents = np.array([[[0, 0, 0]], [[1, 0, 2]], [[2, 2, 0]]])     # [T = 3, B = 1, K = 3]
    tokens = np.array([[[10, 11, 12]], [[20, 21, 22]], [[30, 31, 32]]])
    assert BC.prefixes_ref(parents, tokens, 0) == [[[], [], []]]
    assert BC.prefixes_ref(parents, tokens, 1) == [[[10], [11], [12]]]
    assert BC.prefixes_ref(parents, tokens, 2) == [[[11, 20], [10, 21], [12, 22]]]
    assert BC.prefixes_ref(parents, tokens, 3) == [[[12, 22, 30], [12, 22, 31], [11, 20, 32]]]
    ids = np.array([[[5, 2, 2, 2], [5, 6, 7, 2], [5, 6, 7, 8], [2, 2, 2, 2]]])
    scores = np.array([[-2.0, -3.0, -3.5, -np.inf]])
    r = BC.rerank_ref(ids, scores, 2, 1.0)
    assert r["L"].tolist() == [[2, 4, 4, 1]]                         # the <end> counts; no <end>: T
    np.testing.assert_allclose(r["norm"][0, :3], [-0.75, -0.875, -1.0])
    assert r["order"].tolist() == [[1, 2, 0, 3]] and np.isneginf(r["norm"][0, 3])
    assert BC.rerank_ref(ids, scores, 2, 0.0)["order"].tolist() == [[0, 1, 2, 3]]
    tie = BC.rerank_ref(ids[:, :2], np.array([[-2.0, -4.0]]), 2, 1.0)          # -2 / 2 == -4 / 4: the previous rank decides
    assert tie["order"].tolist() == [[0, 1]]
