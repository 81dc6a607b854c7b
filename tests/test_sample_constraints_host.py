"""CPU: constrained sampling's host side -- the numpy reference of tests/sample_constraints_reference.py on hand-planted prefixes,
the ctypes mirror of `sat_sample_constraints` against the C header, the new symbols, the Python validator's refusals, the
keyword-only arguments of the four `sample_stochastic` methods and `decode_samples`' forwarding, the argument errors the library
returns before it touches a device, and the excuse caps of the GPU sweep counted on the reference alone."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sample_constraints_reference as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
M = importlib.import_module("show-and-tell_amd.models")

ARG, WORKSPACE, UNSUPPORTED = 1001, 1002, 1003
KEYWORDS = dict(suppress_ids=None, min_length=0, no_repeat_ngram_size=0, block_repeat=False, repetition_penalty=1.0, end_id=None)
NEW = ("sat_sample_filtered_ex", "sat_sample_decode_ex_ws_bytes", "sat_sample_decode_ex")
NINF = -np.inf


# ---- the reference itself, on prefixes worked by hand ----
def test_reference_ngram_rule_on_hand_planted_prefixes():
    x = np.arange(1, 9, dtype=np.float32)                                           # V = 8, all positive
    def banned_cols(prefix, **kw):
        return set(np.flatnonzero(np.isneginf(SC.transform(x, prefix, **kw))).tolist())
    # n = 2: the tail is [5]; 5 was followed by 6 and by 7
    assert banned_cols([5, 6, 1, 5, 7, 5], no_repeat_ngram=2) == {6, 7}
    # n = 3, overlapping with the tail: prefix 4 4 4 -> tail [4, 4], the 3-gram starting at 0 is 4 4 4: bans 4
    assert banned_cols([4, 4, 4], no_repeat_ngram=3) == {4}
    assert banned_cols([4, 4], no_repeat_ngram=3) == set()                          # n > t: not yet
    assert banned_cols([1, 2, 3, 1, 2], no_repeat_ngram=3) == {3}
    assert banned_cols([1, 2, 3, 2, 1], no_repeat_ngram=3) == set()
    # n = 1 bans every token drawn so far, from step 1
    assert banned_cols([], no_repeat_ngram=1) == set()
    assert banned_cols([3, 3, 6], no_repeat_ngram=1) == {3, 6}
    # tokens outside [0, V) are no tokens: they set nothing, and match each other only as "no token"
    assert banned_cols([-1, 5, 8, 5], no_repeat_ngram=1) == {5}
    assert banned_cols([7, 8, 3, 7, -1], no_repeat_ngram=3) == {3}


def test_reference_other_rules_and_the_penalty():
    x = np.array([2.0, -2.0, 0.0, 3.0, -1.0, NINF, np.nan, 6.0], dtype=np.float32)
    th = np.float32(1.3)
    # a token that occurs three times is penalised once; positive logits are divided, the others multiplied
    got = SC.transform(x, [0, 0, 1, 0, 2, 5, 6], repetition_penalty=1.3)
    want = x.copy()
    want[0], want[1], want[2] = np.float32(2.0) / th, np.float32(-2.0) * th, 0.0
    assert np.array_equal(got[:6], want[:6]) and np.isnan(got[6]) and got[7] == 6.0 and got.dtype == np.float32
    # theta < 1 rewards: positive logits grow
    got = SC.transform(x, [3, 4], repetition_penalty=0.8)
    assert got[3] == np.float32(3.0) / np.float32(0.8) and got[4] == np.float32(-1.0) * np.float32(0.8)
    # a ban wins over the penalty; the start of the prefix bans nothing by itself
    got = SC.transform(x, [3, 0], repetition_penalty=1.3, block_repeat=True, suppress_ids=[3, 7])
    assert np.isneginf(got[[0, 3, 7]]).all() and got[1] == x[1]
    # min_length holds end_id back while t < min_length
    assert np.isneginf(SC.transform(x, [1, 1], min_length=3, end_id=7)[7])
    assert SC.transform(x, [1, 1, 1], min_length=3, end_id=7)[7] == 6.0
    assert np.array_equal(SC.transform(x, [], block_repeat=True, no_repeat_ngram=2, repetition_penalty=1.3)[:6], x[:6])   # t = 0
    # out-of-range ids are ignored
    assert np.array_equal(SC.transform(x, [8, -1], repetition_penalty=2.0, block_repeat=True, suppress_ids=[8, 99])[:6], x[:6])


def test_reference_row_without_a_candidate_and_the_draw():
    x = np.array([1.0, 0.5, -1.0], dtype=np.float32)
    ref = SC.reference(SC.transform(x, [], suppress_ids=[0, 1, 2]), 1.0, 0, 1.0, 5, 0, 0, 0)
    assert ref[0] == 0 and ref[2] == 0 and ref[4] == NINF and len(ref[5]) == 0
    n, clr, tok, margin, lp, order = SC.reference(SC.transform(x, [], suppress_ids=[0]), 1.0, 0, 1.0, 5, 0, 0, 0)
    assert n == 2 and tok in (1, 2) and order.tolist() == [1, 2]
    w = np.exp(np.array([0.5, -1.0]))
    assert lp == pytest.approx(float(np.log(w[tok - 1] / w.sum())), abs=1e-12)           # renormalised over what is left
    assert SC.check_properties(np.array([[1, 2, 1, 2]]), SC.Rules(block_repeat=True), 3) == 4
    with pytest.raises(AssertionError):
        SC.check_properties(np.array([[1, 2, 2, 0]]), SC.Rules(block_repeat=True), 3)


# ---- the C ABI ----
def test_constraints_struct_layout_matches_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "sat_hip.h"
#define O(f) offsetof(sat_sample_constraints, f)
int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sat_sample_constraints), O(suppress_ids), O(n_suppress), O(min_length),
 O(no_repeat_ngram), O(block_repeat), O(repetition_penalty), O(end_id));return 0;}
'''
    d = os.path.join(ROOT, "tests", "_build")
    os.makedirs(d, exist_ok=True)
    src, exe = os.path.join(d, "sample_constraints_layout.c"), os.path.join(d, "sample_constraints_layout")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    S = L.SatSampleConstraints
    assert out == [C.sizeof(S), S.suppress_ids.offset, S.n_suppress.offset, S.min_length.offset, S.no_repeat_ngram.offset,
                   S.block_repeat.offset, S.repetition_penalty.offset, S.end_id.offset]


def test_new_symbols_are_declared_bound_and_listed():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]
    assert "sat_sample_constraints;" in hdr
    assert lib.sat_version() == L.ABI_VERSION == 18 and "#define SAT_ABI_VERSION 18" in hdr
    assert len(L.SIGNATURES["sat_sample_filtered_ex"][1]) == len(L.SIGNATURES["sat_sample_filtered"][1]) + 3
    assert len(L.SIGNATURES["sat_sample_decode_ex"][1]) == len(L.SIGNATURES["sat_sample_decode"][1]) + 1
    assert lib.sat_sample_decode_ex_ws_bytes(4, 32, 64, 203, 2) == lib.sat_sample_decode_ws_bytes(4, 32, 64, 203, 2) > 0
    assert lib.sat_sample_decode_ex_ws_bytes(0, 32, 64, 203, 2) == 0


def _cons(**kw):
    kw.setdefault("repetition_penalty", 1.0)
    kw.setdefault("end_id", -1)
    return L.SatSampleConstraints(**kw)


def test_filtered_ex_argument_errors_need_no_device():
    """every refusal comes before anything is enqueued: the 'buffers' are host bytes nothing ever reads"""
    lib = L.load()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    R_, V = 2, 8
    ws = lib.sat_sample_filtered_ws_bytes(R_, V)
    ok = _cons(suppress_ids=p, n_suppress=2, min_length=3, no_repeat_ngram=2, block_repeat=1, repetition_penalty=1.2, end_id=2)

    def step(c=ok, t=1, V=V, ldl=V, logits=p, ids=p, prefix=p, stride=64, ws_bytes=ws, tau=1.0):
        return lib.sat_sample_filtered_ex(logits, ldl, R_, V, tau, 0, 1.0, 5, t, 0, ids, 1, None, None, C.byref(c) if c is not None else None,
                                          prefix, stride, p, ws_bytes, None)

    assert step(logits=None) == ARG and step(ids=None) == ARG and step(ldl=V - 1) == ARG and step(t=-1) == ARG and step(tau=0.0) == ARG
    assert step(c=None, logits=None) == ARG                                     # the plain checks hold with or without constraints
    for bad in (dict(n_suppress=-1), dict(min_length=-1, end_id=2), dict(no_repeat_ngram=-1), dict(block_repeat=-1), dict(block_repeat=2),
                dict(n_suppress=257, suppress_ids=p), dict(n_suppress=1), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")), dict(min_length=1),
                dict(min_length=1, end_id=-3)):
        assert step(c=_cons(**bad)) == ARG, bad
    for reads in (dict(block_repeat=1), dict(no_repeat_ngram=1), dict(repetition_penalty=1.5)):
        assert step(c=_cons(**reads), prefix=None) == ARG, reads                # a rule that reads the prefix, t > 0
        assert step(c=_cons(**reads), stride=-1) == ARG, reads
        assert step(c=_cons(**reads), t=64) == UNSUPPORTED and step(c=_cons(**reads), t=1000) == UNSUPPORTED, reads
    assert step(c=_cons(no_repeat_ngram=2), t=64) == UNSUPPORTED
    assert step(V=32769, ldl=32769) == UNSUPPORTED
    assert step(ws_bytes=ws - 1) == WORKSPACE


def test_decode_ex_argument_errors_need_no_device():
    lib = L.load()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    B, E, H, V, steps = 2, 8, 16, 50, 20
    w = (C.c_void_p * 4)(p, p, p, p)
    need = lib.sat_sample_decode_ex_ws_bytes(B, E, H, V, 1)

    def call(c, steps=steps, V=V, ws_bytes=need, ids=p, tau=1.0):
        return lib.sat_sample_decode_ex(p, p, w, 1, p, p, B, E, H, V, steps, tau, 0, 1.0, 5, 0, p, p, p, p, ids, steps, None, None, None, 0,
                                        C.byref(c) if c is not None else None, 256 * 8, ws_bytes, None)

    assert call(_cons(min_length=-1, end_id=2)) == ARG and call(_cons(n_suppress=300, suppress_ids=p)) == ARG
    assert call(_cons(min_length=2)) == ARG and call(_cons(repetition_penalty=0.0)) == ARG and call(_cons(block_repeat=3)) == ARG
    assert call(_cons(block_repeat=1), ids=None) == ARG and call(_cons(block_repeat=1), tau=-1.0) == ARG and call(None, ids=None) == ARG
    for active in (dict(no_repeat_ngram=2), dict(n_suppress=1, suppress_ids=p), dict(repetition_penalty=1.1)):
        assert call(_cons(**active), steps=65, ws_bytes=1 << 40) == UNSUPPORTED, active
    assert call(_cons(block_repeat=1), V=32769, ws_bytes=1 << 40) == UNSUPPORTED
    assert call(_cons(block_repeat=1), ws_bytes=need - 1) == WORKSPACE and call(None, ws_bytes=need - 1) == WORKSPACE


# ---- Python ----
@pytest.mark.parametrize("owner,method", [("DecoderRNN", "sample_stochastic"), ("ShowAndTell", "sample_stochastic"),
                                          ("ShowAttendTellModel", "sample_stochastic"),
                                          ("ShowAttendTellModel", "sample_stochastic_features")])
def test_the_methods_take_the_same_keyword_only_constraints(owner, method):
    p = inspect.signature(getattr(getattr(sat, owner), method)).parameters
    for name, default in KEYWORDS.items():
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, (method, name)
    assert list(inspect.signature(M.check_sample_constraints).parameters)[:6] == list(KEYWORDS)


def test_validator_accepts_and_reports():
    c = M.check_sample_constraints()
    assert not c.active and c is M.check_sample_constraints(end_id=2)           # the defaults build nothing
    c = M.check_sample_constraints([3, 0, 1], 6, 2, True, 1.2, end_id=2, vocab_size=1000, steps=20)
    assert c.active and c.suppress_ids == [3, 0, 1] and (c.min_length, c.no_repeat_ngram_size, c.block_repeat, c.end_id) == (6, 2, True, 2)
    assert c.repetition_penalty == float(np.float32(1.2))
    for kw in (dict(repetition_penalty=0.8), dict(block_repeat=True), dict(no_repeat_ngram_size=1), dict(suppress_ids=[0]),
               dict(min_length=1, end_id=2)):
        assert M.check_sample_constraints(**kw).active, kw
    assert not M.check_sample_constraints(repetition_penalty=1).active and not M.check_sample_constraints(steps=100).active
    assert M.check_sample_constraints(np.array([4, 5]), end_id=2).suppress_ids == [4, 5]
    assert M.check_sample_constraints(suppress_ids=list(range(256)), end_id=300, steps=64).end_id == 300
    assert M.check_sample_constraints(block_repeat=True).end_id == -1


@pytest.mark.parametrize("kw,match", [
    (dict(suppress_ids=[2, 5], end_id=2), "end_id"),
    (dict(suppress_ids=[-1]), "suppress_ids"),
    (dict(suppress_ids=[1000], vocab_size=1000), "suppress_ids"),
    (dict(suppress_ids=[1.5]), "suppress_ids"),
    (dict(suppress_ids=5), "suppress_ids"),
    (dict(suppress_ids=list(range(257))), "256"),
    (dict(min_length=-1, end_id=2), "min_length"),
    (dict(min_length=3), "end_id"),
    (dict(min_length=3, end_id=-1), "end_id"),
    (dict(end_id="x"), "end_id"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
    (dict(block_repeat=2), "block_repeat"),
    (dict(repetition_penalty=0), "repetition_penalty"),
    (dict(repetition_penalty=-1.5), "repetition_penalty"),
    (dict(repetition_penalty=float("nan")), "repetition_penalty"),
    (dict(repetition_penalty=float("inf")), "repetition_penalty"),
    (dict(repetition_penalty=1e39), "repetition_penalty"),
    (dict(repetition_penalty=1e-46), "repetition_penalty"),
    (dict(repetition_penalty=True), "repetition_penalty"),
    (dict(repetition_penalty="a"), "repetition_penalty"),
    (dict(no_repeat_ngram_size=2, steps=65), "64"),
    (dict(repetition_penalty=1.1, steps=65), "64"),
    (dict(suppress_ids=[1], steps=65), "64"),
])
def test_validator_refuses(kw, match):
    with pytest.raises(ValueError, match=match):
        M.check_sample_constraints(**kw)


def test_methods_refuse_bad_constraints_before_any_device_work():
    dec = sat.DecoderRNN(8, 16, 50, 1)
    feats = torch.zeros(2, 8)
    with pytest.raises(ValueError, match="end_id"):
        dec.sample_stochastic(feats, end_id=2, suppress_ids=[2])
    with pytest.raises(ValueError, match="suppress_ids"):
        dec.sample_stochastic(feats, suppress_ids=[50])
    with pytest.raises(ValueError, match="repetition_penalty"):
        dec.sample_stochastic(feats, repetition_penalty=0.0)
    with pytest.raises(ValueError, match="end_id"):
        dec.sample_stochastic(feats, min_length=4)
    with pytest.raises(TypeError):
        dec.sample_stochastic(feats, None, 1.0, 0, 1.0, 1, None, False, False, [3])      # keyword-only
    att = sat.ShowAttendTellModel(12, 8, 11, 4, None, feature_size=(5, 8), compute_dtype="f32", vgg_cfg=[8])
    with pytest.raises(ValueError, match="64"):
        att.sample_stochastic_features(torch.zeros(2, 5, 8), steps=65, block_repeat=True)
    with pytest.raises(ValueError, match="suppress_ids"):
        att.sample_stochastic_features(torch.zeros(2, 5, 8), suppress_ids=[11])

    class Refuses:                                                             # the two methods behind an encoder check first
        def __call__(self, *a, **k):
            raise AssertionError("the encoder ran")
    full = sat.ShowAndTell.__new__(sat.ShowAndTell)
    torch.nn.Module.__init__(full)
    full.decoder, full.encoder = dec, Refuses()
    with pytest.raises(ValueError, match="repetition_penalty"):
        full.sample_stochastic(torch.zeros(2, 3, 8, 8), repetition_penalty=-1.0)
    att._encode = Refuses()
    with pytest.raises(ValueError, match="min_length"):
        att.sample_stochastic(torch.zeros(2, 3, 8, 8), min_length=-2, end_id=2)


def test_decode_samples_forwards_the_constraints():
    Consensus = importlib.import_module("show-and-tell_amd.consensus").ConsensusReranker
    seen = {}

    class Model:
        def sample_stochastic(self, inputs, **kw):
            seen.update(kw)
            raise RuntimeError("forwarded")

    rr = Consensus.__new__(Consensus)
    with pytest.raises(RuntimeError, match="forwarded"):
        Consensus.decode_samples(rr, Model(), None, 3, suppress_ids=[0, 1, 3], min_length=5, end_id=2, no_repeat_ngram_size=3,
                                 repetition_penalty=1.2, top_p=0.9)
    assert seen == dict(num_samples=3, suppress_ids=[0, 1, 3], min_length=5, end_id=2, no_repeat_ngram_size=3, repetition_penalty=1.2,
                        top_p=0.9)
    assert "repetition_penalty" in Consensus.decode_samples.__doc__


# ---- the GPU sweep's excuses, counted before any device exists ----
def test_sweep_excuse_caps_hold_on_the_reference_alone():
    cases = SC.sweep_cases()
    assert len(cases) == 2016
    assert {c[:4] for c in cases} == {(V, ldl, R_, t) for V in SC.VS for ldl in SC.ldls_of(V) for R_ in SC.RS for t in SC.TS}
    for V in SC.VS:                                                             # every pair meets every rule set and every setting
        for pair in [(ldl, R_) for ldl in SC.ldls_of(V) for R_ in SC.RS]:
            mine = [c for c in cases if c[0] == V and c[1:3] == pair]
            assert {c[4] for c in mine} == {n for n, _ in SC.RULE_SETS} and {c[6] for c in mine} == set(SC.SETTINGS), (V, pair)
    total, band, close, empty = SC.sweep_excuses()
    print("sweep: %d launches, %d rows checked; reference alone: %d in the rounding band, %d close draws, %d without a candidate"
          % (len(cases), total, band, close, empty))
    assert total == 4032 and 100 * band <= total and 100 * close <= total
    assert empty > 0                                                            # the "no candidate" case stays in the sweep
