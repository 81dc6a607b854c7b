"""CPU: the rollout of the attention decoder (`sat_rollout_attend_fwd`, `ShowAttendTellModel.rollout` / `scst_forward`,
`SelfCritical.attend`) -- the names exist at every layer, the entry point checks its arguments before anything is enqueued (so it
runs without a GPU), the Python names refuse CPU tensors and eval mode, and the seeds of the GPU replay test have no near tie on the
oracle's own rollout."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

import scst_attend_reference as SA

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import attend as OA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sat_rollout_attend_fwd", "sat_rollout_attend_fwd_ws_bytes")


def test_header_library_and_binding_have_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert int(re.search(r"#define SAT_ABI_VERSION (\d+)", hdr).group(1)) == 18 == L.ABI_VERSION
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI, name
        fn = getattr(lib, name)                   # AttributeError if the built library does not export it
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]
    assert len(L.SIGNATURES["sat_rollout_attend_fwd"][1]) == 28


def test_rollout_attend_checks_arguments_before_any_launch():
    lib = L.load()
    fake = C.c_void_p(4096)                     # never dereferenced: every check below fails first
    B, steps = 5, SA.STEPS
    P, Cc, E, H, V = (SA.SMALL[k] for k in "PCEHV")
    w14, t8 = (C.c_void_p * 14)(*[4096] * 14), (C.c_void_p * 8)(*[4096] * 8)
    need = lib.sat_rollout_attend_fwd_ws_bytes(B, P, Cc, E, H, V)
    assert need >= lib.sat_ss_attend_fwd_ws_bytes(B, P, Cc, E, H, V) > 0
    assert need >= lib.sat_vocab_argmax_ws_bytes(B, V)
    assert lib.sat_rollout_attend_fwd_ws_bytes(0, P, Cc, E, H, V) == 0

    def call(**kw):
        a = dict(feats=fake, ctx_enc=fake, h0=fake, c0=fake, prefix=fake, B=B, steps=steps, P=P, C=Cc, E=E, H=H, V=V, w=w14, tapes=t8,
                 toks=fake, logits=fake, ldl=300, greedy=0, start_id=1, seed=7, rank=0, ids=fake, ids_stride=steps, fed=fake,
                 fed_stride=steps, ws=fake, ws_bytes=need)
        a.update(kw)
        return lib.sat_rollout_attend_fwd(a["feats"], a["ctx_enc"], a["h0"], a["c0"], a["prefix"], a["B"], a["steps"], a["P"], a["C"],
                                          a["E"], a["H"], a["V"], a["w"], a["tapes"], a["toks"], a["logits"], a["ldl"], a["greedy"],
                                          a["start_id"], a["seed"], a["rank"], a["ids"], a["ids_stride"], a["fed"], a["fed_stride"],
                                          a["ws"], a["ws_bytes"], None)

    for greedy in (0, 1):
        assert call(greedy=greedy, ws_bytes=need - 1) == 1002
        for bad in (dict(feats=None), dict(ctx_enc=None), dict(h0=None), dict(c0=None), dict(prefix=None), dict(toks=None),
                    dict(logits=None), dict(ids=None), dict(fed=None), dict(ws=None), dict(B=0), dict(steps=0), dict(P=0), dict(C=30),
                    dict(E=30), dict(H=E + Cc + 4), dict(V=0), dict(ldl=299), dict(ldl=302), dict(start_id=-1), dict(start_id=V),
                    dict(ids_stride=steps - 1), dict(fed_stride=steps - 1), dict(B=1 << 20, steps=1 << 12),
                    dict(w=(C.c_void_p * 14)(*([4096] * 13 + [None]))), dict(tapes=(C.c_void_p * 8)(*([4096] * 6 + [None, 4096])))):
            assert call(greedy=greedy, **bad) == 1001, bad
    assert call(rank=-1) == 1001
    assert call(greedy=1, rank=-1, ws_bytes=need - 1) == 1002          # rank is ignored by the arg-max mode: the next check answers
    # a feature map whose attention rows do not fit the kernel's shared memory: refused before step 0, not in it
    big = lib.sat_rollout_attend_fwd_ws_bytes(B, 20000, Cc, E, H, V)
    assert call(P=20000, ws_bytes=big) == 1003


def tiny_model():
    return sat.ShowAttendTellModel(24, 16, 50, 8, None, feature_size=(4, 16), compute_dtype="f32", vgg_cfg=[8, "M", 16])


def test_new_names_refuse_cpu_tensors():
    model = tiny_model().train()
    feats = torch.zeros(2, 4, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.rollout(feats, feats.mean(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.rollout(feats, feats.mean(1), greedy=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.scst_forward(torch.zeros(2, 3, 32, 32), [0, 1], None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sat.SelfCritical(None).attend(model, feats, feats.mean(1), [0, 1])
    assert model.last_rollout_inputs is None and model.last_rollout_seed is None and model.last_scst is None


def test_rollout_in_eval_mode_raises():
    model = tiny_model().eval()
    feats = torch.zeros(2, 4, 16)
    rng = torch.get_rng_state()
    for greedy in (False, True):
        with pytest.raises(RuntimeError, match="training forward"):
            model.rollout(feats, feats.mean(1), greedy=greedy)
    assert torch.equal(torch.get_rng_state(), rng)                      # refused before a seed is drawn


@pytest.mark.parametrize("case", SA.REPLAY_CASES)
def test_replay_seeds_have_no_near_tie_on_the_oracle(case):
    """the GPU replay test may skip a draw whose top two perturbed scores are within 1e-4; its seeds are chosen so that the
    oracle's own rollout has none"""
    B, rank, steps, ms = case
    p, feats = SA.params(OA), SA.features(B)
    torch.manual_seed(ms)
    seed = sat.models.draw_ss_seed()
    ids, margin, logits, fed = SA.oracle_rollout(OA, p, feats, steps, seed, rank)
    print("draws %d, smallest top-two gap %.3g" % (margin.size, margin.min()))
    assert int((margin < 1e-4).sum()) == 0, margin.min()
    assert ids.min() >= 0 and ids.max() < SA.SMALL["V"]
    assert (fed[:, 0] == SA.START).all() and torch.equal(fed[:, 1:], ids[:, :-1])
    # the step-by-step rollout is the oracle's teacher-forced forward on the tokens fed
    ref = OA.attend_forward(p, feats, fed, [steps] * B)
    assert float((logits - ref).abs().max()) < 1e-5
