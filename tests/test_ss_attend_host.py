"""CPU: the host side of scheduled sampling in the Show-Attend-Tell model -- the C-ABI entry points (exported, bound, workspace
formula, argument errors reported without a launch) and the model's attributes and dispatch (eval mode and ss_prob 0 draw nothing)."""
import importlib

import pytest
import torch

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
A = sat.attend

CFG = [8, "M", 32]


def align(n):
    return (n + 255) // 256 * 256


def ws_formula(lib, B, P, C, E, H, V):
    sk = max(max(lib.sat_skinny_gemm_ws_bytes(m, C, H), lib.sat_skinny_gemm_ws_bytes(m, E, C)) for m in range(1, B + 1))
    return (align(lib.sat_ss_decoder_fwd_ws_bytes(B, V)) + align(lib.sat_attention_ws_bytes(B, P)) + align(sk) + align(B * H * 4)
            + align(E * 4))


def test_ss_attend_symbols_exported_and_bound():
    lib = L.load()
    for name in ("sat_ss_attend_fwd", "sat_ss_attend_fwd_ws_bytes"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.sat_version() == L.ABI_VERSION


@pytest.mark.parametrize("dims", [(5, 16, 32, 32, 64, 300), (64, 196, 512, 512, 1024, 10000), (1, 1, 4, 4, 8, 1),
                                  (200, 49, 256, 128, 384, 7)])
def test_ss_attend_workspace_formula(dims):
    lib = L.load()
    assert lib.sat_ss_attend_fwd_ws_bytes(*dims) == ws_formula(lib, *dims)
    assert lib.sat_ss_attend_fwd_ws_bytes(0, 16, 32, 32, 64, 300) == 0


def call(lib, **kw):
    """sat_ss_attend_fwd with every pointer non-null (fake addresses the validation never dereferences) unless overridden"""
    fake = 4096
    a = dict(feats=fake, ctx_enc=fake, h0=fake, c0=fake, captions=fake, cap_stride=4, bs=(L.C.c_int32 * 4)(3, 3, 2, 1), prefix=fake,
             T=4, P=16, C=32, E=32, H=64, V=300, w=(L.C.c_void_p * 14)(*([fake] * 14)), tapes=(L.C.c_void_p * 8)(*([fake] * 8)),
             toks=fake, logits=fake, ldl=300, prob=0.5, seed=1, rank=0, used=fake, used_stride=4, ws=fake, ws_bytes=0)
    a.update(kw)
    return lib.sat_ss_attend_fwd(a["feats"], a["ctx_enc"], a["h0"], a["c0"], a["captions"], a["cap_stride"], a["bs"], a["prefix"],
                                 a["T"], a["P"], a["C"], a["E"], a["H"], a["V"], a["w"], a["tapes"], a["toks"], a["logits"], a["ldl"],
                                 a["prob"], a["seed"], a["rank"], a["used"], a["used_stride"], a["ws"], a["ws_bytes"], None)


def test_ss_attend_argument_errors_are_reported_not_computed():
    lib = L.load()
    for k in ("feats", "ctx_enc", "h0", "c0", "captions", "prefix", "toks", "logits", "used", "ws", "w", "tapes"):
        assert call(lib, **{k: None}) == 1001, k
    w = (L.C.c_void_p * 14)(*([4096] * 14))
    w[12] = None
    assert call(lib, w=w) == 1001
    tapes = (L.C.c_void_p * 8)(*([4096] * 8))
    tapes[7] = None
    assert call(lib, tapes=tapes) == 1001
    for bad in (dict(T=0), dict(P=0), dict(C=30), dict(E=2), dict(H=65), dict(H=60), dict(V=0), dict(rank=-1), dict(cap_stride=3),
                dict(used_stride=3), dict(ldl=299), dict(ldl=302), dict(bs=(L.C.c_int32 * 4)(3, 3, 4, 1)),
                dict(bs=(L.C.c_int32 * 4)(3, 3, 2, 0))):
        assert call(lib, **bad) == 1001, bad
    assert call(lib, ws_bytes=lib.sat_ss_attend_fwd_ws_bytes(3, 16, 32, 32, 64, 300) - 1) == 1002


def small_model():
    return sat.ShowAttendTellModel(96, 32, 50, 64, None, feature_size=(4, 32), compute_dtype="f32", vgg_cfg=CFG)


def test_attend_model_ss_attributes_and_state_dict_keys():
    m = small_model()
    assert m.ss_prob == 0 and m.ss_rank == 0 and m.last_ss_inputs is None and m.last_ss_seed is None
    enc = {"encoder.%s" % k for k in m.encoder.state_dict()}
    assert set(m.state_dict()) == enc | set(A.PARAM_ORDER)
    m.ss_prob, m.ss_rank = 0.25, 2
    assert set(m.state_dict()) == enc | set(A.PARAM_ORDER)
    assert not any(k.startswith(("ss_", "last_ss")) for k in m.state_dict())


class _Guard:
    def __init__(self, device):
        self.status = torch.empty(1, device=device)

    def submit(self, *a):
        pass


@pytest.mark.parametrize("mode", ["eval", "zero", "train"])
def test_attend_decode_dispatch_draws_only_when_sampling(monkeypatch, mode):
    """decode's host side with the GPU call stubbed out: eval() and ss_prob 0 pass ss=None and leave torch's generator alone; a
    training forward with ss_prob > 0 takes one seed from it and records it"""
    seen = {}

    def fake_apply(model, features, fmean, captions, pi, ss, *params):
        seen["ss"] = ss
        if ss is not None:
            ss["used"] = captions[:, :pi.T].clone()
        return torch.zeros(pi.N, model.vocab_size)

    monkeypatch.setattr(A._AttendFn, "apply", staticmethod(fake_apply))
    monkeypatch.setattr(A, "IdGuard", _Guard)
    monkeypatch.setattr(L, "require_gpu", lambda *a: None)
    m = small_model()
    if mode == "eval":
        m.ss_prob = 0.5
        m.eval()
    elif mode == "train":
        m.ss_prob, m.ss_rank = 0.5, 3
    feats = torch.zeros(2, 4, 32)
    caps = torch.ones(2, 5, dtype=torch.int64)
    torch.manual_seed(3)
    rng = torch.get_rng_state()
    m.decode(feats, feats.mean(1), caps, [5, 3])
    if mode == "train":
        torch.set_rng_state(rng)
        seed = sat.models.draw_ss_seed()
        assert seen["ss"]["prob"] == 0.5 and seen["ss"]["rank"] == 3 and seen["ss"]["seed"] == seed
        assert m.last_ss_seed == seed and m.last_ss_inputs is seen["ss"]["used"]
    else:
        assert seen["ss"] is None
        assert torch.equal(torch.get_rng_state(), rng)
        assert m.last_ss_inputs is None and m.last_ss_seed is None
