"""The launch sequence of `FlatAdam.update` without a device: CPU tensors for the buffers, and a stand-in for the library whose
every function records (name, arguments) and returns 0.  For each configuration the exact list of calls, which buffer and byte
offset every pointer argument denotes, and every scalar are compared with what the RULES say (optim.FlatAdam's docstring; the
expected values below are worked out by hand from the layout, not computed by the code under test).

Layout: parameters of shapes (2, 3), (3,), (5, 7), (1,) -- no size a multiple of 4 -- at offsets 0, 8, 12, 48 of n = 52 floats.
The stand-in's one query, sat_grad_sumsq_partials(k), answers ceil(k / 16) and is not recorded: several partial pairs per segment,
so that the offsets into the one partials array show."""
import importlib

import pytest
import torch

from flat_adam_host import sat

optim = importlib.import_module("show-and-tell_amd.optim")
L = sat._lib

SHAPES = [(2, 3), (3,), (5, 7), (1,)]
LAYOUT = [(0, 6, (2, 3)), (8, 3, (3,)), (12, 35, (5, 7)), (48, 1, (1,))]
N = 52
STREAM = 77
HYPER = dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6)
# which arguments of a call are addresses; sat_adamw_step's argument 12 is the ctypes table of exempt ranges
POINTERS = {"sat_clamp_adam_step": (0, 1, 2, 3), "sat_clamp_adam_step_guarded": (0, 1, 2, 3, 11), "sat_grad_sumsq": (0, 3),
            "sat_adamw_step": (0, 1, 2, 3, 15, 17, 18), "sat_ema_update": (0, 1, 4, 5)}


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == "sat_grad_sumsq_partials":
            return lambda k: (k + 15) // 16

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture(autouse=True)
def no_stream(monkeypatch):
    monkeypatch.setattr(L, "stream", lambda: STREAM)


def core(shapes=SHAPES, tail=0, **settings):
    c = optim.FlatAdam(optim.packed_layout(shapes), "cpu", tail=tail)
    c.lib = Recorder()
    c.lr, c.betas, c.eps = HYPER["lr"], HYPER["betas"], HYPER["eps"]
    c.rehome([torch.nn.Parameter(torch.randn(s)) for s in shapes])
    for k, v in settings.items():
        setattr(c, k, v)
    return c


def decoded(c, extra=()):
    """the recorded calls with every address as (buffer name, byte offset) and the exempt table as a list"""
    buffers = dict(params=c.params, grads=c.grads, m=c.m, v=c.v, ema=c.ema, partials=c._partials, norm=c.last_grad_norm, **dict(extra))

    def where(addr):
        if addr is None:
            return None
        for name, t in buffers.items():
            if t is not None and t.data_ptr() <= addr < t.data_ptr() + t.numel() * t.element_size():
                return (name, addr - t.data_ptr())
        raise AssertionError("address %r lies in no buffer" % (addr,))

    out = []
    for name, args in c.lib.calls:
        args = list(args)
        for i in POINTERS[name]:
            args[i] = where(args[i])
        if name == "sat_adamw_step":
            args[12] = None if args[12] is None else list(args[12])
        out.append((name, tuple(args)))
    return out


def at(name, element=0):
    return (name, 4 * element)


def four(a, g="grads"):
    return (at("params", a), at(g, a), at("m", a), at("v", a))


def test_layout_is_packed_to_multiples_of_four():
    c = core()
    assert c.layout == LAYOUT == optim.packed_layout(SHAPES) and c.n == N
    assert [tuple(t.shape) for t in c.views(c.params)] == SHAPES
    assert all(p.data_ptr() == c.params.data_ptr() + 4 * o and p.grad.data_ptr() == c.grads.data_ptr() + 4 * o
               for p, (o, _, _) in zip(c.tensors, c.layout))
    assert c.lib.calls == [] and c.ema is None and c.last_grad_norm is None and c.step_count == 0


def test_plain_update_behind_a_skip_word_is_one_guarded_launch():
    """TrainStep's defaults: the whole buffer, its fault word (the second of the trailing floats), clip 0.1"""
    c = core(tail=4, clip=0.1)
    versions = [p._version for p in c.tensors]
    c.update(c.grads, None, c.grads[N + 1:N + 2])
    assert decoded(c) == [("sat_clamp_adam_step_guarded", four(0) + (N, 3e-4, 0.8, 0.95, 1e-6, 0.1, 1, at("grads", N + 1), STREAM))]
    assert c.step_count == 1 and [p._version for p in c.tensors] == [v + 1 for v in versions]
    c.update(c.grads, None, c.grads[N + 1:N + 2], lr=0.5)                 # the call's own learning rate, the second step
    assert decoded(c)[1] == ("sat_clamp_adam_step_guarded", four(0) + (N, 0.5, 0.8, 0.95, 1e-6, 0.1, 2, at("grads", N + 1), STREAM))
    assert c.lr == 3e-4 and len(c.lib.calls) == 2


def test_plain_update_without_a_word_is_one_unguarded_launch_per_segment():
    """FusedClampAdam's defaults: no clamp (0.0), no word"""
    c = core()
    c.update(c.grads, [(0, N)])
    c.update(c.grads, [(0, 12), (48, N)])
    assert decoded(c) == [("sat_clamp_adam_step", four(0) + (N, 3e-4, 0.8, 0.95, 1e-6, 0.0, 1, STREAM)),
                          ("sat_clamp_adam_step", four(0) + (12, 3e-4, 0.8, 0.95, 1e-6, 0.0, 2, STREAM)),
                          ("sat_clamp_adam_step", four(48) + (4, 3e-4, 0.8, 0.95, 1e-6, 0.0, 2, STREAM))]
    c.update(c.grads, [])                                                 # every gradient None: the step counts, nothing is launched
    assert len(c.lib.calls) == 3 and c.step_count == 3


def test_norm_decay_and_average_on_the_accumulated_twin():
    """TrainStep with everything on and an open accumulation: `acc` and ITS word in the places of `grads` and the step's.
    The 1-D parameters (8..11, 48..49) do not decay; 52 elements make ceil(52 / 16) = 4 partial pairs"""
    c = core(tail=4, clip=0.1, max_norm=2.5, weight_decay=0.01, ema_decay=0.9)
    c.set_exempt([LAYOUT[1], LAYOUT[3]])
    assert c.exempt == [(8, 11), (48, 49)] and torch.equal(c.ema, c.params) and c.ema is not c.params
    acc = torch.zeros(N + 4)
    for step in (1, 2):
        c.update(acc, None, acc[N + 1:N + 2])
    word, got = at("acc", N + 1), decoded(c, dict(acc=acc))
    for step in (1, 2):
        assert got[3 * step - 3:3 * step] == [
            ("sat_grad_sumsq", (at("acc"), N, 0.1, at("partials"), 0, 4, STREAM)),
            ("sat_adamw_step", four(0, "acc") + (N, 3e-4, 0.8, 0.95, 1e-6, 0.1, step, 0.01, [8, 11, 48, 49], 2, 2.5, at("partials"), 4,
                                                 at("norm"), word, STREAM)),
            ("sat_ema_update", (at("ema"), at("params"), N, 0.9, word, at("norm"), STREAM))]
    assert len(got) == 6 and c._partials.dtype == torch.float64 and c._partials.numel() >= 8
    assert c.last_grad_norm.dtype == torch.float64 and c.last_grad_norm.shape == (2,)


def test_decay_alone_makes_no_norm_pass_and_the_average_follows_the_warm_up():
    c = core(tail=4, weight_decay=0.01, ema_decay=0.999, ema_warmup=True)
    word = c.grads[N + 1:N + 2]
    c.update(c.grads, None, word)
    assert decoded(c) == [
        ("sat_adamw_step", four(0) + (N, 3e-4, 0.8, 0.95, 1e-6, 0.0, 1, 0.01, None, 0, 0.0, None, 0, None, at("grads", N + 1), STREAM)),
        ("sat_ema_update", (at("ema"), at("params"), N, 2 / 11, at("grads", N + 1), None, STREAM))]     # min(0.999, (1 + 1) / (10 + 1))
    assert c.last_grad_norm is None and c._partials is None
    c.ema_decay = 0.0                                                     # off again: the launch goes, the buffer stays
    c.update(c.grads, None, word)
    assert [name for name, _ in c.lib.calls] == ["sat_adamw_step", "sat_ema_update", "sat_adamw_step"] and c.ema is not None


def test_measuring_norm_alone_takes_the_adamw_kernel_without_decay():
    c = core(max_norm=float("inf"))
    c.update(c.grads, [(0, N)])
    assert decoded(c) == [
        ("sat_grad_sumsq", (at("grads"), N, 0.0, at("partials"), 0, 4, STREAM)),
        ("sat_adamw_step", four(0) + (N, 3e-4, 0.8, 0.95, 1e-6, 0.0, 1, 0.0, None, 0, float("inf"), at("partials"), 4, at("norm"), None,
                                      STREAM))]


def test_three_segments_share_one_partials_array():
    """five parameters, the four shapes and (3,) again at 52..55 (n = 56); the second and the fourth have no gradient, so the
    segments are 0..8, 12..48 and 52..56 with 1, 3 and 1 partial pairs at offsets 0, 1, 4 of 5.  The 1-D parameters do not decay:
    8..11, and 48..49 merged with 52..55 (its padded end meets the next start); only the last segment holds any of them, as 0..3"""
    c = core(SHAPES + [(3,)], clip=0.1, max_norm=1.0, weight_decay=0.01, ema_decay=0.5)
    assert c.n == 56
    c.set_exempt([c.layout[1], c.layout[3], c.layout[4]])
    assert c.exempt == [(8, 11), (48, 55)]
    c.update(c.grads, [(0, 8), (12, 48), (52, 56)])
    hp = (3e-4, 0.8, 0.95, 1e-6, 0.1, 1, 0.01)
    tail = (1.0, at("partials"), 5, at("norm"), None, STREAM)
    assert decoded(c) == [
        ("sat_grad_sumsq", (at("grads", 0), 8, 0.1, at("partials"), 0, 5, STREAM)),
        ("sat_grad_sumsq", (at("grads", 12), 36, 0.1, at("partials"), 1, 5, STREAM)),
        ("sat_grad_sumsq", (at("grads", 52), 4, 0.1, at("partials"), 4, 5, STREAM)),
        ("sat_adamw_step", four(0) + (8,) + hp + (None, 0) + tail),
        ("sat_adamw_step", four(12) + (36,) + hp + (None, 0) + tail),
        ("sat_adamw_step", four(52) + (4,) + hp + ([0, 3], 1) + tail),
        ("sat_ema_update", (at("ema"), at("params"), 56, 0.5, None, at("norm"), STREAM))]


def facade(**settings):
    """a FusedClampAdam made without `__init__` (no device) around a recording core"""
    opt = object.__new__(sat.FusedClampAdam)
    opt.core = core(**settings)
    opt.param_groups = [dict(HYPER)]
    opt._views = opt.core.views(opt.core.grads)
    return opt


@pytest.mark.parametrize("missing,segments", [((0,), [(8, N)]), ((2,), [(0, 12), (48, N)]), ((3,), [(0, 48)]), ((0, 3), [(8, 48)]),
                                              ((), [(0, N)])], ids=["first", "middle", "last", "both_ends", "none"])
def test_fused_clamp_adam_covers_the_runs_between_parameters_without_gradient(missing, segments):
    opt = facade(max_norm=1.0)
    for i in missing:
        opt.core.tensors[i].grad = None
    opt.param_groups[0]["lr"] = 0.25                                      # what `set_lr` writes is what the launch gets
    opt.step()
    counts = [(b - a + 15) // 16 for a, b in segments]
    want = [("sat_grad_sumsq", (at("grads", a), b - a, 0.0, at("partials"), sum(counts[:k]), sum(counts), STREAM))
            for k, (a, b) in enumerate(segments)]
    want += [("sat_adamw_step", four(a) + (b - a, 0.25, 0.8, 0.95, 1e-6, 0.0, 1, 0.0, None, 0, 1.0, at("partials"), sum(counts), at("norm"),
                                           None, STREAM)) for a, b in segments]
    assert decoded(opt.core) == want and opt.step_count == 1


def test_fused_clamp_adam_copies_a_stray_gradient_into_its_view_first():
    opt = facade()
    stray = torch.full((5, 7), 3.0)
    opt.core.tensors[2].grad = stray
    opt.step()
    assert torch.equal(opt.flat_grad[12:47], stray.reshape(-1)) and opt.flat_grad[47] == 0
    assert decoded(opt.core) == [("sat_clamp_adam_step", four(0) + (N, 3e-4, 0.8, 0.95, 1e-6, 0.0, 1, STREAM))]
    opt.zero_grad()
    assert opt.core.tensors[2].grad.data_ptr() == opt.flat_grad.data_ptr() + 48 and not opt.flat_grad.any()


def test_update_is_refused_inside_averaged_weights_before_anything_moves():
    c = core(ema_decay=0.9)
    c.averaged = True
    with pytest.raises(RuntimeError, match="averaged"):
        c.update(c.grads)
    assert c.step_count == 0 and c.lib.calls == []
