"""CPU: the host side of the on-device image transform (`main.py:26-36`): `sat_image_augment_u8` is declared, exported by both
builds of the library and rejects bad arguments without a launch; `ImageTransform.draw` draws what RandomCrop / CenterCrop /
RandomHorizontalFlip draw; `ImageTransform.__call__` validates before it touches the GPU; the prefetcher draws in batch order."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
NAME = "sat_image_augment_u8"


def test_symbol_is_declared_bound_and_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert re.search(r"\bint %s\s*\(" % NAME, hdr)
    assert NAME in L.SIGNATURES and NAME in L.ADDED_WITHIN_ABI
    hooks = L.open_library(os.path.join(ROOT, "tests", "_build", "libsat_hip_testhooks.so"))
    for lib in (L.load(), hooks):
        assert hasattr(lib, NAME)
        assert lib.sat_version() == 18                  # an addition does not raise the ABI version
    assert L.ABI_VERSION == 18 and "#define SAT_ABI_VERSION 18\n" in hdr


F3 = C.c_float * 3
MEAN, STD = F3(0.485, 0.456, 0.406), F3(0.229, 0.224, 0.225)
P = 0x1000          # a non-null pointer that is never dereferenced: every call below is rejected before any launch


def call(lib, **kw):
    a = dict(src=P, Bsrc=2, Hs=8, Ws=8, params=P, order=None, B=2, Hc=4, Wc=4, mean=MEAN, std=STD, out=P)
    a.update(kw)
    return lib.sat_image_augment_u8(a["src"], a["Bsrc"], a["Hs"], a["Ws"], a["params"], a["order"], a["B"], a["Hc"], a["Wc"],
                                    a["mean"], a["std"], a["out"], None)


@pytest.mark.parametrize("bad", [
    dict(src=None), dict(params=None), dict(out=None),
    dict(B=0), dict(B=-1), dict(Bsrc=0), dict(Hc=0), dict(Wc=0), dict(Wc=-4),
    dict(Hc=9), dict(Wc=9),
    dict(std=F3(0.229, 0.0, 0.225)), dict(std=F3(float("inf"), 0.224, 0.225)), dict(std=F3(0.229, 0.224, float("nan"))),
], ids=lambda d: "%s=%s" % (next(iter(d)), "bad" if "std" in d else next(iter(d.values()))))
def test_argument_errors_are_reported_without_a_launch(bad):
    assert call(L.load(), **bad) == 1001


def test_draw_dtype_shape_and_ranges():
    t = sat.ImageTransform(224, generator=torch.Generator().manual_seed(0))
    p = t.draw(64, 256, 300)
    assert p.dtype == torch.int32 and tuple(p.shape) == (64, 3) and not p.is_cuda
    assert 0 <= int(p[:, 0].min()) and int(p[:, 0].max()) <= 32
    assert 0 <= int(p[:, 1].min()) and int(p[:, 1].max()) <= 76
    assert set(p[:, 2].tolist()) <= {0, 1}
    hw = sat.ImageTransform((5, 1), generator=torch.Generator().manual_seed(0)).draw(50, 8, 9)
    assert int(hw[:, 0].max()) <= 3 and int(hw[:, 1].max()) <= 8
    with pytest.raises(ValueError):
        t.draw(2, 200, 256)


def test_draw_center_crop_rounds_like_torchvision():
    t = sat.ImageTransform(224, train=False)
    assert t.draw(3, 256, 256).tolist() == [[16, 16, 0]] * 3
    for hs, ws in ((229, 231), (227, 225), (224, 224), (235, 226)):           # odd differences: int(round(./2.)), half to even
        want = [int(round((hs - 224) / 2.)), int(round((ws - 224) / 2.)), 0]
        assert t.draw(2, hs, ws).tolist() == [want] * 2
    assert t.draw(1, 229, 227).tolist() == [[2, 2, 0]]                        # 2.5 -> 2, 1.5 -> 2


def test_draw_is_reproducible_from_the_seed():
    def seq(seed):
        t = sat.ImageTransform(224, generator=torch.Generator().manual_seed(seed))
        return torch.cat([t.draw(8, 256, 256) for _ in range(3)])
    assert torch.equal(seq(7), seq(7))
    assert not torch.equal(seq(7), seq(8))
    torch.manual_seed(11)
    a = sat.ImageTransform(224).draw(8, 256, 256)                             # generator=None: torch's default CPU generator
    torch.manual_seed(11)
    assert torch.equal(a, sat.ImageTransform(224).draw(8, 256, 256))


def test_draw_reaches_both_extremes():
    p = sat.ImageTransform(14, generator=torch.Generator().manual_seed(1)).draw(300, 16, 16)
    assert set(p[:, 0].tolist()) == {0, 1, 2} and set(p[:, 1].tolist()) == {0, 1, 2}


def test_draw_flips_half_of_the_images():
    p = sat.ImageTransform(14, generator=torch.Generator().manual_seed(2)).draw(4096, 16, 16)
    assert abs(float(p[:, 2].float().mean()) - 0.5) <= 0.05                   # sigma = 0.0078: more than 6 sigma, fixed seed


def test_call_validates_on_the_host_before_any_gpu_work():
    t = sat.ImageTransform(16)
    u8 = torch.zeros(2, 20, 24, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # a CPU tensor, everything else in order
        t(u8)
    with pytest.raises(TypeError):
        t(u8.float())
    with pytest.raises(ValueError):
        t(torch.zeros(2, 3, 20, 24, dtype=torch.uint8))                       # CHW layout
    with pytest.raises(ValueError):
        t(torch.zeros(2, 12, 24, 3, dtype=torch.uint8))                       # crop larger than the source
    ok = torch.tensor([[4, 8, 1], [0, 0, 0]], dtype=torch.int32)
    for r, c, v in ((0, 0, 5), (0, 0, -1), (1, 1, 9), (1, 1, -1), (0, 2, 2), (1, 2, -1)):
        bad = ok.clone()
        bad[r, c] = v
        with pytest.raises(ValueError, match="out of range"):
            t(u8, params=bad)
    with pytest.raises(TypeError):
        t(u8, params=ok.long())
    with pytest.raises(ValueError):
        t(u8, params=ok[:1])
    with pytest.raises(ValueError):
        t(u8, params=ok, order=[0, 2])                                        # names an image that is not there
    with pytest.raises(ValueError):
        sat.ImageTransform(16, std=(0.2, 0.0, 0.2))


class _HostOnlyPrefetcher(sat.DevicePrefetcher):
    """the real queue (`__iter__`, `_stage`, `_draw`) with the two device halves cut off"""

    def __init__(self, batches, depth, transform):
        self.batches, self.depth, self.transform = batches, depth, transform
        self._queue, self._done = [], False

    def _upload(self, batch, params):
        return tuple(batch) + (params,), None

    def _acquire(self, ready, ev):
        pass


def test_prefetcher_draws_in_batch_order_whatever_the_depth():
    batches = [(torch.zeros(2, 20, 24, 3, dtype=torch.uint8), torch.zeros(2, 5, dtype=torch.long), [5, 5]) for _ in range(5)]
    batches.insert(2, (torch.zeros(2, 3, 16, 16), torch.zeros(2, 5, dtype=torch.long), [5, 5]))      # a float batch draws nothing

    def run(depth):
        t = sat.ImageTransform(16, generator=torch.Generator().manual_seed(5))
        return [b[-1] for b in _HostOnlyPrefetcher(batches, depth, t)]
    d1, d3 = run(1), run(3)
    direct = sat.ImageTransform(16, generator=torch.Generator().manual_seed(5))
    assert len(d1) == len(d3) == 6
    for i, (a, b) in enumerate(zip(d1, d3)):
        if i == 2:
            assert a is None and b is None
        else:
            assert torch.equal(a, b) and torch.equal(a, direct.draw(2, 20, 24))
    assert len({tuple(p.flatten().tolist()) for p in d1 if p is not None}) > 1
