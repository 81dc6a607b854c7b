"""MI355X: `sat_image_augment_u8` through `ImageTransform` and `DevicePrefetcher(transform=...)` against the plain-torch CPU
restatement of `main.py:26-36` (tests/augment_reference.py).  Every comparison is `torch.equal`: there are only 3 x 256 possible
outputs and the kernel makes them with the reference's own two IEEE divisions.  The shapes are the smallest at which each
failure mode can appear (misaligned source rows, store head and tail, more than one workgroup per image, the real sizes)."""
import functools
import importlib

import pytest
import torch

import augment_reference as R

sat = importlib.import_module("show-and-tell_amd")
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def source(B, Hs, Ws):
    return R.source(B, Hs, Ws, seed=B * 1000 + Hs + Ws)


def params_of(rows):
    return torch.tensor(rows, dtype=torch.int32)


def run(u8, crop, params, **kw):
    t = sat.ImageTransform(crop, **{k: kw.pop(k) for k in ("mean", "std", "train") if k in kw})
    out = t(u8.cuda(), params=params, **kw)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    return out.cpu()


CASES = {
    # odd Ws: misaligned source row bases; Wc % 4 != 0: head and tail of the stores; left covers every residue mod 4
    "row alignments a": (3, 19, 23, (13, 13), [(0, 0, 0), (3, 1, 1), (6, 2, 0)]),
    "row alignments b": (3, 19, 23, (13, 13), [(5, 3, 1), (1, 5, 0), (6, 10, 1)]),
    "extremes": (4, 20, 24, (16, 16), [(0, 0, 0), (4, 8, 1), (0, 8, 1), (4, 0, 0)]),
    "no crop": (2, 16, 16, (16, 16), [(0, 0, 0), (0, 0, 1)]),
    "width 1 tail": (1, 8, 9, (5, 1), [(2, 7, 1)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_small_geometries_are_bit_exact(name):
    B, Hs, Ws, crop, rows = CASES[name]
    u8, p = source(B, Hs, Ws), params_of(rows)
    assert torch.equal(run(u8, crop, p), R.augment(u8, p, crop))


@pytest.mark.parametrize("B,S,crop", [(2, 256, 224), (1, 320, 299)], ids=["256 to 224", "320 to 299"])
def test_real_geometries_with_random_train_params(B, S, crop):
    u8 = source(B, S, S)
    t = sat.ImageTransform(crop, generator=torch.Generator().manual_seed(3))
    p = t.draw(B, S, S)
    want = R.augment(u8, p, (crop, crop))
    assert torch.equal(t(u8.cuda(), params=p).cpu(), want)
    # params=None draws from the generator: the same seed gives the same images
    t2 = sat.ImageTransform(crop, generator=torch.Generator().manual_seed(3))
    assert torch.equal(t2(u8.cuda()).cpu(), want)


def test_order_is_a_gather_with_repeats():
    u8 = source(3, 19, 23)
    order = [2, 0, 2, 1]                               # B = 4 outputs from Bsrc = 3 images, one of them twice
    p = params_of([(0, 0, 0), (3, 1, 1), (6, 2, 0), (2, 7, 1)])
    assert torch.equal(run(u8, (13, 13), p, order=order), R.augment(u8, p, (13, 13), order=order))
    order = [2, 0]                                     # and fewer outputs than images
    assert torch.equal(run(u8, (13, 13), p[:2], order=order), R.augment(u8, p[:2], (13, 13), order=order))
    order = [2, 0, 2]
    assert torch.equal(run(u8, (13, 13), p[:3], order=order), R.augment(u8, p[:3], (13, 13), order=order))


def test_eval_mode_is_the_centre_crop():
    u8 = source(2, 256, 256)
    got = sat.ImageTransform(224, train=False)(u8.cuda()).cpu()
    assert torch.equal(got, R.augment(u8, [(16, 16, 0)] * 2, (224, 224)))
    u8 = source(3, 19, 23)                             # odd differences: int(round(6 / 2.)) = 3, int(round(10 / 2.)) = 5
    assert torch.equal(sat.ImageTransform(13, train=False)(u8.cuda()).cpu(), R.augment(u8, [(3, 5, 0)] * 3, (13, 13)))


def test_runs_on_the_current_stream():
    u8, p = source(4, 20, 24), params_of(CASES["extremes"][4])
    st = torch.cuda.Stream()
    d = u8.cuda()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        out = sat.ImageTransform(16)(d, params=p)
    st.synchronize()
    assert torch.equal(out.cpu(), R.augment(u8, p, (16, 16)))


@pytest.mark.parametrize("offset", [0, 5])
def test_out_is_filled_and_nothing_else_is_written(offset):
    """`out=` inside a larger buffer of a sentinel (offset 5: a base that is not 16-byte aligned, so every row has a head)"""
    B, Hs, Ws, crop, rows = CASES["row alignments b"]
    u8, p = source(B, Hs, Ws), params_of(rows)
    n, guard, sentinel = B * 3 * 13 * 13, 64, -12345.0
    buf = torch.full((guard + offset + n + guard,), sentinel, device="cuda")
    out = buf[guard + offset: guard + offset + n].view(B, 3, 13, 13)
    got = sat.ImageTransform(crop)(u8.cuda(), params=p, out=out)
    assert got is out
    host = buf.cpu()
    assert torch.equal(host[guard + offset: guard + offset + n].view(B, 3, 13, 13), R.augment(u8, p, crop))
    assert bool((host[:guard + offset] == sentinel).all()) and bool((host[guard + offset + n:] == sentinel).all())


def test_other_mean_and_std():
    B, Hs, Ws, crop, rows = CASES["extremes"]
    u8, p = source(B, Hs, Ws), params_of(rows)
    mean, std = (0.5, 0.25, 0.1), (0.5, 1.5, 0.3)
    assert torch.equal(run(u8, crop, p, mean=mean, std=std), R.augment(u8, p, crop, mean=mean, std=std))


def host_batches(n=4):
    g = torch.Generator().manual_seed(9)
    return [(R.source(2, 20, 24, seed=100 + i).pin_memory(), torch.randint(1, 50, (2, 5), generator=g).pin_memory(), [5, 5])
            for i in range(n)]


def test_prefetcher_transforms_uint8_batches_behind_the_copy():
    batches = host_batches()
    pf = sat.DevicePrefetcher(batches, "cuda", transform=sat.ImageTransform(16, generator=torch.Generator().manual_seed(4)))
    ref = sat.ImageTransform(16, generator=torch.Generator().manual_seed(4))
    seen = 0
    for (im, cp, ln), (u8, caps, lens) in zip(pf, batches):
        assert im.is_cuda and im.dtype == torch.float32 and tuple(im.shape) == (2, 3, 16, 16)
        assert torch.equal(im.cpu(), R.augment(u8, ref.draw(2, 20, 24), (16, 16)))
        assert torch.equal(cp.cpu(), caps) and ln == lens
        seen += 1
    assert seen == 4


def test_prefetcher_upcoming_images_are_the_tensors_yielded_later():
    batches = host_batches()
    pf = sat.DevicePrefetcher(batches, "cuda", depth=2, transform=sat.ImageTransform(16, generator=torch.Generator().manual_seed(4)))
    announced, yielded = [], []
    for i, (im, cp, ln) in enumerate(pf):
        up = pf.upcoming_images(wait=True)
        assert len(up) == min(2, 3 - i) and up.last == (i >= 2)
        for t in up:
            assert t.dtype == torch.float32 and tuple(t.shape) == (2, 3, 16, 16) and hasattr(t, "_sat_ready_event")
        announced.append([(t, t.cpu()) for t in up])             # wait=True: safe to read on this stream now
        yielded.append(im)
    for i, ups in enumerate(announced):
        for k, (t, snapshot) in enumerate(ups):
            assert t is yielded[i + 1 + k] and torch.equal(snapshot, yielded[i + 1 + k].cpu())


def test_prefetcher_passes_float_batches_through():
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(2, 3, 16, 16, generator=g).pin_memory(), torch.randint(1, 50, (2, 5), generator=g).pin_memory(), [5, 5])
               for _ in range(2)]
    pf = sat.DevicePrefetcher(batches, "cuda", transform=sat.ImageTransform(16, generator=torch.Generator().manual_seed(4)))
    for (im, cp, ln), (f32, caps, lens) in zip(pf, batches):
        assert torch.equal(im.cpu(), f32) and torch.equal(cp.cpu(), caps)
