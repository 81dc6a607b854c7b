#!/usr/bin/env python3
"""`sat_image_augment_u8` at B = 64, 256x256 -> 224x224 beside `sat_gather_rows_f32` on [64, 150528] (the other streaming kernel
of the input path), N launches each, for `rocprofv3 --kernel-trace --stats -- python tools/augment_trace.py` (`DESIGN.md` §8).
Also prints an event-timed figure per launch; the trace is the record."""
import importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
lib = L.load()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
B = 64
u8 = torch.randint(0, 256, (B, 256, 256, 3), dtype=torch.uint8).cuda()
tf = sat.ImageTransform(224, generator=torch.Generator().manual_seed(1))
params = tf.draw(B, 256, 256)
out = torch.empty(B, 3, 224, 224, device="cuda")
src = torch.randn(B, 150528, device="cuda")
dst = torch.empty_like(src)
order = torch.randperm(B).int().cuda()
def gather():
    L.check(lib.sat_gather_rows_f32(src.data_ptr(), order.data_ptr(), B, src.shape[1], dst.data_ptr(), L.stream()), "gather")
def augment():
    tf(u8, params=params, out=out)
for name, fn, nbytes in (("sat_image_augment_u8", augment, B * 224 * 224 * 3 * 5), ("sat_gather_rows_f32", gather, src.numel() * 8)):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    print("%s: %.1f us per launch incl. launch gaps (%d launches), %.1f MB moved -> %.2f TB/s" % (name, us, reps, nbytes / 1e6, nbytes / us / 1e6), flush=True)
