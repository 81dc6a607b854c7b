#!/usr/bin/env python3
"""Throughput of the Show-Attend-Tell path (model2.py, the model train.py:37 constructs) on one MI355X: training step
(VGG16 features[:-3] frozen + attention decoder fwd + CE + hand-written backward + clamp + torch Adam, train.py:134-146) and
greedy sampling (eval.py:99), batch 64, 224x224, hidden 1024 / embed 512 (config.py:27-28 defaults), vocab 10000, len-20 captions.
    python tools/bench_attend.py [bf16|f32] [--ss-prob P] [--alpha-c A] [--ab REGIONS] [--forwards N]
--ss-prob: scheduled sampling (model.ss_prob) in the training step.  --alpha-c: doubly stochastic attention (model.alpha_c; the
step's loss is CE + model.last_attention_penalty).  --ab REGIONS: only the training step, two settings interleaved (order
alternating per region, 10 steps each), per-region times, medians and spread: alpha_c 0 against A when --alpha-c is given (ss_prob
fixed at P), else ss_prob 0 against P.  --forwards N: only N sampled decoder forwards on fixed features (for a kernel trace)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sat = importlib.import_module("show-and-tell_amd")
ap = argparse.ArgumentParser()
ap.add_argument("dtype", nargs="?", default="bf16", choices=["bf16", "f32"])
ap.add_argument("--ss-prob", type=float, default=0.0)
ap.add_argument("--alpha-c", type=float, default=0.0)
ap.add_argument("--ab", type=int, default=0)
ap.add_argument("--forwards", type=int, default=0)
args = ap.parse_args()
dtype = args.dtype
B, T, V = 64, 20, 10000
torch.manual_seed(123)
model = sat.ShowAttendTellModel(1024, 512, V, 512, None, compute_dtype=dtype).cuda()
images = torch.randn(B, 3, 224, 224, device="cuda")
caps = torch.randint(4, V, (B, T), device="cuda")
caps[:, 0], caps[:, -1] = 1, 2
lengths = [T] * B
targets, l1 = sat.pack_targets(caps, lengths)
FUSED_OPT = os.environ.get("SAT_FUSED_OPT", "1") != "0"     # clip_gradient + Adam as one launch (sat.FusedClampAdam) vs torch
if FUSED_OPT:
    opt = sat.FusedClampAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3, clip=0.1)
else:
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
crit = torch.nn.CrossEntropyLoss()


images_b = torch.randn(B, 3, 224, 224, device="cuda")
batches = [images, images_b]
LOOKAHEAD = os.environ.get("SAT_LOOKAHEAD", "1") != "0"


def step(i=0, last=True):
    if FUSED_OPT:
        opt.zero_grad()
    else:
        model.zero_grad()
    x = batches[i & 1]
    # forward of THIS batch first consumes its (possibly prefetched) features; the NEXT batch's frozen VGG stack then starts on
    # the side stream and runs under this batch's decoder forward / backward / Adam (ShowAttendTellModel.prefetch_features)
    feats, fmean = model._encode(x)
    if LOOKAHEAD and not last:
        model.prefetch_features(batches[(i + 1) & 1])
    loss = crit(model.decode(feats, fmean, caps[:, :-1], l1), targets)
    if model.last_attention_penalty is not None:
        loss = loss + model.last_attention_penalty
    loss.backward()
    if not FUSED_OPT:
        for p in opt.param_groups[0]["params"]:
            p.grad.data.clamp_(-0.1, 0.1)
    opt.step()
    return loss


def region(n=10):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        loss = step(i, i == n - 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, loss


if args.forwards:
    model.ss_prob = args.ss_prob
    feats, fmean = model._encode(images)
    with torch.no_grad():
        for _ in range(args.forwards):
            model.decode(feats, fmean, caps[:, :-1], l1)
    torch.cuda.synchronize()
    print("%d decoder forwards, ss_prob %g" % (args.forwards, args.ss_prob))
    sys.exit(0)
if args.ab:
    if args.alpha_c > 0:
        name, vals = "alpha_c", (0.0, args.alpha_c)
        model.ss_prob = args.ss_prob
    else:
        name, vals = "ss_prob", (0.0, args.ss_prob)
    for v in vals:
        setattr(model, name, v)
        for i in range(3):
            step(i, i == 2)
    times = {v: [] for v in vals}
    for r in range(args.ab):
        for v in (vals if r % 2 == 0 else vals[::-1]):
            setattr(model, name, v)
            times[v].append(region()[0] * 1e3)
    for v in vals:
        print("%s %-5g ms/step per region: %s" % (name, v, " ".join("%.3f" % t for t in times[v])))
    m0, m1 = statistics.median(times[vals[0]]), statistics.median(times[vals[1]])
    print("Show-Attend-Tell train step (%s conv stack, %s), median of %d regions x 10 steps: %s 0 %.3f ms (min %.3f, max %.3f), "
          "%s %g %.3f ms (min %.3f, max %.3f), delta %+.3f ms (%+.1f %%)"
          % (dtype, "FusedClampAdam" if FUSED_OPT else "torch clamp + Adam", args.ab, name, m0, min(times[vals[0]]), max(times[vals[0]]),
             name, vals[1], m1, min(times[vals[1]]), max(times[vals[1]]), m1 - m0, 100 * (m1 - m0) / m0))
    sys.exit(0)
model.ss_prob, model.alpha_c = args.ss_prob, args.alpha_c
for i in range(3):
    loss = step(i, i == 2)
dt, loss = region()
print("Show-Attend-Tell train step (%s conv stack, drop-in autograd path + torch CE, %s, ss_prob %g, alpha_c %g): %.2f ms/step = "
      "%.0f img/s, loss %.4f" % (dtype, "FusedClampAdam" if FUSED_OPT else "torch clamp + Adam", args.ss_prob, args.alpha_c, dt * 1e3,
                                 B / dt, loss.item()))
model.ss_prob = model.alpha_c = 0
with torch.no_grad():
    feats, fmean = model._encode(images)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        model._encode(images)
    torch.cuda.synchronize()
    enc = (time.perf_counter() - t0) / 5
    t0 = time.perf_counter()
    for _ in range(5):
        ids = model.sample_features(feats, None)
    torch.cuda.synchronize()
    dec = (time.perf_counter() - t0) / 5
print("VGG16 features[:-3] forward %.2f ms (%.0f TFLOP/s); greedy sample (20 steps) %.2f ms => %.0f captions/s end to end"
      % (enc * 1e3, 2 * 14.884e9 * B / enc / 1e12, dec * 1e3, B / (enc + dec)))
with torch.no_grad():          # eval.py:99 as a loop over batches with the next batch's frozen VGG stack prefetched
    def pipeline(n):
        for i in range(n):
            if i + 1 < n:
                model.prefetch_features(batches[(i + 1) & 1])
            model.sample(batches[i & 1])
    pipeline(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 12
    pipeline(n)
    torch.cuda.synchronize()
    print("greedy sample with the features look-ahead: %.0f captions/s end to end" % (B * n / (time.perf_counter() - t0)))
    hp = torch.cuda.Stream(priority=-1)          # the decode loop's small dependent launches ahead of the conv workgroups
    hp.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(hp):
        pipeline(3)
        hp.synchronize()
        t0 = time.perf_counter()
        pipeline(n)
        hp.synchronize()
        print("... the same on a high-priority stream: %.0f captions/s" % (B * n / (time.perf_counter() - t0)))
