#!/usr/bin/env python3
"""Headline benchmark: images/sec of one Show-and-Tell training step (the reference's hot-loop window
`/root/reference/train.py:123-149`: forward, CE, backward, elementwise clamp, Adam) on synthetic data.

    python bench.py --gpus N --steps K --warmup W [--workload train|inception|decode] [--dump-outputs DIR] [--full]

N > 1: when not already running under torch.distributed.run, this process starts the N ranks itself (a child
`python -m torch.distributed.run --nproc-per-node N`, spawned BEFORE anything here touches the GPU) and passes their
exit code on; under torch.distributed.run (RANK / WORLD_SIZE set) it is one rank.  One rank per GPU over RCCL
(`SAT_BENCH_BACKEND=gloo` swaps the transport: the rehearsal of the N > 1 branch on a box with one GPU, together with
`SAT_BENCH_SHARE_DEVICE=1`, which lets several ranks sit on one device).

Workloads (BASELINE.json `configs`):
  train      configs[1], the headline: per-GPU batch 64, 224x224x3 images, length-20 captions, embed 256, hidden 512, vocab 10000,
             1 LSTM layer, ResNet-152 encoder (frozen, train-mode batch statistics); configs[2] is the same step at --gpus 8
  inception  configs[3]: Inception-v3 encoder (299x299) + 2-layer LSTM hidden 1024 (embed 512), batch 64: the same train step
  decode     configs[4]: beam_size=5 decode (`--beam 1`: greedy, models.py:56-67) of 64 images per GPU, eval-mode ResNet-152
             encoder included (eval.py:93-99); captions/sec; shards by image across ranks with no exchange step
Conv stack in bf16 MFMA (f32 accumulate).  Inputs are resident in HBM when the timed region starts.  Weak scaling: the per-GPU
batch is fixed.  Prints ONE JSON line on rank 0 (contract in the task statement).

A plain run sets up, warms up, times exactly K steps once, writes the last step's outputs when --dump-outputs is given, and prints
the line.  --full adds everything else on top of that line: the `roofline` object (per-launch conv timing, PMC traffic), the f32
parity mode, the sequential schedule, the LSTM / decode-step rooflines, the decode breakdown and feature check, the `cpu_baseline`
object, and the median of 5 timed regions.
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# main stream + two look-ahead streams + RCCL's stream: more streams than HIP's default 4 hardware queues would serialise two of
# them (the package sets the same default at import; here before torch can initialise the runtime, and inherited by spawned ranks)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

CFG = dict(batch=64, image=224, embed=256, hidden=512, vocab=10000, layers=1, cap_len=20)
WORKLOADS = {
    "train": dict(CFG, arch=None, metric="images/sec (train step)", unit="images/sec",
                  name="BASELINE configs[1]: batch=64/GPU 224x224x3 + len-20 captions, ResNet-152 encoder (frozen, train-mode BN), "
                       "embed=256 hidden=512 vocab=10000 L=1; fwd+CE+bwd+clamp+Adam"),
    "inception": dict(CFG, image=299, embed=512, hidden=1024, layers=2, arch="inception_v3", metric="images/sec (train step)",
                      unit="images/sec",
                      name="BASELINE configs[3]: batch=64/GPU 299x299x3 + len-20 captions, Inception-v3 encoder (frozen, train-mode BN), "
                           "embed=512 hidden=1024 vocab=10000 L=2; fwd+CE+bwd+clamp+Adam"),
    "decode": dict(CFG, arch=None, metric="captions/sec (decode, encoder included)", unit="captions/sec",
                   name="BASELINE configs[4]: batch=64 images/GPU 224x224x3, eval-mode ResNet-152 encoder + 20-step decode "
                        "(embed=256 hidden=512 vocab=10000 L=1), eval.py:93-99"),
}
INCEPTION_V3_CONV_MACS = 5711168096        # per 299x299 image, 94 convs (= oracle.inception.conv_macs(): tests/test_cabi_and_host.py)
PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.0        # dense f32 MFMA peak (v_mfma_f32_32x32x2_f32), same guide
PEAK_HBM_GBS = 8000.0
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "r05_pmc_traffic.json")
LIB_FILE = os.path.join(ROOT, "show-and-tell_amd", "libsat_hip.so")
BF16_CE_TOL = 2e-3             # stated tolerance of the bf16 mode's mean CE against the f32 oracle (tests/test_gpu_parity_full.py)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="train")
    ap.add_argument("--beam", type=int, default=5, help="--workload decode: beam width (1 = greedy, models.py:56-67)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: the conv roofline (and its PMC traffic), the CPU "
                         "baseline, the f32 parity mode, the sequential schedule, the LSTM / decode-step rooflines, the decode "
                         "breakdown and feature check; the timed region is repeated 5 times unless --repeats says otherwise")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step to DIR/<name>.npy (float32 / "
                         "float64): train: the loss and the updated trainable parameters (tensors above 2^20 elements as a fixed, "
                         "seeded sample of 2^20); decode: the caption ids")
    ap.add_argument("--repeats", type=int, default=None,
                    help="the K-step timed region (barrier + synchronize on both sides, MAX over ranks) is run this many times "
                         "(default 1, 5 with --full); `value` / `ms_per_step` are the MEDIAN repetition, min and max ride along as extra fields")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-f32-mode", action="store_true", help="with --full: skip the secondary measurements (f32 parity mode, sequential schedule, LSTM roofline)")
    ap.add_argument("--no-lookahead", dest="lookahead", action="store_false",
                    help="run the frozen conv stack of batch i+1 strictly after batch i's optimizer step (no side-stream overlap)")
    ap.add_argument("--force-dist", action="store_true", help="initialise RCCL and run the bucket all-reduces even with one rank")
    ap.add_argument("--selftest-launch", action="store_true",
                    help="CPU-only check of the rank plumbing (spawn, rendezvous, barrier, max-over-ranks, one JSON line): gloo, no GPU work")
    ap.add_argument("--selftest-fail-rank", type=int, default=-1,
                    help="with --selftest-launch: this rank exits with code 7 (the launcher must hand a rank's failure on)")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` outside torch.distributed.run: start the N ranks as a child process tree and hand
    their exit code on.  Nothing in this parent has touched the GPU (torch is not even imported yet), and the parent
    is never replaced by exec."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def synth_batch(torch, B, V, T, H, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)          # SURVEY 8d synthetic inputs
    images = torch.randn(B, 3, H, H, generator=g)
    caps = torch.randint(4, V, (B, T), generator=g)
    caps[:, 0], caps[:, T - 1] = 1, 2
    return images.to(device), caps.to(device), [T] * B


DUMP_SAMPLE = 1 << 20              # --dump-outputs: larger tensors are written as this many elements at fixed, seeded positions
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """--dump-outputs: `arrays` = [(name, tensor)], written as dirname/<name>.npy -- floating tensors as float32, integer ones as
    float64 (exact) -- flattened to a fixed, seeded sample of DUMP_SAMPLE elements when larger, so two builds compare element for
    element"""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    total = 0
    for name, t in arrays:
        a = t.detach().cpu().numpy()
        a = a.astype(np.float32 if a.dtype.kind == "f" else np.float64)
        if a.size > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_SAMPLE, replace=False))
            a = a.reshape(-1)[idx]
        total += a.nbytes
        if total > DUMP_LIMIT_BYTES:
            raise SystemExit("--dump-outputs: more than %d MB" % (DUMP_LIMIT_BYTES >> 20))
        np.save(os.path.join(dirname, name + ".npy"), a)


def conv_in_sequence_us(torch, model, images, reps=3, groups=1):
    """Duration of every implicit-GEMM conv launch of the stack (the dominant kernel) measured IN SEQUENCE: the whole
    encoder program runs in order (BatchNorm kernels between the convs, as in the step) and each conv launch reports
    its own dispatch begin/end timestamps (HIP events attached to the launch on the stream it runs on) -- the same
    quantity rocprofv3 --kernel-trace lists per launch.  Returns (sum of conv durations per pass in ms, launches)."""
    if groups > 1:
        # the program the timed steps really run: `groups` look-ahead batches per launch (EncoderCNN.prefetch_many); an instance of
        # its own, so nothing of the model's running statistics moves (deferred updates that are never applied)
        prog = model.encoder._program(images, instance="g_bench", groups=groups)
        arg = [images] + [images.clone() for _ in range(groups - 1)]
    else:
        prog, arg = model.encoder._program(images), images
    prog.run_timed(arg)                                    # warm
    tot, n = 0.0, 0
    for _ in range(reps):
        _, us = prog.run_timed(arg)
        tot += sum(us)
        n = len(us)
    return tot / reps * 1e-3, n


def host_cores():
    """(cores this process may run on, cgroup CPU quota in cores or None, os.cpu_count())"""
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                # cgroup v2: "<quota us> <period us>" or "max <period>"
            q, p = f.read().split()
            if q != "max":
                quota = round(int(q) / int(p), 2)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, p = int(f.read()), int(g.read())
                if q > 0:
                    quota = round(q / p, 2)
        except (OSError, ValueError):
            pass
    return aff, quota, os.cpu_count() or 1


def _thread_probe(torch, fn, units, candidates):
    """best (rate, threads) of one timed call of fn() per torch thread count (after one warm-up call each)"""
    best = (0.0, torch.get_num_threads())
    for th in candidates:
        torch.set_num_threads(th)
        fn()
        t0 = time.perf_counter()
        fn()
        rate = units / (time.perf_counter() - t0)
        if rate > best[0]:
            best = (rate, th)
    return best


def _baseline_threads(torch):
    aff, quota, ncpu = host_cores()
    default_threads = torch.get_num_threads()
    cap = min(aff, ncpu)
    cands = sorted({t for t in (8, 16, 32, default_threads, int(quota) if quota else 0) if 0 < t <= cap})
    return aff, quota, ncpu, default_threads, cands or [default_threads]


def cpu_baseline(torch, seed, wl, workload):
    """The CPU oracle (a port of the reference path, validated against the reference's goldens) timed on this host's
    cores on a bounded sample of the same workload, at the best torch thread count of a short probe.  `cores` = the cores this
    process may run on (sched_getaffinity; the cgroup CPU quota rides along), `threads` = the torch threads used."""
    from oracle import decoder as OD
    from oracle import encoder as OE
    from oracle import train_step as OT
    aff, quota, ncpu, default_threads, cands = _baseline_threads(torch)
    gen = torch.Generator().manual_seed(seed)
    E, H, V, Lh, T, S = wl["embed"], wl["hidden"], wl["vocab"], wl["layers"], wl["cap_len"], wl["image"]
    dp = OD.init_decoder_params(E, H, V, Lh, generator=gen)

    def batch(B):
        images = torch.randn(B, 3, S, S, generator=gen)
        caps = torch.randint(4, V, (B, T), generator=gen)
        caps[:, 0], caps[:, -1] = 1, 2
        return images, caps, [T] * B

    common = {"cores": aff, "threads": None, "host_cpu_count": ncpu, "cgroup_cpu_quota": quota, "kind": "port"}
    if workload == "decode":
        ep, eb = OE.init_encoder_params(E, OE.RESNET152, generator=gen)
        B = 16
        images, _, _ = batch(B)
        beam = wl["beam"]

        def run():
            with torch.no_grad():
                feats = OE.encoder_forward(ep, eb, images, OE.RESNET152, training=False)
                return OD.beam_search(dp, feats, beam, Lh, end_id=2) if beam > 1 else OD.greedy_sample(dp, feats, Lh)

        rate, threads = _thread_probe(torch, run, B, cands)
        torch.set_num_threads(threads)
        n = 3
        t0 = time.perf_counter()
        for _ in range(n):
            run()
        rate = max(rate, B * n / (time.perf_counter() - t0))
        torch.set_num_threads(default_threads)
        common.update(value=round(rate, 2), unit="captions/sec", threads=threads,
                      sample="CPU oracle (oracle/encoder.py eval-mode ResNet-152 + oracle/decoder.py %s, torch-CPU fp32): %d timed batches "
                             "of %d images at the best of %s torch threads (%d)"
                             % ("beam_search(%d, end_id=2)" % beam if beam > 1 else "greedy_sample", n, B, cands, threads))
        return common
    if workload == "inception":
        from oracle import inception as OI
        ep, eb = OI.init_inception_params(E, generator=gen)
        state = {}

        def step(images, caps, lengths):
            bufs = eb
            pooled = OI.inception_forward(ep, bufs, images, training=True)
            feats, tape = OE.head_forward(ep, bufs, pooled, training=True)
            loss, grads, d_feat, _ = OT.decoder_loss_and_grads(dp, feats, caps, lengths, Lh)
            hg = OE.head_backward(ep, tape, d_feat)
            grads = dict(grads)
            grads.update(hg)
            OT.clamp_(grads, 0.1)
            allp = {k: ep[k] for k in hg}
            allp.update(dp)
            OT.adam_step_(allp, grads, state, lr=1e-3)
            return loss
    else:
        ep, eb = OE.init_encoder_params(E, OE.RESNET152, generator=gen)
        state = {}

        def step(images, caps, lengths):
            return OT.full_step(ep, eb, dp, images, caps, lengths, state)

    # The box gives this job a CPU quota well below os.cpu_count() (16 of 256 hardware threads on the 1-GPU boxes):
    # torch's default thread count oversubscribes it ~10x.  Take the best of a short thread-count probe.
    pb = 16
    pim, pcaps, plen = batch(pb)
    rate16, threads = _thread_probe(torch, lambda: step(pim, pcaps, plen), pb, cands)
    torch.set_num_threads(threads)
    B, n = wl["batch"], 3 if workload == "train" else 2
    images, caps, lengths = batch(B)
    step(images, caps, lengths)
    t0 = time.perf_counter()
    for _ in range(n):
        step(images, caps, lengths)
    dt = time.perf_counter() - t0
    torch.set_num_threads(default_threads)
    rate64 = B * n / dt
    # `value` is the rate at the WORKLOAD's batch (64: like for like with the GPU line).  The oracle is slower per image there than
    # at the probe's batch 16 on these hosts -- with a CPU quota of 16 cores the conv stack's batch-64 working set (a layer-1
    # activation is 64 x 256 x 56 x 56 x 4 B = 205 MB, im2col buffers on top) leaves the last-level-cache share of those cores, at
    # batch 16 it does not -- so the batch-16 rate rides along as an extra
    common.update(value=round(rate64, 2), unit="images/sec", threads=threads, images_per_sec_batch64=round(rate64, 2))
    common["images_per_sec_batch%d" % pb] = round(rate16, 2)
    common["sample"] = ("CPU oracle (%s, torch-CPU fp32) on the same shapes: %d timed steps at batch %d (= value) and one at batch %d "
                        "(extra field), at the best of %s torch threads (%d)"
                        % ("oracle/inception.py + oracle/train_step.py" if workload == "inception" else "oracle/train_step.py full_step",
                           n, B, pb, cands, threads))
    return common


def f32_mode_rate(torch, sat, dev, wl, images, caps, lengths, steps=6, lookahead=True):
    """Secondary figure: the same step with the conv stack in the f32 PARITY mode (exact-f32 MFMA everywhere; the mode
    whose CE matches the CPU oracle to 1e-4, tests/test_gpu_parity.py)."""
    kw = {"arch": wl["arch"]} if wl["arch"] else {}
    torch.manual_seed(123)
    model = sat.ShowAndTell(wl["embed"], wl["hidden"], wl["vocab"], wl["layers"], compute_dtype="f32", **kw).to(dev).train()
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    # the SAME weights (same seed) in the bf16 throughput mode: mean CE of the first forward in both modes -- what the reduced
    # precision of the conv stack and of the decoder GEMMs costs on this batch
    torch.manual_seed(123)
    m16 = sat.ShowAndTell(wl["embed"], wl["hidden"], wl["vocab"], wl["layers"], compute_dtype="bf16", **kw).to(dev).train()
    ts16 = sat.TrainStep(m16, lr=1e-3, grad_clip=0.1)
    inv = 1.0 / sum(l - 1 for l in lengths)
    ce32 = float(ts.forward_backward((images, caps, lengths), inv).item())
    ce16 = float(ts16.forward_backward((images, caps, lengths), inv).item())
    del ts16, m16
    torch.cuda.empty_cache()
    depth = model.encoder.lookahead_depth if lookahead else 0
    batches = [images] + [images.clone() for _ in range(depth)]

    def run(n):
        out = None
        for i in range(n):
            nxt = [batches[j % (depth + 1)] for j in range(i + 1, i + 1 + depth) if j < n]
            out = ts.step(batches[i % (depth + 1)], caps, lengths, next_images=nxt or None)
        return out

    run(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = run(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"value": round(wl["batch"] * steps / dt, 1), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 3),
            "steps": steps, "final_loss": round(float(loss.item()), 4), "lookahead_depth": depth,
            "ce_first_forward_f32": round(ce32, 6), "ce_first_forward_bf16_mode": round(ce16, 6),
            "bf16_vs_f32_ce_delta_same_weights": float("%.3g" % abs(ce16 - ce32)),
            "note": "conv stack f32 (v_mfma_f32_32x32x2_f32, 157 TFLOP/s peak): the oracle-parity mode (|dCE| <= 1e-4 vs the CPU oracle), not the headline"}


def lstm_roofline(torch, sat, wl, reps=30):
    """north_star's second target: the LSTM gate GEMMs (ih + hh, forward + backward) against the MFMA roofline.  The layer-0
    calls of the step (`sat_lstm_fwd_bf16` / `sat_lstm_bwd_bf16`: x-gates GEMM, persistent recurrence, persistent backward
    recurrence, dW_ih / dW_hh / dX GEMMs) at the workload's shapes, each timed with HIP events on the stream it runs on, mean
    over `reps` back-to-back calls."""
    L = sat._lib
    lib = L.load()
    B, T, In, H = wl["batch"], wl["cap_len"] - 1, wl["embed"], wl["hidden"]
    pi = sat.PackInfo.get([T] * B, "cuda")
    N = pi.N
    k = 1.0 / H ** 0.5
    X = torch.randn(N, In, device="cuda")
    w_ih = torch.empty(4 * H, In, device="cuda").uniform_(-k, k)
    w_hh = torch.empty(4 * H, H, device="cuda").uniform_(-k, k)
    b = torch.zeros(4 * H, device="cuda")
    GA, CS, HS, HP = (torch.empty(N, c, device="cuda") for c in (4 * H, H, H, H))
    cst = torch.empty(B, H, device="cuda")
    wsb = lib.sat_lstm_fwd_ws_bytes(B, H)
    ws = torch.zeros(max(wsb, 16), dtype=torch.uint8, device="cuda")
    mixed = torch.empty(lib.sat_lstm_mixed_ws_bytes(N, In, H), dtype=torch.uint8, device="cuda")
    dHS = torch.randn(N, H, device="cuda") * 1e-3
    DG, dX = torch.empty(N, 4 * H, device="cuda"), torch.empty(N, In, device="cuda")
    dw_ih, dw_hh = torch.empty(4 * H, In, device="cuda"), torch.empty(4 * H, H, device="cuda")
    db1, db2 = torch.empty(4 * H, device="cuda"), torch.empty(4 * H, device="cuda")
    bws = lib.sat_lstm_bwd_ws_bytes_full(N, B, In, H)
    bw = torch.zeros(bws // 4, device="cuda")
    st = L.stream()

    def fwd():
        L.check(lib.sat_lstm_fwd_bf16(X.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), b.data_ptr(), b.data_ptr(), pi.bs_c, T, In, H,
                                      GA.data_ptr(), CS.data_ptr(), HS.data_ptr(), HP.data_ptr(), cst.data_ptr(), ws.data_ptr(), wsb,
                                      mixed.data_ptr(), mixed.numel(), st), "sat_lstm_fwd_bf16")

    def bwd():
        L.check(lib.sat_lstm_bwd_bf16(dHS.data_ptr(), X.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), GA.data_ptr(), CS.data_ptr(),
                                      HP.data_ptr(), pi.bs_c, T, In, H, DG.data_ptr(), dw_ih.data_ptr(), dw_hh.data_ptr(),
                                      db1.data_ptr(), db2.data_ptr(), dX.data_ptr(), bw.data_ptr(), bws, mixed.data_ptr(), mixed.numel(),
                                      st), "sat_lstm_bwd_bf16")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    t_f = timed(fwd)
    fwd()                                  # the tapes the backward reads (GA holds activated gates)
    t_b = timed(bwd)
    # ih: N x In x 4H, hh: N x H x 4H MACs forward; backward = dX + dW_ih (2 x ih) and dh + dW_hh (2 x hh)
    gf_f = 2.0 * N * 4 * H * (In + H) / 1e9
    gf = 3.0 * gf_f
    tf = gf / ((t_f + t_b) * 1e-6) / 1e3
    return {"kernel": "LSTM layer 0 of the step: sat_lstm_fwd_bf16 + sat_lstm_bwd_bf16 (x-gates GEMM on the bf16 pipe, persistent "
                      "exact-f32 recurrence forward and backward, dW_ih / dW_hh / dX on the bf16 pipe)",
            "gflop_ih_hh_fwd_bwd": round(gf, 3), "fwd_us": round(t_f, 1), "bwd_us": round(t_b, 1),
            "achieved": round(tf, 2), "unit": "TFLOP/s",
            "frac_of_f32_mfma_peak": round(tf / PEAK_F32_TFLOPS, 4), "peak_f32": PEAK_F32_TFLOPS,
            "frac_of_bf16_mfma_peak": round(tf / PEAK_BF16_TFLOPS, 5), "peak_bf16": PEAK_BF16_TFLOPS,
            "target": "north_star: >= 0.5 x MFMA roofline on the LSTM gate GEMMs",
            "how": "HIP events around %d back-to-back calls of each entry point, shapes of this workload (N=%d packed rows, In=%d, H=%d)"
                   % (reps, N, In, H)}


def vocab_step_roofline(torch, sat, wl, rows, reps=30):
    """The decode loop's dominant kernel: the vocab projection of ONE step over `rows` hypotheses -- the kernel the loop runs: with
    >= 128 rows (beam decode) the three-way bf16 split on the bf16 pipe (sat_gemm_f32x3: six bf16 products per f32 product), with
    fewer (greedy) the exact-f32 MFMA GEMM."""
    L = sat._lib
    lib = L.load()
    H, V = wl["hidden"], wl["vocab"]
    ldl = (V + 3) // 4 * 4
    x = torch.randn(rows, H, device="cuda")
    w = torch.empty(V, H, device="cuda").uniform_(-0.1, 0.1)
    b = torch.zeros(V, device="cuda")
    out = torch.zeros(rows, ldl, device="cuda")
    st = L.stream()
    x3 = rows >= 128 and os.environ.get("SAT_BEAM_X3", "1") != "0" and lib.sat_gemm_f32x3_packed_bytes(V, H) > 0 and V % 4 == 0
    if x3:
        packed = torch.empty(lib.sat_gemm_f32x3_packed_bytes(V, H), dtype=torch.uint8, device="cuda")
        L.check(lib.sat_gemm_f32x3_pack(w.data_ptr(), V, H, packed.data_ptr(), st), "sat_gemm_f32x3_pack")

        def fn():
            L.check(lib.sat_gemm_f32x3(x.data_ptr(), H, packed.data_ptr(), b.data_ptr(), out.data_ptr(), ldl, rows, V, H, st), "sat_gemm_f32x3")
    else:
        def fn():
            L.check(lib.sat_vocab_logits_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), rows, H, V, out.data_ptr(), ldl, st), "sat_vocab_logits_fwd")

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    gf = 2.0 * rows * H * V / 1e9                         # the f32 product's flops
    nbytes = 4.0 * (V * H + rows * H + rows * V)
    if x3:
        nbytes = 6.0 * V * H + 4.0 * (rows * H + rows * V)      # three bf16 copies of the weights
        return {"kernel": "sat_gemm_f32x3 of one decode step: [%d x %d] x [%d x %d]^T, f32 accuracy from a three-way bf16 split of both operands "
                          "(6 bf16 MFMA products per f32 product, hi*hi and the corrections in separate f32 accumulators)" % (rows, H, V, H),
                "bound": "mfma", "achieved": round(6.0 * gf / (us * 1e-6) / 1e3, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                "frac": round(6.0 * gf / (us * 1e-6) / 1e3 / PEAK_BF16_TFLOPS, 4), "avg_launch_us": round(us, 2),
                "executed_bf16_gflop_per_launch": round(6.0 * gf, 3), "algorithmic_gflop_per_launch": round(gf, 3),
                "f32_product_tflops": round(gf / (us * 1e-6) / 1e3, 2), "f32_product_frac_of_f32_mfma_peak": round(gf / (us * 1e-6) / 1e3 / PEAK_F32_TFLOPS, 4),
                "algorithmic_bytes_per_launch": int(nbytes), "gbytes_per_s": round(nbytes / (us * 1e-6) / 1e9, 1)}
    return {"kernel": "sat_vocab_logits_fwd of one decode step: [%d x %d] x [%d x %d]^T, exact-f32 MFMA" % (rows, H, V, H),
            "bound": "mfma", "achieved": round(gf / (us * 1e-6) / 1e3, 2), "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s",
            "frac": round(gf / (us * 1e-6) / 1e3 / PEAK_F32_TFLOPS, 4), "avg_launch_us": round(us, 2),
            "algorithmic_gflop_per_launch": round(gf, 3), "algorithmic_bytes_per_launch": int(nbytes),
            "gbytes_per_s": round(nbytes / (us * 1e-6) / 1e9, 1)}


def selftest_launch(torch, rank, world, fail_rank=-1):
    """The multi-rank skeleton of main() on the CPU (tests/test_bench_launch.py): same env contract, barrier + timed
    region + barrier, MAX over ranks, ONE JSON line from rank 0."""
    import torch.distributed as dist
    if rank == fail_rank:
        sys.exit(7)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"selftest": True, "n_gpus": world, "max_dt": float(t.item())}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def attach_traffic(out, TRAFFIC_FILE=TRAFFIC_FILE):
    # HBM bytes per conv launch come from separate rocprofv3 --pmc passes (tools/run_gpu_pmc.sh -> profiles/): only a
    # measurement taken on THIS library build is quoted -- a file older than libsat_hip.so describes other kernels
    if not os.path.exists(TRAFFIC_FILE):
        out["roofline"]["traffic_note"] = "null: no PMC traffic file for this round (%s)" % os.path.relpath(TRAFFIC_FILE, ROOT)
        return
    with open(TRAFFIC_FILE) as f:
        tj = json.load(f)
    lib_stamp = tj.get("libsat_hip_sha16")
    import hashlib
    with open(LIB_FILE, "rb") as f:
        cur = hashlib.sha256(f.read()).hexdigest()[:16]
    if lib_stamp != cur:
        out["roofline"]["traffic_note"] = ("null: %s was measured on library build %s, this run is build %s (re-run tools/run_gpu_pmc.sh)"
                                           % (os.path.relpath(TRAFFIC_FILE, ROOT), lib_stamp, cur))
    else:
        out["roofline"]["traffic"] = round(tj["hbm_bytes_per_launch_corrected"])
        out["roofline"]["traffic_unit"] = "HBM bytes per launch (FETCH_SIZE x2 + WRITE_SIZE, %s)" % os.path.relpath(TRAFFIC_FILE, ROOT)


def conv_roofline(torch, sat, model, images, wl, what, groups=1):
    """`groups` > 1: the grouped program of the look-ahead (every launch covers `groups` batches): algorithmic flops per launch
    and launch durations are those of the launches the timed steps run"""
    conv_ms, n_conv = conv_in_sequence_us(torch, model, images, groups=groups)
    if wl["arch"] == "inception_v3":
        conv_flops = 2.0 * INCEPTION_V3_CONV_MACS * wl["batch"]
    else:
        conv_flops = sat.conv_flops(sat.RESNET152, wl["image"], wl["image"]) * wl["batch"]
    conv_flops *= groups
    achieved = conv_flops / (conv_ms * 1e-3) / 1e12
    if groups > 1:
        what = "pass of the grouped program = %d batches of %d images" % (groups, wl["batch"])
    return {"bound": "mfma", "batches_per_launch": groups,
            "kernel": "bf16 implicit-GEMM conv launches (%d per %s: conv_pw_kernel for the 3x3 convs, conv_aw_kernel / conv_ap_kernel / conv_xp_kernel / conv_glds_kernel ring variants for the 1x1 convs, conv_stem_kernel; per geometry the variant the committed table show-and-tell_amd/tune/gfx950.json names -- no timing at start-up)" % (n_conv, what),
            "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": None,
            "algorithmic_gflop_per_launch": round(conv_flops / n_conv / 1e9, 3),
            "avg_launch_us": round(conv_ms * 1e3 / n_conv, 2),
            "algorithmic_gflop_per_step": round(conv_flops / groups / 1e9, 1), "ms_per_step_in_kernel": round(conv_ms / groups, 3),
            "ms_per_program_pass_in_kernel": round(conv_ms, 3),
            "how": "per-launch dispatch timestamps (HIP events attached to each conv launch), whole encoder program in sequence, mean of 3 passes"}


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.selftest_launch:
        return selftest_launch(torch, rank, world, args.selftest_fail_rank)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    ndev = torch.cuda.device_count()
    dev_index = local_rank
    if local_rank >= ndev:
        # rehearsal of the N > 1 branch on a box with fewer devices than ranks: only on request, never silently
        if os.environ.get("SAT_BENCH_SHARE_DEVICE", "0") != "1" or ndev < 1:
            raise SystemExit("rank %d needs cuda:%d but only %d device(s) are visible (SAT_BENCH_SHARE_DEVICE=1 lets ranks share)" % (rank, local_rank, ndev))
        dev_index = local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    import torch.distributed as dist
    use_dist = world > 1 or args.force_dist
    backend = os.environ.get("SAT_BENCH_BACKEND", "nccl")
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # RCCL announces itself on stdout ("Librccl path : ..."): keep stdout for the ONE JSON line
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            if backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
        if world > 1 and timed_tuning() and not os.environ.get("SAT_TUNE_FILE"):
            # (only with SAT_AUTOTUNE=1 / force: by default every rank takes its kernel variants from the committed table,
            # show-and-tell_amd/tune/gfx950.json, and nothing is timed)
            # ONE autotune per node, not one per rank: local rank 0 times the conv variants first (alone on its device, nothing of
            # another rank's competing for the host or -- when ranks share a device -- for the GPU), writes the table, and the
            # other ranks load it: every rank runs the same kernels, so the frozen stack sums in the same order on every rank
            os.environ["SAT_TUNE_FILE"] = os.path.join(tempfile.gettempdir(), "sat_tune_%s_%s.json"
                                                       % (os.environ.get("MASTER_PORT", "0"), os.environ.get("TORCHELASTIC_RUN_ID", "run")))
            if rank == 0 and os.path.exists(os.environ["SAT_TUNE_FILE"]):
                os.remove(os.environ["SAT_TUNE_FILE"])

    sat = importlib.import_module("show-and-tell_amd")
    wl = dict(WORKLOADS[args.workload])
    wl["beam"] = args.beam
    if args.workload == "decode":
        return run_decode(args, torch, dist, sat, wl, dev, rank, world, use_dist, backend)

    kw = {"arch": wl["arch"]} if wl["arch"] else {}
    torch.manual_seed(123)                                           # config.py:15; same weights on every rank
    model = sat.ShowAndTell(wl["embed"], wl["hidden"], wl["vocab"], wl["layers"], compute_dtype="bf16", **kw).to(dev).train()
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    dp = sat.DataParallelStep(ts)
    if args.force_dist:
        dp.world = 2          # take the multi-rank code path (async bucket all-reduces) on the single rank
        dp.cap_lookahead()    # ... with the look-ahead depth that path runs at
    images, caps, lengths = synth_batch(torch, wl["batch"], wl["vocab"], wl["cap_len"], wl["image"], dev, 123 + rank)
    global_tokens = world * sum(l - 1 for l in lengths)
    if use_dist and world > 1 and timed_tuning():
        # build (and autotune) the conv-stack programs on rank 0 first, then everywhere from rank 0's table
        if rank == 0:
            model.encoder._program(images)
            if args.lookahead:
                model.encoder.build_lookahead(images)
            torch.cuda.synchronize()
        dist.barrier()

    # synthetic image batches in rotation: with look-ahead (default) a step hands the next `lookahead_depth` (3) batches' images to the engine,
    # which runs their frozen conv stacks on side streams next to each other and under this batch's decoder work
    # (EncoderCNN.prefetch).  Warm-up leaves nothing in flight, so the timed region holds exactly K conv-stack passes and K
    # decoder passes: pipeline fill (step 1's stack runs alone, on the main stream) and drain are inside it.
    depth = model.encoder.lookahead_depth
    groups = model.encoder.lookahead_groups                                    # batches per grouped program run
    n_streams = model.encoder.lookahead_streams or max(1, depth // groups)
    nb = depth + 1
    batches = [images] + [synth_batch(torch, wl["batch"], wl["vocab"], wl["cap_len"], wl["image"], dev, 977 * (k + 1) + rank)[0]
                          for k in range(nb - 1)]

    def run_steps(n):
        out = None
        for i in range(n):
            nxt = [batches[j % nb] for j in range(i + 1, i + 1 + depth) if j < n] if args.lookahead else None
            out = dp.step((batches[i % nb], caps, lengths), global_tokens, next_images=nxt or None)
        return out

    if args.lookahead:
        model.encoder.build_lookahead(images)          # op programs of the look-ahead instances: autotune + graph capture, before any step
    if args.warmup:
        loss = run_steps(args.warmup)
    # The timed region: EXACTLY K steps between barrier + synchronize on both sides, MAX over ranks.  K = 20 steps are 0.1 s of
    # GPU time, and boxes of the pool (and DVFS states of one box) differ by several percent, so the region is repeated and
    # the MEDIAN repetition is the reported one (every repetition starts with nothing in flight: pipeline fill and drain inside)
    last = {}
    dts = timed_regions(args, torch, dist, dev, use_dist, lambda: last.__setitem__("loss", run_steps(args.steps)))
    dt = sorted(dts)[len(dts) // 2]
    final_loss = float(last["loss"].item())
    ts.check_ids()
    if args.dump_outputs and rank == 0:
        # what a caller of the step receives: the last step's loss and the trainable parameters it updated (the flat buffer Adam writes)
        fp = ts.flat
        dump_outputs(args.dump_outputs, [("loss", last["loss"])] +
                     [("param." + name, fp.params[o:o + n].view(shape)) for name, (o, n, shape) in fp.slices.items()])

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = world * wl["batch"] * args.steps / dt
        out = {
            "metric": wl["metric"], "value": round(value, 2), "unit": wl["unit"], "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "repeats": {"n": len(dts), "stat": "median of n timed regions of `steps` steps each",
                        "images_per_sec_min": round(world * wl["batch"] * args.steps / max(dts), 1),
                        "images_per_sec_max": round(world * wl["batch"] * args.steps / min(dts), 1)},
            "config": {"workload": wl["name"],
                       "global_batch": world * wl["batch"], "parallelism": "dp%d" % world,
                       "precision": "conv stack bf16 MFMA / f32 accumulate; vocab projection + its gradients and the LSTM's batched GEMMs on the bf16 MFMA pipe from bf16 operand copies (f32 accumulate, f32 logits / outputs / master weights); LSTM recurrence, head, CE, Adam f32.  "
                                    "Stated CE tolerance of this mode against the f32 CPU oracle: %.0e on trained-like (well-conditioned) weights (tests/test_gpu_parity_full.py: 8.5e-4 measured at this size).  The kernel variants -- and with them every summation order -- come from the committed table show-and-tell_amd/tune/gfx950.json, so the delta no longer changes from run to run or process to process (tests/test_gpu_reproducible.py); on THIS line's He-initialised random weights `f32_parity_mode.bf16_vs_f32_ce_delta_same_weights` is a property of the table: 4.1e-4 ... 2.3e-3 on the five tables measured in round 5, 1.0e-3 on the geometry-only defaults (round 4, a stopwatch picking: 7e-5 ... 1.4e-3) -- summation-order noise of the BatchNorm statistics amplified through 152 train-mode BatchNorm layers without a trained model's conditioning; the 1e-4 bar of north_star is met by the f32 parity mode (`f32_parity_mode` below)" % BF16_CE_TOL,
                       "ce_tolerance_vs_f32_oracle": BF16_CE_TOL,
                       "schedule": ("encoder look-ahead depth %d on %d side stream%s: the frozen conv stacks of batches i+1..i+%d run on side streams next to each other and under batch i's head/decoder/backward/Adam%s%s; "
                                    "K conv passes + K decoder passes inside the timed region, fill and drain included"
                                    % (depth, n_streams, "" if n_streams == 1 else "s", depth,
                                       (", %d batches per grouped program run (every launch of the stack covers %d batches, per-batch BatchNorm statistics: bit-identical per batch)" % (groups, groups)) if groups > 1 else "",
                                       " (the data-parallel step spreads the runs over fewer streams: the collective's stream needs a hardware queue, trainer.DataParallelStep.cap_lookahead)" if n_streams < max(1, depth // groups) else "")) if args.lookahead
                                   else "strictly sequential steps",
                       "lookahead_depth": depth if args.lookahead else 0, "lookahead_streams": n_streams if args.lookahead else 0,
                       "lookahead_groups": groups if args.lookahead else 0,
                       "backend": (backend if backend != "nccl" else "nccl (RCCL)") if use_dist else None,
                       "final_loss": round(final_loss, 4)},
        }
        if args.full:
            out["roofline"] = conv_roofline(torch, sat, model, images, wl, "step", groups if args.lookahead else 1)
            if groups > 1 and args.lookahead:
                # the same figure for the ungrouped program (one batch per launch: what a strictly sequential step runs)
                seq = conv_roofline(torch, sat, model, images, wl, "step", 1)
                out["roofline"]["one_batch_per_launch"] = {k: seq[k] for k in ("achieved", "frac", "avg_launch_us", "ms_per_step_in_kernel")}
            if args.workload == "train":
                attach_traffic(out)
            else:
                attach_traffic(out, os.path.join(ROOT, "profiles", "r05_cfg3_pmc_traffic.json"))      # the same passes on configs[3]
            if world == 1 and args.lookahead and not args.no_f32_mode:
                # the same K steps with strictly sequential steps (what --no-lookahead times), for comparison in the same process
                def seq_steps(n):
                    o = None
                    for i in range(n):
                        o = dp.step((batches[i % nb], caps, lengths), global_tokens)
                    return o
                seq_steps(2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seq_steps(args.steps)
                torch.cuda.synchronize()
                dts_ = time.perf_counter() - t0
                out["sequential_schedule"] = {"value": round(wl["batch"] * args.steps / dts_, 1), "unit": "images/sec",
                                              "ms_per_step": round(dts_ / args.steps * 1e3, 3),
                                              "note": "same engine, no look-ahead: batch i+1's conv stack starts after batch i's optimizer step"}
            if world == 1 and not args.no_f32_mode:
                del dp, ts, model
                torch.cuda.empty_cache()
                out["roofline_lstm"] = lstm_roofline(torch, sat, wl)
                out["f32_parity_mode"] = f32_mode_rate(torch, sat, dev, wl, images, caps, lengths, lookahead=args.lookahead)
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(torch, 123, wl, args.workload)
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def timed_tuning():
    """SAT_AUTOTUNE=1 / force: kernel variants of geometries outside the committed table are chosen by timing (tune.py)"""
    return os.environ.get("SAT_AUTOTUNE", "").strip().lower() in ("1", "time", "force")


def timed_regions(args, torch, dist, dev, use_dist, region):
    """`--repeats` timed regions, each bracketed by barrier + synchronize on both sides, MAX over ranks"""
    dts = []
    for _ in range(max(1, args.repeats)):
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        region()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        dt = time.perf_counter() - t0
        if use_dist:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        dts.append(dt)
    return dts


def run_decode(args, torch, dist, sat, wl, dev, rank, world, use_dist, backend):
    """BASELINE configs[4]: decode of 64 images per GPU per step -- eval-mode encoder (eval.py:65,93) + `model.sample` /
    beam search (eval.py:99; `--beam`) -- captions/sec.  Shards by image: every rank decodes its own batch, no exchange step."""
    B, beam = wl["batch"], int(args.beam)
    torch.manual_seed(123)
    model = sat.ShowAndTell(wl["embed"], wl["hidden"], wl["vocab"], wl["layers"], compute_dtype="bf16").to(dev)
    depth = model.encoder.lookahead_depth
    nb = depth + 1
    batches = [synth_batch(torch, B, wl["vocab"], wl["cap_len"], wl["image"], dev, 123 + 977 * k + rank)[0] for k in range(nb)]
    # random-init weights (no checkpoints offline): give the 155 BatchNorms running statistics that match the data, as a trained
    # model's do -- a few dozen train-mode passes (momentum 0.1) -- so that the eval-mode stack computes finite features
    model.train()
    with torch.no_grad():
        for i in range(48):
            model.encoder(batches[i % nb])
    model.eval()
    if use_dist and world > 1 and timed_tuning():
        if rank == 0:
            model.encoder._program(batches[0])
            if args.lookahead:
                model.encoder.build_lookahead(batches[0])
            torch.cuda.synchronize()
        dist.barrier()
    if args.lookahead:
        model.encoder.build_lookahead(batches[0])

    def decode(f):
        return model.decoder.sample_beam(f, beam, end_id=2) if beam > 1 else model.decoder.sample(f)

    def run_steps(n):
        ids = None
        with torch.no_grad():
            for i in range(n):
                if args.lookahead:             # the next batches' stacks run ahead, two batches per program run (eval mode: concatenated)
                    model.encoder.prefetch_many([batches[j % nb] for j in range(i + 1, i + 1 + depth) if j < n],
                                                own_stack=not model.encoder._is_in_flight(batches[i % nb]))      # (the first step runs its own stack beside them)
                ids = decode(model.encoder(batches[i % nb]))
        return ids

    run_steps(max(args.warmup, 1))
    last = {}
    dts = timed_regions(args, torch, dist, dev, use_dist, lambda: last.__setitem__("ids", run_steps(args.steps)))
    dt = sorted(dts)[len(dts) // 2]
    ids = last["ids"]                  # the captions of the last timed step
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, [("ids", ids)])
    if args.full:
        finite = bool(torch.isfinite(model.encoder(batches[0])).all().item())
    if rank == 0:
        out = {"metric": "captions/sec (beam_size=%d decode, encoder included)" % beam if beam > 1 else "captions/sec (greedy decode, encoder included)",
               "value": round(world * B * args.steps / dt, 2), "unit": "captions/sec", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
               "repeats": {"n": len(dts), "stat": "median of n timed regions of `steps` steps each",
                           "captions_per_sec_min": round(world * B * args.steps / max(dts), 1),
                           "captions_per_sec_max": round(world * B * args.steps / min(dts), 1)},
               "config": {"workload": wl["name"], "global_batch": world * B, "parallelism": "dp%d (sharded by image, no collective in the decode)" % world,
                          "beam_size": beam, "end_id": 2 if beam > 1 else None, "steps_per_caption": 20,
                          "precision": "conv stack bf16 MFMA / f32 accumulate (eval mode: BatchNorm + add + ReLU in the conv epilogues); head, LSTM step, vocab projection, log-softmax / top-k exact f32",
                          "schedule": ("encoder look-ahead depth %d: the conv stacks of batches i+1..i+%d run on side streams under batch i's decode loop, %d batches per program run (eval mode: the batches of a run concatenate)" % (depth, depth, model.encoder.lookahead_groups))
                                      if args.lookahead else "strictly sequential batches",
                          "backend": (backend if backend != "nccl" else "nccl (RCCL)") if use_dist else None,
                          "ids_shape": list(ids.shape)}}
        if args.full:
            out["config"]["features_finite"] = finite
            out["roofline"] = conv_roofline(torch, sat, model, batches[0], wl, "batch", model.encoder.lookahead_groups if args.lookahead else 1)
            out["roofline"]["traffic_note"] = "null: the PMC traffic passes of this round were taken on the headline workload (profiles/r05_pmc_traffic.json)"
            if world == 1 and not args.no_f32_mode:
                feats = model.encoder(batches[0]).clone()

                def t_of(fn, n=10):
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / n * 1e3

                with torch.no_grad():
                    out["breakdown_ms"] = {"encoder_eval": round(t_of(lambda: model.encoder(batches[0])), 3),
                                           "greedy_decode_20_steps": round(t_of(lambda: model.decoder.sample(feats)), 3),
                                           "beam%d_decode_20_steps" % max(beam, 2): round(t_of(lambda: model.decoder.sample_beam(feats, max(beam, 2), end_id=2)), 3)}
                out["roofline_decode"] = vocab_step_roofline(torch, sat, wl, B * beam)
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(torch, 123, wl, "decode")
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
