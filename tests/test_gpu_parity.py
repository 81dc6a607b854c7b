"""GPU (MI355X) parity of the HIP path against (a) the golden vectors produced by the reference's own
`models.DecoderRNN` + train.py arithmetic and (b) the CPU oracle, on identical seeded inputs, plus
size-independent properties at BASELINE.json's cfg-2 size.  Everything goes through libsat_hip.so."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
from oracle import decoder as OD  # noqa: E402
from oracle import encoder as OE  # noqa: E402
from oracle import train_step as OT  # noqa: E402

TINY = dict(layers=(1, 1, 1, 1), width=8)
SMALL = dict(layers=(2, 1, 2, 1), width=16)


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: z[k] for k in z.files}


def golden_setup(g):
    E, H, V, Lh, B, T = [int(x) for x in g["dims"]]
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(int(g["seed"])))
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    return dec.cuda(), params, (E, H, V, Lh, B, T)


@pytest.mark.parametrize("name", ["G1_dec_fwd_bwd_small.npz", "G2_dec_varlen_small.npz", "G5_dec_L2.npz"])
def test_decoder_autograd_path_matches_reference_goldens(golden_dir, name):
    """drop-in path: DecoderRNN.forward -> torch CE -> loss.backward() exactly as train.py:134-144 drives it"""
    g = load(golden_dir, name)
    dec, params, (E, H, V, Lh, B, T) = golden_setup(g)
    feats = torch.from_numpy(g["features"]).cuda().requires_grad_(True)
    caps = torch.from_numpy(g["captions"]).cuda()
    lengths = [int(x) for x in g["lengths"]]
    targets, l1 = sat.pack_targets(caps, lengths)                      # train.py:134-135
    assert np.array_equal(targets.cpu().numpy(), g["targets"])
    dec.zero_grad()
    out = dec(feats, caps[:, :-1], l1)                                 # train.py:139
    assert out.shape == (sum(l1), V)
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["logits"], rtol=0, atol=1e-5)
    loss = torch.nn.CrossEntropyLoss()(out, targets)                   # train.py:143
    assert abs(loss.item() - float(g["loss"])) < 1e-4                  # north_star: CE within 1e-4 fp32
    loss.backward()                                                    # train.py:144
    np.testing.assert_allclose(feats.grad.cpu().numpy(), g["d_features"], rtol=1e-3, atol=1e-7)
    for k, p in dec.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g["grad." + k], rtol=1e-3, atol=1e-7, err_msg=k)


def _decoder_only_model(g):
    E, H, V, Lh, B, T = [int(x) for x in g["dims"]]
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY, compute_dtype="f32")
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(int(g["seed"])))
    model.decoder.load_state_dict(params)
    return model.cuda().train()


def test_fused_trainstep_three_adam_steps_match_reference(golden_dir):
    """fused path: HIP CE + backward + clamp + Adam, decoder-only (cached features), vs torch.optim.Adam goldens"""
    g = load(golden_dir, "G1_dec_fwd_bwd_small.npz")
    model = _decoder_only_model(g)
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    feats = torch.from_numpy(g["features"]).cuda()
    caps = torch.from_numpy(g["captions"]).cuda()
    lengths = [int(x) for x in g["lengths"]]
    for it in range(3):
        loss = ts.step(feats, caps, lengths)
        assert abs(loss.item() - float(g["losses"][it])) < 1e-4
        if it == 0:
            np.testing.assert_allclose(ts.last_d_features.cpu().numpy(), g["d_features"], rtol=1e-3, atol=1e-7)
        if it + 1 in (1, 3):
            for k, p in model.decoder.named_parameters():
                np.testing.assert_allclose(p.detach().cpu().numpy(), g["param_after%d.%s" % (it + 1, k)], rtol=0,
                                           atol=2e-6, err_msg="%s after %d" % (k, it + 1))


def test_dropin_loop_with_fused_clamp_adam_matches_reference_goldens(golden_dir):
    """drop-in path (train.py:134-146 as written: forward, torch CE, loss.backward()) with `sat.FusedClampAdam` standing in for
    clip_gradient + optim.Adam.step(): losses and parameters after 1 and 3 steps vs the reference-generated goldens"""
    g = load(golden_dir, "G1_dec_fwd_bwd_small.npz")
    dec, params, (E, H, V, Lh, B, T) = golden_setup(g)
    opt = sat.FusedClampAdam(dec.parameters(), lr=1e-3, clip=0.1)
    feats = torch.from_numpy(g["features"]).cuda()
    caps = torch.from_numpy(g["captions"]).cuda()
    lengths = [int(x) for x in g["lengths"]]
    targets, l1 = sat.pack_targets(caps, lengths)
    crit = torch.nn.CrossEntropyLoss()
    for it in range(3):
        dec.zero_grad()                                                # train.py:137 (drops the flat views: step() copies in)
        loss = crit(dec(feats, caps[:, :-1], l1), targets)
        assert abs(loss.item() - float(g["losses"][it])) < 1e-4
        loss.backward()
        opt.step()
        if it + 1 in (1, 3):
            for k, p in dec.named_parameters():
                np.testing.assert_allclose(p.detach().cpu().numpy(), g["param_after%d.%s" % (it + 1, k)], rtol=0,
                                           atol=2e-6, err_msg="%s after %d" % (k, it + 1))


@pytest.mark.parametrize("name", ["G2_dec_varlen_small.npz", "G5_dec_L2.npz"])
def test_fused_trainstep_grads_varlen_and_two_layers(golden_dir, name):
    g = load(golden_dir, name)
    model = _decoder_only_model(g)
    ts = sat.TrainStep(model)
    feats, caps = torch.from_numpy(g["features"]).cuda(), torch.from_numpy(g["captions"]).cuda()
    lengths = [int(x) for x in g["lengths"]]
    n_tok = sum(l - 1 for l in lengths)
    loss = ts.forward_backward((feats, caps, lengths), 1.0 / n_tok)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    for k, p in model.decoder.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g["grad." + k], rtol=1e-3, atol=1e-7, err_msg=k)


def test_cfg1_summary_and_argmax(golden_dir):
    g = load(golden_dir, "G3_dec_cfg1_summary.npz")
    dec, params, (E, H, V, Lh, B, T) = golden_setup(g)
    feats, caps = torch.from_numpy(g["features"]).cuda(), torch.from_numpy(g["captions"]).cuda()
    lengths = [int(x) for x in g["lengths"]]
    targets, l1 = sat.pack_targets(caps, lengths)
    out = dec(feats, caps[:, :-1], l1)
    loss = torch.nn.functional.cross_entropy(out, targets)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    assert np.array_equal(out.argmax(1).cpu().numpy(), g["argmax"])          # bit-exact token ids
    np.testing.assert_allclose(out[:, :64].detach().cpu().numpy(), g["logits_head"], rtol=0, atol=1e-5)
    loss.backward()
    for k, p in dec.named_parameters():
        n = float(p.grad.double().norm().item())
        assert abs(n - float(g["gradnorm." + k])) <= 1e-4 * float(g["gradnorm." + k]) + 1e-9, k


@pytest.mark.parametrize("name", ["G1_dec_fwd_bwd_small.npz", "G3_dec_cfg1_summary.npz", "G5_dec_L2.npz"])
def test_greedy_decode_ids_bit_exact(golden_dir, name):
    g = load(golden_dir, name)
    dec, params, (E, H, V, Lh, B, T) = golden_setup(g)
    ids = dec.eval().sample(torch.from_numpy(g["features"]).cuda(), None)
    assert ids.shape == (B, 20) and ids.dtype == torch.int64
    assert np.array_equal(ids.cpu().numpy(), g["greedy_ids"])


@pytest.mark.parametrize("name", ["G9_dec_sample_states_L1.npz", "G9_dec_sample_states_L2.npz"])
def test_sample_honours_the_initial_state(golden_dir, name):
    """models.py:56,61 hands `states` to the LSTM; eval.py:82-89 passes a stacked [2,B,H] tensor.  G9 = the reference decoder's
    own submodules from a seeded non-zero (h0, c0): bit-exact ids for the tuple form, the stacked form (one layer: [2,B,H];
    any: [2,L,B,H]), through ShowAndTell-style `sample(features, state)`; any other shape raises instead of decoding from zeros"""
    g = load(golden_dir, name)
    dec, params, (E, H, V, Lh, B, T) = golden_setup(g)
    dec.eval()
    feats = torch.from_numpy(g["features"]).cuda()
    h0, c0 = torch.from_numpy(g["h0"]).cuda(), torch.from_numpy(g["c0"]).cuda()
    ids = dec.sample(feats, (h0, c0))
    assert np.array_equal(ids.cpu().numpy(), g["greedy_ids"])
    assert np.array_equal(ids.cpu().numpy(), OD.greedy_sample(params, torch.from_numpy(g["features"]), Lh,
                                                              states=(h0.cpu(), c0.cpu())).numpy())
    assert np.array_equal(dec.sample(feats, torch.stack([h0, c0])).cpu().numpy(), g["greedy_ids"])      # [2,L,B,H]
    if Lh == 1:
        assert np.array_equal(dec.sample(feats, torch.stack([h0[0], c0[0]])).cpu().numpy(), g["greedy_ids"])   # eval.py:89
        assert np.array_equal(dec.sample(feats, (h0[0], c0[0])).cpu().numpy(), g["greedy_ids"])
    assert np.array_equal(dec.sample(feats, None).cpu().numpy(), g["greedy_ids_zero_state"])
    assert np.array_equal(dec.sample(feats, torch.zeros(2, Lh, B, H, device="cuda")).cpu().numpy(), g["greedy_ids_zero_state"])
    # the state is not modified by the call
    assert torch.equal(h0.cpu(), torch.from_numpy(g["h0"])) and torch.equal(c0.cpu(), torch.from_numpy(g["c0"]))
    for bad in ((h0[:, :-1], c0[:, :-1]), (h0,), torch.zeros(3, B, H, device="cuda"), (h0[..., :-1], c0[..., :-1]),
                torch.zeros(2, B + 1, H, device="cuda")):
        with pytest.raises((ValueError, TypeError)):
            dec.sample(feats, bad)
    with pytest.raises(TypeError):
        dec.sample(feats, "zeros")
    # models.py:67 `sampled_ids.squeeze()`: one image gives [20]
    one = dec.sample(feats[:1], (h0[:, :1], c0[:, :1]))
    assert one.shape == (20,) and np.array_equal(one.cpu().numpy(), g["greedy_ids"][0])


@pytest.mark.parametrize("name", ["G1_dec_fwd_bwd_small.npz", "G3_dec_cfg1_summary.npz", "G5_dec_L2.npz"])
def test_beam_width_one_reproduces_golden_greedy_ids(golden_dir, name):
    """sample_beam has no reference counterpart (model2.py:113-114 is a stub); width 1 must be the pinned greedy ids"""
    g = load(golden_dir, name)
    dec, params, (E, H, V, Lh, B, T) = golden_setup(g)
    ids = dec.eval().sample_beam(torch.from_numpy(g["features"]).cuda(), beam_size=1)
    assert np.array_equal(ids.cpu().numpy(), g["greedy_ids"])


@pytest.mark.parametrize("name,K,end_id", [("G1_dec_fwd_bwd_small.npz", 5, None), ("G5_dec_L2.npz", 3, None),
                                           ("G1_dec_fwd_bwd_small.npz", 4, "auto"), ("G3_dec_cfg1_summary.npz", 5, 2)])
def test_beam_search_matches_oracle(golden_dir, name, K, end_id):
    g = load(golden_dir, name)
    dec, params, (E, H, V, Lh, B, T) = golden_setup(g)
    feats = torch.from_numpy(g["features"])
    if end_id == "auto":                   # a token the search really emits, so finished hypotheses occur
        end_id = int(OD.beam_search(params, feats, K, Lh)[0][0, 0, 2])
    ref_ids, ref_scores = OD.beam_search(params, feats, K, Lh, end_id=end_id)
    ids, scores = dec.eval().sample_beam(feats.cuda(), beam_size=K, end_id=end_id, return_all=True)
    assert ids.shape == (B, K, 20) and ids.dtype == torch.int64
    assert np.array_equal(ids.cpu().numpy(), ref_ids.numpy())
    np.testing.assert_allclose(scores.cpu().numpy(), ref_scores.numpy(), rtol=0, atol=1e-4)
    best = dec.sample_beam(feats.cuda(), beam_size=K, end_id=end_id)
    assert torch.equal(best, ids[:, 0])


def test_wide_beam_decode_matches_oracle():
    """the WIDE decode path (>= 128 hypothesis rows, one LSTM layer: the gate GEMM over [x | h] dealt over K slices, the vocab
    projection on the bf16 pipe from a three-way split of both operands -- sat_gemm_x3.hip -- the merge launch moving (h, c)) against
    the CPU oracle: ids bit-exact, scores to 1e-4; then once more in a fresh process on the exact-f32 pipe (SAT_BEAM_X3=0)"""
    gen = torch.Generator().manual_seed(99)
    E, H, V, B, K = 64, 256, 1000, 32, 5
    params = OD.init_decoder_params(E, H, V, 1, generator=gen)
    params["linear.weight"] = params["linear.weight"] * 6.0      # a trained projection separates its logits: no 1e-6 ties
    feats = torch.randn(B, E, generator=gen)
    dec = sat.DecoderRNN(E, H, V, 1)
    dec.load_state_dict(params)
    dec.cuda().eval()
    ref_ids, ref_scores = OD.beam_search(params, feats, K, 1, end_id=2)
    ids, scores = dec.sample_beam(feats.cuda(), beam_size=K, end_id=2, return_all=True)
    assert np.array_equal(ids.cpu().numpy(), ref_ids.numpy())
    np.testing.assert_allclose(scores.cpu().numpy(), ref_scores.numpy(), rtol=0, atol=1e-4)
    if os.environ.get("SAT_BEAM_X3") != "0":
        import subprocess
        import sys
        here = os.path.abspath(__file__)
        r = subprocess.run([sys.executable, "-m", "pytest", here, "-q", "-x", "-m", "gpu", "-k", "test_wide_beam_decode_matches_oracle"],
                           env=dict(os.environ, SAT_BEAM_X3="0"), capture_output=True, text=True, timeout=600,
                           cwd=os.path.dirname(os.path.dirname(here)))
        assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_beam_step_ties_dead_and_finished_hypotheses():
    """sat_beam_step on hand-made logits: exact ties resolve to the lower k*V+v, -inf hypotheses never win,
    a finished hypothesis continues only with end_id at unchanged score"""
    from importlib import import_module
    L = import_module("show-and-tell_amd._lib")
    lib = L.load()
    B, K, V = 2, 3, 700
    logits = torch.zeros(B * K, V, device="cuda")                 # uniform rows: log-prob = -log(V) everywhere
    logits[4, 650] = 3.0                                          # image 1, hypothesis 1: one clear winner
    scores = torch.tensor([[0.0, 0.0, float("-inf")], [-1.0, -1.0, -0.5]], device="cuda")
    last = torch.tensor([5, 6, 7, 9, 8, 2], device="cuda")        # image 1 / hypothesis 2 ended (end_id 2)
    parent = torch.empty(B * K, dtype=torch.int32, device="cuda")
    token = torch.empty(B * K, dtype=torch.int64, device="cuda")
    out = torch.empty(B * K, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.sat_beam_step_ws_bytes(B, K), dtype=torch.uint8, device="cuda")
    L.check(lib.sat_beam_step(logits.data_ptr(), V, scores.data_ptr(), last.data_ptr(), 2, B, K, V, parent.data_ptr(),
                              token.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), st))
    parent, token, out = parent.cpu().view(B, K), token.cpu().view(B, K), out.cpu().view(B, K)
    # image 0: everything ties at -log(V): flat indices 0, 1, 2 of hypothesis 0
    assert parent[0].tolist() == [0, 0, 0] and token[0].tolist() == [0, 1, 2]
    np.testing.assert_allclose(out[0].numpy(), -math.log(V), atol=1e-5)
    # image 1: finished hypothesis 2 keeps -0.5 with token 2; then hypothesis 1's spike; then the tie at index 0
    lse1 = math.log(V - 1 + math.exp(3.0))
    assert parent[1].tolist() == [2, 1, 0] and token[1].tolist() == [2, 650, 0]
    np.testing.assert_allclose(out[1].numpy(), [-0.5, -1.0 + 3.0 - lse1, -1.0 - math.log(V)], atol=1e-5)
    # argument errors
    assert lib.sat_beam_step(logits.data_ptr(), V, scores.data_ptr(), None, -1, B, 9, V, parent.data_ptr(),
                             token.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), st) == 1003
    assert lib.sat_beam_step(logits.data_ptr(), V, scores.data_ptr(), None, -1, B, K, V, parent.data_ptr(),
                             token.data_ptr(), out.data_ptr(), ws.data_ptr(), 8, st) == 1002
    assert lib.sat_beam_step(None, V, scores.data_ptr(), None, -1, B, K, V, None, None, None, None, 0, st) == 1001


# ------------------------------------------------------------------------------------------------------
def _encoder_pair(arch, E, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    params, buffers = OE.init_encoder_params(E, arch, generator=gen, randomize_bn=True)
    enc = sat.EncoderCNN(E, arch=arch, compute_dtype=dtype)
    sd = dict(params)
    sd.update(buffers)
    enc.load_state_dict(sd)
    return enc.cuda(), params, buffers


@pytest.mark.parametrize("arch,hw", [(TINY, 64), (SMALL, 96)])
def test_encoder_f32_matches_oracle_train_and_eval(arch, hw):
    E, B = 32, 6
    enc, params, buffers = _encoder_pair(arch, E, 21, "f32")
    x = torch.randn(B, 3, hw, hw, generator=torch.Generator().manual_seed(22))
    bufs = {k: v.clone() for k, v in buffers.items()}
    pooled_ref, _ = OE.resnet_forward(params, bufs, x, arch, training=True)
    ref, _ = OE.head_forward(params, bufs, pooled_ref, training=True)
    enc.train()
    pooled = enc.pooled_features(x.cuda()).clone()
    np.testing.assert_allclose(pooled.cpu().numpy(), pooled_ref.numpy(), rtol=2e-3, atol=2e-4)
    # running statistics were updated exactly once, in place
    sd = enc.state_dict()
    for k in ("resnet.bn1.running_mean", "resnet.layer1.0.bn3.running_var", "resnet.layer4.0.downsample.1.running_mean"):
        np.testing.assert_allclose(sd[k].cpu().numpy(), bufs[k].numpy(), rtol=1e-3, atol=1e-5, err_msg=k)
    assert int(sd["resnet.layer2.0.bn2.num_batches_tracked"]) == 1
    # full forward (second training pass) then eval pass with the running statistics
    bufs2 = {k: v.clone() for k, v in bufs.items()}
    ref2 = OE.encoder_forward(params, bufs2, x, arch, training=True)
    out2 = enc(x.cuda())
    # BatchNorm1d over a batch of 6 divides by a small batch std: pooled-feature error (<=2e-4 above) is amplified
    np.testing.assert_allclose(out2.detach().cpu().numpy(), ref2.numpy(), rtol=0, atol=2e-2)
    ref_eval = OE.encoder_forward(params, bufs2, x, arch, training=False)
    out_eval = enc.eval()(x.cuda())
    np.testing.assert_allclose(out_eval.detach().cpu().numpy(), ref_eval.numpy(), rtol=0, atol=2e-2)
    assert ref.shape == out2.shape


def test_encoder_bf16_close_to_oracle():
    arch, E, B = SMALL, 32, 8
    enc, params, buffers = _encoder_pair(arch, E, 23, "bf16")
    x = torch.randn(B, 3, 96, 96, generator=torch.Generator().manual_seed(24))
    bufs = {k: v.clone() for k, v in buffers.items()}
    pooled_ref, _ = OE.resnet_forward(params, bufs, x, arch, training=True)
    pooled = enc.train().pooled_features(x.cuda())
    # (a) against the f32 oracle: bf16 storage (2^-8 relative rounding) through 6 bottlenecks whose BatchNorms
    #     renormalise with the statistics of 72..4608 samples: a few percent, direction preserved
    diff = (pooled.cpu() - pooled_ref)
    assert (diff.norm() / pooled_ref.norm()).item() < 0.08
    cos = torch.nn.functional.cosine_similarity(pooled.cpu().flatten(), pooled_ref.flatten(), dim=0).item()
    assert cos > 0.997
    # (b) against the oracle with bf16 STORAGE emulated at the same points (f32 arithmetic): only summation
    #     order is left, plus the occasional 1-ulp bf16 flip it causes downstream
    ref_bf = OE.resnet_forward_bf16_storage(params, x, arch)
    d2 = (pooled.cpu() - ref_bf)
    assert (d2.norm() / ref_bf.norm()).item() < 0.01, (d2.norm() / ref_bf.norm()).item()
    assert d2.abs().max().item() < 0.03 * ref_bf.abs().max().item() + 0.01


def test_encoder_bf16_eval_fused_epilogues_vs_oracle():
    """eval mode (eval.py:65): BatchNorm + add + ReLU ride in the conv epilogues -- 3-4 launches per bottleneck, no normalise
    launch at all -- against the f32 oracle in eval mode and the bf16 train-mode program's launch count"""
    arch, E, B = SMALL, 32, 8
    x = torch.randn(B, 3, 96, 96, generator=torch.Generator().manual_seed(26))
    fused, params, buffers = _encoder_pair(arch, E, 25, "bf16")
    out = fused.eval().pooled_features(x.cuda()).clone()
    prog = next(v for k, v in fused._programs.items() if k[7] is None)       # the forward's own program
    kinds = [prog.ops[i].kind for i in range(prog.n_ops)]
    L = sat._lib
    assert L.OP_BN_RELU not in kinds and L.OP_BN_ADD_RELU not in kinds and L.OP_BN_FINALIZE not in kinds
    assert kinds.count(L.OP_CONV) == 1 + 3 * sum(arch["layers"]) + len(arch["layers"])      # stem + 3 per bottleneck + 4 projections
    bufs = {k: v.clone() for k, v in buffers.items()}
    pooled_ref, _ = OE.resnet_forward(params, bufs, x, arch, training=False)
    rel = ((out.cpu() - pooled_ref).norm() / pooled_ref.norm()).item()
    assert rel < 0.05, rel
    for k in ("resnet.bn1.running_mean", "resnet.layer2.0.bn3.running_var"):      # eval never touches the statistics
        assert torch.equal(fused.state_dict()[k].cpu(), buffers[k])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_encoder_graph_replay_is_bit_identical_to_eager_launches(monkeypatch, dtype):
    """sat_graph_create / sat_graph_launch (one hipGraph per step parity) vs sat_run_ops_parity, 6 training steps"""
    arch, E, B = SMALL, 32, 8
    monkeypatch.setenv("SAT_GRAPH", "0")
    eager, _, _ = _encoder_pair(arch, E, 41, dtype)
    gen = torch.Generator().manual_seed(42)
    xs = [torch.randn(B, 3, 96, 96, generator=gen).cuda() for _ in range(6)]
    eager.train()
    ref = [eager.pooled_features(x).clone() for x in xs]
    monkeypatch.setenv("SAT_GRAPH", "1")
    graphed, _, _ = _encoder_pair(arch, E, 41, dtype)
    graphed.train()
    out = [graphed.pooled_features(x).clone() for x in xs]
    prog = next(v for k, v in graphed._programs.items() if k[7] is None)     # the forward's own program (not the look-ahead leader)
    if prog is not None:
        assert prog._graphs[0] is not None and prog._graphs[1] is not None     # really replayed, not eager
    for a, b in zip(ref, out):
        assert torch.equal(a, b)
    sa, sb = eager.state_dict(), graphed.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_full_train_step_matches_oracle():
    """whole train.py:126-146 iteration (encoder f32 + decoder + CE + backward + clamp + Adam) vs the CPU oracle"""
    arch, E, H, V, Lh, B, T = TINY, 32, 64, 300, 1, 6, 12
    gen = torch.Generator().manual_seed(31)
    enc_params, enc_buffers = OE.init_encoder_params(E, arch, generator=gen, randomize_bn=True)
    dec_params = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    model = sat.ShowAndTell(E, H, V, Lh, arch=arch, compute_dtype="f32")
    sd = dict(enc_params)
    sd.update(enc_buffers)
    model.encoder.load_state_dict(sd)
    model.decoder.load_state_dict(dec_params)
    model.cuda().train()
    images = torch.randn(B, 3, 64, 64, generator=gen)
    lengths = [12, 12, 10, 9, 7, 4]
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, V, (l - 2,), generator=gen)
        caps[b, l - 1] = 2
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    state = {}
    for it in range(2):
        ref_loss, ref_grads = OT.full_step(enc_params, enc_buffers, dec_params, images, caps, lengths, state, arch=arch,
                                           num_layers=Lh)
        loss = ts.step(images.cuda(), caps.cuda(), lengths)
        assert abs(loss.item() - ref_loss.item()) < 1e-4, it
    # resnet.fc.bias is left out: under train-mode BatchNorm1d its gradient is mathematically zero, so what Adam
    # normalises to +-lr is pure rounding noise -- in the torch reference as much as here.
    name_map = {"encoder.resnet.fc.weight": enc_params["resnet.fc.weight"], "encoder.bn.weight": enc_params["bn.weight"],
                "encoder.bn.bias": enc_params["bn.bias"]}
    for k, ref in name_map.items():
        got = dict(model.named_parameters())[k].detach().cpu()
        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=2e-5, err_msg=k)
    for k, ref in dec_params.items():
        got = dict(model.decoder.named_parameters())[k].detach().cpu()
        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=2e-5, err_msg=k)


def test_training_trajectory_eight_steps_vs_oracle():
    """eight whole iterations (fresh batch every step) against the CPU oracle: covers the eager -> hipGraph capture ->
    replay hand-over of the encoder program for both step parities, running-statistics updates and the Adam state"""
    arch, E, H, V, Lh, B, T = TINY, 32, 64, 300, 1, 6, 12
    gen = torch.Generator().manual_seed(61)
    enc_params, enc_buffers = OE.init_encoder_params(E, arch, generator=gen, randomize_bn=True)
    dec_params = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    model = sat.ShowAndTell(E, H, V, Lh, arch=arch, compute_dtype="f32")
    sd = dict(enc_params)
    sd.update(enc_buffers)
    model.encoder.load_state_dict(sd)
    model.decoder.load_state_dict(dec_params)
    model.cuda().train()
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    state = {}
    for it in range(8):
        images = torch.randn(B, 3, 64, 64, generator=gen)
        lengths = sorted(torch.randint(3, T + 1, (B,), generator=gen).tolist(), reverse=True)
        caps = torch.zeros(B, T, dtype=torch.long)
        for b, l in enumerate(lengths):
            caps[b, 0] = 1
            caps[b, 1:l - 1] = torch.randint(4, V, (l - 2,), generator=gen)
            caps[b, l - 1] = 2
        ref_loss, _ = OT.full_step(enc_params, enc_buffers, dec_params, images, caps, lengths, state, arch=arch, num_layers=Lh)
        loss = ts.step(images.cuda(), caps.cuda(), lengths)
        assert abs(loss.item() - ref_loss.item()) < 1e-4 * (it + 1), (it, loss.item(), ref_loss.item())
    prog = next(v for k, v in model.encoder._programs.items() if k[7] is None)
    assert prog._graphs[0] is not None and prog._graphs[1] is not None
    got = model.encoder.state_dict()
    for k in ("resnet.bn1.running_mean", "resnet.layer3.0.bn2.running_var", "resnet.layer4.0.downsample.1.running_var",
              "bn.running_mean"):
        # pooled features agree to ~2e-4 (f32 conv stack, different summation order); the statistics inherit that
        np.testing.assert_allclose(got[k].cpu().numpy(), enc_buffers[k].numpy(), rtol=2e-3, atol=2e-4, err_msg=k)
    assert int(got["resnet.layer1.0.bn1.num_batches_tracked"]) == 8
    for k, ref in dec_params.items():
        g = dict(model.decoder.named_parameters())[k].detach().cpu()
        np.testing.assert_allclose(g.numpy(), ref.numpy(), rtol=0, atol=2e-4, err_msg=k)


def _small_model_and_batch(seed, dtype="bf16"):
    arch, E, H, V, Lh, B, T = SMALL, 32, 64, 300, 2, 8, 12
    torch.manual_seed(seed)
    model = sat.ShowAndTell(E, H, V, Lh, arch=arch, compute_dtype=dtype).cuda().train()
    gen = torch.Generator().manual_seed(seed + 1)
    batches = []
    for _ in range(4):
        images = torch.randn(B, 3, 96, 96, generator=gen)
        lengths = sorted(torch.randint(4, T + 1, (B,), generator=gen).tolist(), reverse=True)
        caps = torch.zeros(B, T, dtype=torch.long)
        for b, l in enumerate(lengths):
            caps[b, 0] = 1
            caps[b, 1:l - 1] = torch.randint(4, V, (l - 2,), generator=gen)
            caps[b, l - 1] = 2
        batches.append((images.cuda(), caps.cuda(), lengths))
    return model, batches, (E, H, V, Lh, arch, dtype)


def test_checkpoint_resume_is_bit_exact_and_interchanges_with_torch_adam():
    """model.state_dict() (train.py:193 saves exactly that) + the Adam state in torch.optim.Adam layout: a run resumed
    from them continues bit-identically, and the state loads into a torch Adam built as train.py:55-56 builds it"""
    model, batches, (E, H, V, Lh, arch, dtype) = _small_model_and_batch(51)
    ts = sat.TrainStep(model, lr=2e-3, grad_clip=0.1)
    for b in batches[:2]:
        ts.step(*b)
    ck_model = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    ck_opt = ts.optimizer_state_dict()
    ck_opt = {"state": {i: {k: v.cpu() for k, v in s.items()} for i, s in ck_opt["state"].items()},
              "param_groups": ck_opt["param_groups"]}
    for b in batches[2:]:
        ts.step(*b)
    # resume in a fresh model + fresh TrainStep
    model2 = sat.ShowAndTell(E, H, V, Lh, arch=arch, compute_dtype=dtype)
    model2.load_state_dict(ck_model)
    model2.cuda().train()
    ts2 = sat.TrainStep(model2)
    ts2.load_optimizer_state_dict(ck_opt)
    assert ts2.step_count == 2 and ts2.lr == 2e-3
    for b in batches[2:]:
        ts2.step(*b)
    sa, sb = model.state_dict(), model2.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(ts.flat.m, ts2.flat.m) and torch.equal(ts.flat.v, ts2.flat.v)
    # torch.optim.Adam over filter(requires_grad, parameters()) accepts the same dict (train.py:55-56)
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(cpu, lr=1e-3)
    opt.load_state_dict(ck_opt)
    assert opt.param_groups[0]["lr"] == 2e-3
    st0 = opt.state[cpu[0]]
    assert int(st0["step"]) == 2 and st0["exp_avg"].shape == cpu[0].shape
    # and its own state_dict loads back
    ts2.load_optimizer_state_dict(opt.state_dict())
    assert ts2.step_count == 2


def test_trainstep_lstm_workspaces_follow_the_batch_not_the_caption_width():
    """Caption widths 12 -> 20 -> 12 at one batch size: every step's loss and gradients equal, bit for bit, those of a fresh
    TrainStep (same parameters and Adam state) fed that batch alone, and the second width-12 batch runs on the LSTM workspaces
    the width-20 one grew instead of allocating new ones.  B * (width - 1) > 4H: the backward workspace size depends on the width"""
    E, H, V, Lh, B = 32, 64, 300, 2, 32
    torch.manual_seed(5)
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY).cuda().train()
    ts = sat.TrainStep(model, lr=1e-3, grad_clip=0.1)
    gen = torch.Generator().manual_seed(6)
    held = []                   # the owner's buffers after each step, kept alive: a freed buffer's address could come back
    for width in (12, 20, 12):
        feats = torch.randn(B, E, generator=gen).cuda()                    # cached features: decoder-only steps
        lengths = [width] + sorted(torch.randint(3, width + 1, (B - 1,), generator=gen).tolist(), reverse=True)
        caps = torch.randint(4, V, (B, width), generator=gen).cuda()
        inv = 1.0 / sum(l - 1 for l in lengths)
        fresh = sat.ShowAndTell(E, H, V, Lh, arch=TINY)
        fresh.load_state_dict(model.state_dict())
        ts2 = sat.TrainStep(fresh.cuda().train())
        ts2.load_optimizer_state_dict(ts.optimizer_state_dict())
        loss = ts.forward_backward((feats, caps, lengths), inv).clone()
        ref = ts2.forward_backward((feats, caps, lengths), inv).clone()
        assert torch.equal(loss, ref) and torch.equal(ts.flat_grad, ts2.flat_grad), width
        held.append(ts.lstm_ws.fwd + ts.lstm_ws.bwd)
        if len(held) == 3:      # the last step ran on buffers larger than the fresh engine's
            assert all(a.numel() > b.numel() for a, b in zip(ts.lstm_ws.bwd, ts2.lstm_ws.bwd))
        ts.optimizer_step()
        ts2.check_ids()
    ts.check_ids()
    assert all(b.numel() > a.numel() for a, b in zip(held[0][Lh:], held[1][Lh:]))      # width 20 grew the backward buffers
    assert all(a is b for a, b in zip(held[2], held[1]))                                # width 12 again: nothing reallocated


# ------------------------------------------------------------------------------------------------------
# BASELINE cfg-2 size (B=64, 224x224, E=256, H=512, V=10000): size-independent properties
def _cfg2(seed=123, B=64):
    torch.manual_seed(seed)
    model = sat.ShowAndTell(256, 512, 10000, 1, compute_dtype="bf16").cuda().train()
    images = torch.randn(B, 3, 224, 224, device="cuda")
    caps = torch.randint(4, 10000, (B, 20), device="cuda")
    caps[:, 0], caps[:, 19] = 1, 2
    return model, images, caps, [20] * B


def test_cfg2_full_size_properties():
    model, images, caps, lengths = _cfg2()
    ts = sat.TrainStep(model)
    w0 = model.decoder.linear.weight.detach().clone()
    l0 = ts.forward_backward((images, caps, lengths), 1.0 / (64 * 19)).clone()   # the slot itself is reused
    g_a = ts.flat.grads.clone()
    l1 = ts.forward_backward((images, caps, lengths), 1.0 / (64 * 19)).clone()
    # (1) determinism: identical inputs -> bit-identical loss and gradients (fixed-order reductions, no atomics)
    assert l0.item() == l1.item()
    assert torch.equal(g_a[:ts.flat.n], ts.flat.grads[:ts.flat.n])
    # (2) at random init the mean CE is ln(V) to within the logit scale
    assert abs(l0.item() - math.log(10000)) < 0.1
    # (3) softmax-minus-onehot rows sum to zero => the vocab bias gradient sums to ~0.  In the bf16 throughput mode
    # d(loss)/d(logits) is stored as bf16: the 1216 target entries -(1-p)/N are nearly EQUAL at initialisation, so their bf16
    # rounding (2^-9 relative of 8e-4 each) is systematic, not random: the row sums miss zero by up to 2e-3 in total.  The
    # exact-f32 decoder keeps the 1e-4.
    assert ts.decoder_gemm_dtype == "bf16"
    assert abs(ts.flat.grad("decoder.linear.bias").sum().item()) < 5e-3
    ts.decoder_gemm_dtype = "f32"
    l32 = ts.forward_backward((images, caps, lengths), 1.0 / (64 * 19)).clone()
    assert abs(ts.flat.grad("decoder.linear.bias").sum().item()) < 1e-4
    assert abs(l32.item() - l0.item()) < 1e-4            # bf16 vs exact-f32 vocab projection: the CE moves by < 1e-4
    ts.decoder_gemm_dtype = "bf16"
    ts.forward_backward((images, caps, lengths), 1.0 / (64 * 19))
    # (4) linearity of the backward in the loss scale
    ts.forward_backward((images, caps, lengths), 2.0 / (64 * 19))
    torch.testing.assert_close(ts.flat.grad("decoder.lstm.weight_hh_l0"), 2 * g_a[slice(*_slice(ts, "decoder.lstm.weight_hh_l0"))].view(2048, 512),
                               rtol=1e-4, atol=1e-9)
    # (5) the elementwise clamp bounds every Adam update by lr (|m/sqrt(v)| <= 1 on the first step)
    ts.forward_backward((images, caps, lengths), 1.0 / (64 * 19))
    ts.optimizer_step()
    assert (model.decoder.linear.weight.detach() - w0).abs().max().item() <= 1e-3 * 1.001
    # (6) loss goes down on a fixed batch
    losses = [ts.step(images, caps, lengths).item() for _ in range(5)]
    assert losses[-1] < l0.item() - 0.05, losses


def _slice(ts, name):
    o, n, _ = ts.flat.slices[name]
    return o, o + n


def test_cfg2_greedy_and_dropin_forward():
    model, images, caps, lengths = _cfg2(B=8)
    out = model(images, caps[:, :-1], [19] * 8)
    assert out.shape == (8 * 19, 10000) and torch.isfinite(out).all()
    ids = model.eval().sample(images, None)
    assert ids.shape == (8, 20) and ids.dtype == torch.int64
    assert int(ids.min()) >= 0 and int(ids.max()) < 10000


def test_cfg2_decode_full_size_vs_oracle_and_eval_determinism():
    """BASELINE configs[4] shape on one GPU: batch 64, V=10000, beam 5 and greedy, decoded from the REAL eval-mode encoder
    output: a well-conditioned stack (`conditioning="trained_like"`) whose running statistics were brought to the data by
    train-mode passes, as a trained model's are (eval.py:65 `model.eval()`), and a vocabulary projection with trained-like logit
    spread.  The decoder half is compared with the CPU oracle on the SAME encoder features: greedy ids bit-exact, beam-5 best
    hypothesis equal on >= 95 % of the images (a candidate pair closer than the f32 summation-order noise may swap); the eval-mode
    encoder (running-statistics BatchNorm in the conv epilogues, hipGraph replay from the 3rd call on) must be bit-reproducible
    call after call."""
    gen = torch.Generator().manual_seed(321)
    ep, eb = OE.init_encoder_params(256, OE.RESNET152, generator=gen, conditioning="trained_like")
    dp = OD.init_decoder_params(256, 512, 10000, 1, generator=gen)
    dp["linear.weight"] = dp["linear.weight"] * 6.0          # a trained projection separates its logits: no 1e-6 ties among 10000 words
    model = sat.ShowAndTell(256, 512, 10000, 1, compute_dtype="bf16")
    model.encoder.load_state_dict({**ep, **eb})
    model.decoder.load_state_dict(dp)
    model.cuda().train()
    images = torch.randn(64, 3, 224, 224, generator=gen).cuda()
    with torch.no_grad():
        for _ in range(40):                                   # momentum 0.1: the running statistics converge to this data's
            model.encoder(images)
    model.eval()
    with torch.no_grad():
        feats = [model.encoder(images).clone() for _ in range(4)]      # eager, eager, graph capture, graph replay
    for f in feats[1:]:
        assert torch.equal(feats[0].view(torch.int32), f.view(torch.int32))       # bit patterns (NaN-proof)
    f0 = feats[0]
    assert bool(torch.isfinite(f0).all()) and 0.05 < float(f0.std()) < 20.0, (float(f0.abs().max()), float(f0.std()))
    assert float((f0[0] - f0[1]).norm() / f0[0].norm()) > 0.05            # the features really depend on the image
    params = {k: v.detach().cpu() for k, v in model.decoder.state_dict().items()}
    f_cpu = f0.cpu()
    greedy = model.decoder.sample(f0)
    assert torch.equal(greedy.cpu(), OD.greedy_sample(params, f_cpu, 1))
    ids, scores = model.decoder.sample_beam(f0, 5, end_id=2, return_all=True)
    ref_ids, ref_scores = OD.beam_search(params, f_cpu, 5, 1, end_id=2)
    np.testing.assert_allclose(scores.cpu().numpy(), ref_scores.numpy(), rtol=0, atol=5e-2)
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    same = (ids[:, 0].cpu() == ref_ids[:, 0]).all(dim=1).float().mean().item()
    assert same >= 0.95, same
    # ids and scores are consistent: teacher-forcing the returned best sequence reproduces its score
    for b in (0, 17, 63):
        seq = ids[b, 0].cpu()
        logits = OD.decoder_forward(params, f_cpu[b:b + 1], seq[:19].unsqueeze(0), [20], 1)
        lp = torch.log_softmax(logits, 1)
        total, done = 0.0, False
        for t in range(20):
            if not done:
                total += lp[t, seq[t]].item()
            done = done or int(seq[t]) == 2
        assert abs(total - scores[b, 0].item()) < 2e-3, (b, total, scores[b, 0].item())
    assert torch.equal(model.sample_beam(images, 5, end_id=2), ids[:, 0])
    # beam-1 vs greedy at full size: bit-equal on the goldens; here the two paths' logits differ in summation order
    # (skinny arg-max kernel vs GEMM + sat_beam_step), so a near-tie may flip in one or two of the 64 images
    b1 = model.decoder.sample_beam(f0, 1)
    assert (b1 == greedy).all(dim=1).float().mean().item() >= 0.95


@pytest.mark.timeout(900)
def test_resnet152_f32_matches_oracle_cfg1():
    """BASELINE cfg-1 shape: batch 4, 224x224, the real [3,8,36,3] stack, f32 MFMA vs the CPU oracle"""
    arch, E, B = OE.RESNET152, 256, 4
    enc, params, buffers = _encoder_pair(arch, E, 41, "f32")
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(42))
    bufs = {k: v.clone() for k, v in buffers.items()}
    pooled_ref, _ = OE.resnet_forward(params, bufs, x, arch, training=True)
    pooled = enc.train().pooled_features(x.cuda())
    err = (pooled.cpu() - pooled_ref).abs().max().item()
    assert err < 2e-3 * max(1.0, pooled_ref.abs().max().item()), err


@pytest.mark.parametrize("B,T,E,H,V,Lh", [(70, 9, 36, 40, 1003, 1), (5, 14, 32, 64, 300, 2), (1, 6, 32, 32, 64, 1),
                                          (130, 5, 64, 128, 500, 1),
                                          (16, 20, 512, 1024, 10000, 2)])     # BASELINE configs[3] decoder (cfg4)
def test_decoder_odd_shapes_ragged_vs_oracle(B, T, E, H, V, Lh):
    """edge cases the reference's collate_fn can produce: batch 1, batches larger than one 64-row chunk of the skinny
    kernels, steeply ragged lengths (down to the minimum 2), vocab / hidden sizes that are not tile multiples"""
    gen = torch.Generator().manual_seed(B * 131 + T)
    params = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    lengths = sorted([int(x) for x in torch.randint(2, T + 1, (B,), generator=gen)], reverse=True)
    lengths[0] = T
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(lengths):
        caps[b, 0] = 1
        if l > 2:
            caps[b, 1:l - 1] = torch.randint(4, V, (l - 2,), generator=gen)
        caps[b, l - 1] = 2
    feats = torch.randn(B, E, generator=gen)
    ref_loss, ref_grads, ref_dfeat, ref_logits = OT.decoder_loss_and_grads(params, feats, caps, lengths, Lh)
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    dec.cuda()
    fd = feats.cuda().requires_grad_(True)
    cd = caps.cuda()
    targets, l1 = sat.pack_targets(cd, lengths)
    out = dec(fd, cd[:, :-1], l1)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_logits.numpy(), rtol=0, atol=2e-5)
    loss = torch.nn.functional.cross_entropy(out, targets)
    assert abs(loss.item() - ref_loss.item()) < 1e-4
    loss.backward()
    np.testing.assert_allclose(fd.grad.cpu().numpy(), ref_dfeat.numpy(), rtol=2e-3, atol=2e-7)
    for k, p in dec.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref_grads[k].numpy(), rtol=2e-3, atol=2e-7, err_msg=k)
    ids = dec.eval().sample(feats.cuda(), None)
    assert tuple(ids.shape) == ((B, 20) if B > 1 else (20,))                 # models.py:67 `sampled_ids.squeeze()`
    assert np.array_equal(ids.cpu().numpy().reshape(B, 20), OD.greedy_sample(params, feats, Lh).numpy())


def test_decoder_rejects_bad_inputs():
    dec = sat.DecoderRNN(32, 64, 100, 1).cuda()
    f = torch.zeros(3, 32, device="cuda")
    c = torch.zeros(3, 5, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError):
        dec(f, c, [3, 5, 2])            # not sorted (pack_padded_sequence would raise too)
    with pytest.raises(ValueError):
        dec(f, c, [6, 6])               # wrong batch size
    with pytest.raises(ValueError):
        dec(f, c, [9, 3, 2])            # longer than captions + 1


def test_device_prefetcher_feeds_the_step_like_direct_copies():
    """H2D prefetch on a side stream (pinned host batches) must deliver exactly the tensors a blocking .cuda() would,
    in order, and a TrainStep fed through it must reproduce the directly-fed run bit for bit"""
    model, batches, (E, H, V, Lh, arch, dtype) = _small_model_and_batch(71)
    host = [(im.cpu().pin_memory(), cp.cpu().pin_memory(), ln) for im, cp, ln in batches]
    seen = list(sat.DevicePrefetcher(host, "cuda"))
    assert len(seen) == len(host)
    for (im, cp, ln), (him, hcp, hln) in zip(seen, host):
        assert im.is_cuda and torch.equal(im.cpu(), him) and torch.equal(cp.cpu(), hcp) and ln == hln
    assert list(sat.DevicePrefetcher([], "cuda")) == []
    ts = sat.TrainStep(model, lr=1e-3)
    ref = [ts.step(*b).item() for b in batches]
    model2, _, _ = _small_model_and_batch(71)
    ts2 = sat.TrainStep(model2, lr=1e-3)
    got = [ts2.step(im, cp, ln).item() for im, cp, ln in sat.DevicePrefetcher(host, "cuda")]
    assert got == ref
    # depth 3 + the encoder look-ahead fed from the prefetcher's upcoming batches: still the same losses, bit for bit
    model3, _, _ = _small_model_and_batch(71)
    ts3 = sat.TrainStep(model3, lr=1e-3)
    pf = sat.DevicePrefetcher(host, "cuda", depth=3)
    got3 = []
    for im, cp, ln in pf:
        ahead = pf.upcoming_images()
        assert len(ahead) <= 3 and all(t.is_cuda for t in ahead)
        got3.append(ts3.step(im, cp, ln, next_images=ahead or None).item())
    assert got3 == ref and not model3.encoder._inflight


def test_validation_forward_unshifted_captions_and_end_truncation_golden(golden_dir):
    """The validation half of `evaluation` (eval.py:91-109) against G8 (the imported reference decoder): the drop-in
    forward with UNSHIFTED captions and FULL lengths, its mean CE against `pack(captions, lengths)`, the greedy ids, and the
    device-side '<end>' truncation counts (`sat_kept_tokens`)."""
    g = load(golden_dir, "G8_dec_eval_unshifted.npz")
    dec, params, (E, H, V, Lh, B, T) = golden_setup(g)
    dec.eval()
    feats, caps = torch.from_numpy(g["features"]).cuda(), torch.from_numpy(g["captions"]).cuda()
    lengths = [int(x) for x in g["lengths"]]
    with torch.no_grad():
        logits = dec(feats, caps, lengths)                                    # eval.py:93
        targets, pi = sat.pack_validation_targets(caps, lengths)             # eval.py:91
        loss = sat.mean_cross_entropy(logits.contiguous(), targets)          # eval.py:95
        ids = dec.sample(feats, None)                                         # eval.py:99
    assert logits.shape == (sum(lengths), V)
    assert np.array_equal(targets.cpu().numpy(), g["targets"])
    np.testing.assert_allclose(logits.cpu().numpy(), g["logits"], rtol=0, atol=1e-5)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    assert np.array_equal(ids.cpu().numpy(), g["greedy_ids"])
    planted = torch.from_numpy(g["ids_planted"]).cuda()
    kept = sat.kept_tokens(planted, int(g["end_id"]))
    assert kept.dtype == torch.int32 and kept.cpu().tolist() == [int(x) for x in g["kept_tokens"]]
    # a strided view (one hypothesis plane of beam ids [B,K,T]) and the host-side join of eval.py:101-110
    beams = torch.stack([planted, planted.flip(1)], 1)
    assert sat.kept_tokens(beams[:, 0], int(g["end_id"])).cpu().tolist() == [int(x) for x in g["kept_tokens"]]
    words = {i: "w%d" % i for i in range(V)}
    sents = sat.sentences(planted.cpu(), kept.cpu(), words)
    assert sents[1] == "" and len(sents[0].split()) == 5 and len(sents[3].split()) == 20


def test_validation_step_whole_model_eval_mode_vs_oracle():
    """`validation_step` on the whole Show-and-Tell model in eval mode (eval.py:65: running statistics in every BatchNorm):
    loss and greedy ids against the oracle (encoder f32 eval + `validation_loss` + `greedy_sample`)"""
    E, H, V, Lh, B, T = 32, 64, 120, 1, 5, 9
    gen = torch.Generator().manual_seed(77)
    ep, eb = OE.init_encoder_params(E, TINY, generator=gen, randomize_bn=True)
    for k in eb:                                         # non-trivial running statistics
        if k.endswith("running_mean"):
            eb[k] = torch.randn(eb[k].shape, generator=gen) * 0.1
        elif k.endswith("running_var"):
            eb[k] = torch.rand(eb[k].shape, generator=gen) + 0.5
    dp = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    model = sat.ShowAndTell(E, H, V, Lh, arch=TINY, compute_dtype="f32")
    model.encoder.load_state_dict({**ep, **eb})
    model.decoder.load_state_dict(dp)
    model.cuda().eval()
    images = torch.randn(B, 3, 64, 64, generator=gen)
    lengths = [9, 9, 7, 4, 2]
    caps = torch.zeros(B, T, dtype=torch.long)
    for b, l in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, V, (max(l - 2, 0),), generator=gen)
        caps[b, l - 1] = 2
    out = sat.validation_step(model, images.cuda(), caps.cuda(), lengths, end_id=2)
    bufs = {k: v.clone() for k, v in eb.items()}
    feats = OE.encoder_forward(ep, bufs, images, TINY, training=False)
    ref_loss, _ = OT.validation_loss(dp, feats, caps, lengths, Lh)
    ref_ids = OD.greedy_sample(dp, feats, Lh)
    assert abs(out["loss"].item() - ref_loss.item()) < 1e-4
    assert torch.equal(out["ids"].cpu(), ref_ids)
    assert out["kept"].cpu().tolist() == OT.kept_tokens(ref_ids, 2)
    with pytest.raises(RuntimeError):
        sat.validation_step(model.train(), images.cuda(), caps.cuda(), lengths)
