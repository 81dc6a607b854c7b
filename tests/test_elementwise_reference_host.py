"""CPU: tests/elementwise_reference.py is validated before the GPU sweep (tests/test_gpu_elementwise_edges.py) trusts it -- against
torch's own batch_norm (train and eval, running statistics included), max_pool2d, mean, cross_entropy with autograd, optim.Adam,
nn.Embedding + pack_padded_sequence with autograd, and `oracle.encoder.head_forward / head_backward` -- and the float32
restatement's error against float64 is measured at every case of the sweep: the GPU test allows `TOL_FACTOR` x that value where
the tolerances of the existing one-shape tests do not hold.  Run with -s to print the table elementwise_reference.F32_ERR keeps."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_reference as R
from oracle import encoder as OE

D = torch.float64


def near(a, b, rtol=1e-12, atol=1e-13):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=rtol, atol=atol)


@pytest.mark.parametrize("tiles,C", [(1, 4), (33, 40), (300, 64)])
def test_finalize_and_derived_table_equal_torch_batch_norm(tiles, C):
    """the slabs and the integer sums of real activations give torch's train-mode normalisation and running statistics (as far as
    the f32 slabs and the 2^-22 fixed point carry: the activations below are small dyadic numbers, so both are exact), and the
    eval table gives torch's eval mode"""
    g = R.gen(100, tiles, C)
    rows = 8
    x = (torch.randint(-2 ** 9, 2 ** 9, (tiles, rows, C), generator=g).double() * 2.0 ** -7)       # |x| < 4, multiples of 2^-7
    part = torch.stack([x.sum(1), (x * x).sum(1)], 1).float()
    assert torch.equal(part.double(), torch.stack([x.sum(1), (x * x).sum(1)], 1)), "the slabs are exact"
    count = tiles * rows
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    flat = x.reshape(count, C)
    trm, trv = rm.double(), rv.double()
    want = F.batch_norm(flat, trm, trv, gamma.double(), beta.double(), True, R.f32v(R.BN_MOMENTUM), R.f32v(R.BN_EPS))
    acc = torch.stack([torch.round(flat.sum(0) * R.STAT_SCALE), torch.round((flat * flat).sum(0) * R.STAT_SCALE)]).long()
    assert torch.equal(acc, R.slabs_to_acc(part)) and torch.equal(acc, R.slabs_to_acc(part.flip(0))), "exact in any order"
    for t in (R.bn_finalize(part, count, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, 1),
              R.bn_table_from_acc(acc, count, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS)):
        near(flat * t["scale"] + t["shift"], want, rtol=1e-9, atol=1e-10)        # E[x^2] - mean^2 against torch's two-pass variance
        # the batch statistics enter the running update as f32 values: 2^-24 relative of the statistic, times the momentum
        near(t["running_mean"], trm, rtol=0, atol=0.1 * 2.0 ** -24 * 4)
        near(t["running_var"], trv, rtol=0, atol=0.1 * 2.0 ** -24 * 16)
    ev = R.bn_finalize(None, count, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, 0)
    near(flat * ev["scale"] + ev["shift"], F.batch_norm(flat, rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.1, R.f32v(R.BN_EPS)))
    # count = 1: the biased variance goes into the running statistics
    one = R.bn_finalize(part[:1] * 0 + torch.stack([x[0, 0], x[0, 0] ** 2]).float(), 1, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, 1)
    near(one["running_var"], (1 - R.f32v(0.1)) * rv.double(), rtol=1e-12)
    near(one["scale"], gamma.double() / np.sqrt(R.f32v(R.BN_EPS)))


def test_constant_channel_of_the_finalize_inputs_has_exactly_zero_variance():
    for tiles in R.FIN_TILES:
        d, r = R.finalize_inputs(tiles, 4), R.finalize_case(tiles, 4)
        assert r["scale"][1].item() == d["gamma"][1].double().item() / np.sqrt(R.f32v(R.BN_EPS))


def test_running_apply_is_one_rounding_of_the_float64_expression():
    g = R.gen(101)
    rm, rv, bm, bv = (torch.randn(600, generator=g) for _ in range(4))
    m = np.float64(np.float32(0.1))
    wm, wv = R.running_apply(rm, rv, bm, bv, 0.1)
    assert np.array_equal(wm.numpy(), ((1.0 - m) * rm.numpy().astype(np.float64) + m * bm.numpy().astype(np.float64)).astype(np.float32))
    assert np.array_equal(wv.numpy(), ((1.0 - m) * rv.numpy().astype(np.float64) + m * bv.numpy().astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("shape", R.POOL_SHAPES + [(3, 10, 10, 32)])
def test_normalise_and_pools_equal_torch(shape):
    d = R.bn_inputs("f32", shape)
    x, z, s, t, s1, t1 = (d[k].double() for k in ("x", "z", "scale", "shift", "scale1", "shift1"))
    nchw = lambda a: a.permute(0, 3, 1, 2)
    y = x * s + t
    assert torch.equal(R.bn_act(x, s, t), F.relu(y))
    assert torch.equal(R.bn_act(x, s, t, z), F.relu(y + z))
    assert torch.equal(R.bn_act(x, s, t, z, s1, t1), F.relu(y + (z * s1 + t1)))
    want = F.max_pool2d(F.relu(nchw(y)), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(R.bn_relu_maxpool(x, s, t), want)
    N, H, W, C = shape
    near(R.avgpool(x.reshape(N, H * W, C)), x.mean((1, 2)))
    # the derived table is torch's train-mode batch_norm of any batch that has these sums: checked through the statistics
    tab = R.bn_table_from_acc(d["acc"], d["count"], d["gamma"], d["beta"], d["rm"], d["rv"], R.BN_MOMENTUM, R.BN_EPS)
    mean = d["acc"][0].double() / R.STAT_SCALE / d["count"]
    var = d["acc"][1].double() / R.STAT_SCALE / d["count"] - mean ** 2
    near(tab["scale"], d["gamma"].double() / torch.sqrt(var + R.f32v(R.BN_EPS)))
    near(tab["shift"], d["beta"].double() - mean * tab["scale"])


@pytest.mark.parametrize("V", [1, 5, 1003])
def test_cross_entropy_equals_torch_and_autograd(V):
    logits, targets, kinds = R.ce_inputs(V)
    assert set(kinds) == set(R.CE_KINDS) and {0, V - 1, 4 * (V // 4) if V % 4 else V - 1, -1, V} <= set(targets.tolist()) | {V - 1}
    r = R.ce_rows(logits.double(), targets, R.CE_INV)
    lg = logits.double().requires_grad_(True)
    t = targets.clamp(0, V - 1)                               # -1 and V: the kernel clamps for memory safety
    rows = F.cross_entropy(lg, t, reduction="none")
    (rows.sum() * R.f32v(R.CE_INV)).backward()
    near(r["row_loss"], rows, atol=1e-12)
    near(r["grad"], lg.grad, atol=1e-15)
    near(r["loss"], rows.sum() * R.f32v(R.CE_INV))
    assert torch.isfinite(r["grad"]).all() and torch.isfinite(r["row_loss"]).all()


def test_weighted_cross_entropy_equals_autograd_on_the_live_rows():
    d = R.ce_weighted_inputs()
    r = R.ce_rows(d["logits"].double(), d["targets"], d["w"])
    live = d["w"] != 0
    assert int((~live).sum()) == 2 and torch.isnan(d["logits"][~live]).all()
    assert {1000, 1001, 1002} <= set(d["targets"].tolist())
    assert (r["grad"][~live] == 0).all() and torch.isfinite(r["loss"])
    lg = d["logits"][live].double().requires_grad_(True)
    loss = (F.cross_entropy(lg, d["targets"][live], reduction="none") * d["w"][live].double()).sum()
    loss.backward()
    near(r["grad"][live], lg.grad, atol=1e-15)
    near(r["loss"], loss)
    # packed row n = t * B + b reads ids[b][t]
    assert all(int(d["targets"][t * d["B"] + b]) == int(d["ids"][b, t]) for t in range(d["T"]) for b in range(d["B"]))


@pytest.mark.parametrize("clip", R.ADAM_CLIP)
def test_clamp_adam_equals_torch_optim_adam(clip):
    n = 1023
    d = R.adam_inputs(n)
    ref = R.adam_case(n, clip)
    p = d["p"].double().clone().requires_grad_(True)
    hp = {k: R.f32v(v) for k, v in R.ADAM_HP.items()}          # the values the C ABI carries
    opt = torch.optim.Adam([p], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=d["m"].double().clone(), exp_avg_sq=d["v"].double().clone())
    moved = torch.zeros(n, dtype=D)
    for step, gr in enumerate(d["grads"]):
        before = p.detach().clone()
        p.grad = gr.double().clamp(-R.f32v(clip), R.f32v(clip)) if clip > 0 else gr.double().clone()
        opt.step()
        assert torch.equal(ref[step]["g"], p.grad)
        near(ref[step]["m"], opt.state[p]["exp_avg"], rtol=1e-11, atol=1e-17)          # torch's lerp form rounds otherwise
        near(ref[step]["v"], opt.state[p]["exp_avg_sq"], rtol=1e-11, atol=1e-17)
        # the launcher rounds lr / bc1 and sqrt(bc2) to float32 (2^-24 relative each, of the update), torch keeps them in float64
        moved = moved + (p.detach() - before).abs()                    # the difference of a step stays in p: summed over the steps
        assert ((ref[step]["p"] - p.detach()).abs() <= 2.0 ** -22 * moved + 1e-15).all()


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", R.BN1D_SHAPES)
def test_bn1d_head_equals_the_oracle(shape, training):
    d = {k: v.double() for k, v in R.bn1d_inputs(*shape).items()}
    r = R.bn1d_fwd(d["pooled"], d["w"], d["b"], d["gamma"], d["beta"], d["rm"], d["rv"], R.BN1D_MOMENTUM, R.BN_EPS, int(training))
    params = {"resnet.fc.weight": d["w"], "resnet.fc.bias": d["b"], "bn.weight": d["gamma"], "bn.bias": d["beta"]}
    bufs = {"bn.running_mean": d["rm"].clone(), "bn.running_var": d["rv"].clone(), "bn.num_batches_tracked": torch.zeros((), dtype=torch.int64)}
    y, tape = OE.head_forward(params, bufs, d["pooled"], training)
    # eps and the momentum are float32 values here, python floats there: 2.5e-8 relative of eps under the square root
    near(r["feats"], y, rtol=1e-6, atol=1e-6)
    near(r["running_mean"], bufs["bn.running_mean"], rtol=1e-6, atol=1e-8)
    near(r["running_var"], bufs["bn.running_var"], rtol=1e-6, atol=1e-8)
    gr = OE.head_backward(params, tape, d["dy"])
    b = R.bn1d_bwd(d["dy"], d["pooled"], tape["xhat"], tape["rstd"], d["gamma"])
    for k, name in (("dgamma", "bn.weight"), ("dbeta", "bn.bias"), ("dw", "resnet.fc.weight"), ("db", "resnet.fc.bias")):
        near(b[k], gr[name], rtol=1e-11, atol=1e-12)
    if training and shape[0] > 1:         # and the forward is torch's batch_norm
        rm, rv = d["rm"].clone(), d["rv"].clone()
        z = d["pooled"] @ d["w"].t() + d["b"]
        near(r["feats"], F.batch_norm(z, rm, rv, d["gamma"], d["beta"], True, R.f32v(R.BN1D_MOMENTUM), R.f32v(R.BN_EPS)), rtol=1e-9, atol=1e-9)
        near(r["running_var"], rv, rtol=1e-12)


@pytest.mark.parametrize("name", list(R.EMBED_CASES))
def test_embedding_gather_and_scatter_equal_nn_embedding_with_packed_sequences(name):
    d = R.embed_inputs(name)
    B, T, E, V, bs = d["B"], d["T"], d["E"], d["V"], d["bs"]
    assert d["N"] == sum(d["lengths"]) and bs[0] == B
    cap = d["captions"].clamp(0, V - 1)                       # what the kernels do with an id outside [0, V)
    emb = torch.nn.Embedding(V, E).double()
    with torch.no_grad():
        emb.weight.copy_(d["embed"])
    feats = d["features"].double().requires_grad_(True)
    seq = torch.cat([feats[:, None], emb(cap[:, :T - 1])], 1)
    packed = torch.nn.utils.rnn.pack_padded_sequence(seq, d["lengths"], batch_first=True)
    assert packed.batch_sizes.tolist() == bs
    X = R.embed_concat_fwd(d["features"], d["embed"], d["captions"], bs)
    assert torch.equal(X.double(), packed.data.detach())
    (packed.data * d["dX"].double()).sum().backward()
    df, de = R.embed_concat_bwd(d["dX"], d["captions"], bs, V)
    near(de, emb.weight.grad)
    near(df, feats.grad)
    df32, de32 = R.embed_concat_bwd(d["dX"], d["captions"], bs, V, row_ordered_f32=True)
    near(de32.double(), de, rtol=0, atol=2.0 ** -22 * max(d["N"], 1))
    assert torch.equal(df32, d["dX"][:B])
    tg = torch.nn.utils.rnn.pack_padded_sequence(d["captions"][:, 1:], d["lengths"], batch_first=True).data
    assert torch.equal(R.pack_targets(d["captions"], bs), tg)
    if name == "same_e256":
        assert int((de.abs().sum(1) > 0).sum()) == 1
    if name == "repeat_e257":
        assert len(set(cap[:, :T - 1].flatten().tolist())) <= 4 < d["N"]


# ---------------------------------------------------------------------------------------------- the tolerance table

def test_f32_restatement_error_at_every_case_of_the_sweep():
    """The figures of elementwise_reference.F32_ERR: max abs error of the float32 restatement against float64 at each case and seed,
    re-measured and compared with the frozen table.  The same figure on the host that measured it; elsewhere torch's float32
    summation order (vector width, threads) moves it by a small factor -- 16 x is allowed, as for the attention sweep."""
    got = R.measure_all()
    assert set(got) == set(R.F32_ERR), set(got) ^ set(R.F32_ERR)
    for key, errs in got.items():
        names, frozen = R.ERR_NAMES[key[0]], R.F32_ERR[key]
        print("%-44s " % (key,) + "  ".join("%s %.3g" % (k, v) for k, v in zip(names, errs)))
        assert len(errs) == len(frozen) == len(names)
        for k, v, f in zip(names, errs, frozen):
            assert np.isfinite(v), (key, k, v)
            assert (v == 0) == (f == 0) and f / 16 <= v <= f * 16, (key, k, v, f)
