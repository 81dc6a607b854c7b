"""GPU: every bf16 conv kernel variant (kVariants[], csrc/sat_conv_glds.hip) in every mode it admits -- the rows of
tests/conv_cases.py -- against the f64 definition on the kernel's bf16 operands, and against its bit family.

Every launch goes through `conv_cases.run_named`: the library is asked first which variant the op will run, and a row whose
variant would be replaced fails, so each comparison is with the kernel the row names and the two sides of a bit comparison are
different kernels.  Tolerances are the suite's own for the same quantities (test_gpu_kernels.py):
  * output, plain:                    2e-2 absolute (bf16 rounding of |y| <~ 4; test_conv_bf16_every_kernel_variant)
  * output, inference epilogue:       3e-2 + 8e-3 max|ref| (test_conv_inference_epilogue_affine_residual_relu)
  * output, fused input BatchNorm:    3e-2 + 4e-3 max|ref| (test_conv1x1_with_input_bn_relu_fused)
  * column sums / sums of squares:    1e-3 sqrt(M) + 1e-4 / rtol 2e-4 + 1e-3 (test_conv_fwd_and_stats); the integer-atomic sums are the
    same numbers rounded to 2^-22 once per tile (at most 588 tiles here: < 1e-4), so they get the same bound; behind a fused
    input BatchNorm 2e-3 sqrt(M) + 1e-3 / rtol 5e-4 + 5e-3 (test_conv3x3_lds_resident_patch_with_fused_input_bn_relu)
Bit families are the library's promise (`sat_conv_variant_family`, `sat_conv_variant_signature`): on one op, variants of one
family give the same output bits and variants of one signature the same statistics bits."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc

pytestmark = pytest.mark.gpu
L = cc.L
SCALE = 4194304.0            # 2^22: the fixed point of the integer statistics


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    return L.load()


@functools.lru_cache(maxsize=None)
def _data(geo, mode):
    """operands (bf16, host) and the f64 results of one (geometry, mode): the same for every variant that runs it"""
    g = cc.GEOS[geo]
    gen = torch.Generator().manual_seed(sum(map(ord, geo + mode)))
    fused = mode in cc.BN + cc.ADMITS["ay"]
    N, H, W, Cin, Cout, M = g["N"], g["H"], g["W"], g["Cin"], g["Cout"], g["M"]
    d = {}
    if g["layout"] == "stem":
        x = torch.randn(N, H, W, 4, generator=gen).bfloat16()
        w = (torch.randn(Cout, 7, 32, generator=gen) / 15.0).bfloat16()
    else:
        x = torch.randn(N, H, W, Cin, generator=gen)
        x = (x * 1.5 + 0.2 if fused else x).bfloat16()
        w = (torch.randn(Cout, g["KH"], g["KW"], Cin, generator=gen) / g["K"] ** 0.5).bfloat16()
    d["x"], d["w"] = x, w.reshape(Cout, -1).contiguous()
    a = x.float()
    if fused:                                           # operand = relu(bn(x) [+ residual]) rounded to bf16, as the kernel stages it
        gamma, beta = torch.rand(Cin, generator=gen) + 0.5, torch.randn(Cin, generator=gen) * 0.2 + 0.3
        xf = x.float().reshape(-1, Cin).double()
        mean, var = xf.mean(0), xf.var(0, unbiased=False)
        scale = (gamma.double() / torch.sqrt(var + 1e-5)).float()
        shift = (beta.double() - mean * scale.double()).float()
        d.update(gamma=gamma, beta=beta, mean=mean, var=var, scale=scale, shift=shift, rows=xf.shape[0],
                 sums=torch.stack([torch.round(xf.sum(0) * SCALE), torch.round((xf ** 2).sum(0) * SCALE)]).long())
        if mode in cc.ADMITS["ay"]:
            d["res"] = torch.clamp(torch.randn(M, Cin, generator=gen) + 0.2, min=0).bfloat16()
            d["y_ref"] = (xf * scale.double() + shift.double() + d["res"].double()).clamp(min=0)
            a = None                                    # the conv's reference is formed on the y the kernel wrote
        else:
            a = torch.clamp(x.float() * scale + shift, min=0).bfloat16().float()
    if a is not None:
        d["ref"] = _conv_f64(g, a, w)
    if mode in cc.EVAL:
        d["osc"], d["osh"] = torch.rand(Cout, generator=gen) + 0.5, torch.randn(Cout, generator=gen) * 0.3
        ref = d["ref"] * d["osc"].double() + d["osh"].double()
        if mode == "eval_res":
            d["res"] = torch.randn(M, max(g["ldc"], Cout), generator=gen).bfloat16()
            ref = ref + d["res"][:, :Cout].double()
        d["ref"] = ref.clamp(min=0)
    return d


def _conv_f64(g, a, w):
    Cout = g["Cout"]
    if g["layout"] == "stem":                           # windows of 8 pixels x 4 channels per kernel row, `stride` pixels apart
        s, Ho, Wo = g["stride"], g["Hout"], g["Wout"]
        af = a.double()
        rows = torch.stack([af[:, kh:kh + s * Ho:s][:, :Ho].reshape(g["N"], Ho, g["W"] * 4) for kh in range(7)], 2)
        win = torch.stack([rows[..., 4 * s * wo:4 * s * wo + 32] for wo in range(Wo)], 2)
        return torch.einsum("nhwkc,okc->nhwo", win, w.double()).reshape(-1, Cout)
    return F.conv2d(a.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, g["stride"],
                    (g["pad"], g["padw"])).permute(0, 2, 3, 1).reshape(-1, Cout)


_ran = {}            # (geometry, mode) -> {variant: results}: the rows of one op that ran so far, for the bit-family comparison


@pytest.mark.parametrize("row", cc.CASES, ids=cc.case_id)
def test_conv_variant_against_f64_and_its_bit_family(lib, row):
    variant, mode, geo = row
    g, d = cc.GEOS[geo], _data(geo, mode)
    Cin, Cout, M = g["Cin"], g["Cout"], g["M"]
    ldc = max(g["ldc"], Cout)
    fused, ay = mode in cc.BN + cc.ADMITS["ay"], mode in cc.ADMITS["ay"]
    t = {"in0": d["x"].cuda(), "w": d["w"].cuda(),
         "out": torch.full((M, ldc), float("nan"), device="cuda", dtype=torch.bfloat16)}
    if variant in cc.NEEDS_PACKED:
        t["w_packed"] = torch.empty_like(t["w"])
        L.check(lib.sat_conv_pack_weights(t["w"].data_ptr(), t["w_packed"].data_ptr(), Cout, Cin, g["KH"] * g["KW"], L.stream()))
    stats = mode if mode in cc.STATS else ("atomic" if fused else "none")
    if stats == "slab":
        t["stat_partial"] = torch.full((lib.sat_conv_tiles_m(M), 2, Cout), float("nan"), device="cuda")
    if stats == "atomic":
        t["stat_acc"] = torch.zeros(2, 2, Cout, dtype=torch.int64, device="cuda")
        t["stat_acc"][1] = 12345                        # the other parity's half is not this launch's to touch
    if mode in cc.EVAL:
        t["scale1"], t["shift1"] = d["osc"].cuda(), d["osh"].cuda()
    if "res" in d:
        t["in1"] = d["res"].cuda()
    if mode in ("bn_table", "ay_table"):
        t["scale0"], t["shift0"] = d["scale"].cuda(), d["shift"].cuda()
    if mode in ("bn_derive", "ay_derive"):
        t["stat_acc1"] = torch.full((2, 2, Cin), 777, dtype=torch.int64, device="cuda")
        t["stat_acc1"][0] = d["sums"].cuda()
        t["gamma1"], t["beta1"] = d["gamma"].cuda(), d["beta"].cuda()
        t["running_mean1"], t["running_var1"] = torch.zeros(Cin, device="cuda"), torch.ones(Cin, device="cuda")
    if ay:
        t["out1"] = torch.full((M, Cin), float("nan"), device="cuda", dtype=torch.bfloat16)
    o = cc.build_op(lib, variant, mode, geo, {k: v.data_ptr() for k, v in t.items()})
    cc.run_named(lib, o)
    torch.cuda.synchronize()

    got = {"out": t["out"][:, :Cout].cpu()}
    out = got["out"].float().double()
    assert torch.isfinite(out).all()
    if ldc > Cout:
        assert torch.isnan(t["out"][:, Cout:].float()).all(), "wrote past Cout"
    ref = d.get("ref")
    if ay:
        got["y"] = t["out1"].cpu()
        yerr = (got["y"].float().double() - d["y_ref"]).abs().max().item()
        print("%s: max |y - f64| = %.3g (bound 6e-2)" % (cc.case_id(row), yerr))
        assert yerr < 6e-2                              # bf16 rounding of |y| < ~8 (test_gpu_conv_ay.py)
        ref = got["y"].float().double() @ d["w"].double().t()
    bound = 3e-2 + 4e-3 * ref.abs().max().item() if fused else 3e-2 + 8e-3 * ref.abs().max().item() if mode in cc.EVAL else 2e-2
    err = (out - ref).abs().max().item()
    print("%s: max |out - f64| = %.3g (bound %.3g)" % (cc.case_id(row), err, bound))
    assert err < bound
    if mode in cc.EVAL:
        assert float(out.min()) >= 0.0
    if stats != "none":
        if stats == "slab":
            got["stats"] = t["stat_partial"].cpu()
            assert torch.isfinite(got["stats"]).all()
            s, q = got["stats"][:, 0].double().sum(0), got["stats"][:, 1].double().sum(0)
        else:
            got["stats"] = t["stat_acc"].cpu()
            assert int((got["stats"][1] - 12345).abs().sum()) == 0
            s, q = got["stats"][0, 0].double() / SCALE, got["stats"][0, 1].double() / SCALE
        print("%s: max |colsum - f64| = %.3g, max |colsumsq - f64| = %.3g" % (cc.case_id(row), (s - ref.sum(0)).abs().max().item(),
                                                                             (q - (ref ** 2).sum(0)).abs().max().item()))
        if fused:
            np.testing.assert_allclose(s.numpy(), ref.sum(0).numpy(), rtol=0, atol=2e-3 * M ** 0.5 + 1e-3)
            np.testing.assert_allclose(q.numpy(), (ref ** 2).sum(0).numpy(), rtol=5e-4, atol=5e-3)
        else:
            np.testing.assert_allclose(s.numpy(), ref.sum(0).numpy(), rtol=0, atol=1e-3 * M ** 0.5 + 1e-4)
            np.testing.assert_allclose(q.numpy(), (ref ** 2).sum(0).numpy(), rtol=2e-4, atol=1e-3)
    if mode in ("bn_derive", "ay_derive"):              # running statistics updated once, the other parity's sums cleared
        rows = d["rows"]
        got["run"] = torch.stack([t["running_mean1"], t["running_var1"]]).cpu()
        assert int(t["stat_acc1"][1].abs().sum()) == 0
        np.testing.assert_allclose(got["run"][0].numpy(), (0.1 * d["mean"]).numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(got["run"][1].numpy(), (0.9 + 0.1 * d["var"] * rows / (rows - 1)).numpy(), rtol=1e-4)

    # the bit family: every other variant that ran this op so far
    for v, other in _ran.setdefault((geo, mode), {}).items():
        if lib.sat_conv_variant_family(v) == lib.sat_conv_variant_family(variant):
            assert torch.equal(got["out"], other["out"]), "output bits differ from variant %d (same output family)" % v
            if ay:
                assert torch.equal(got["y"], other["y"]), "y bits differ from variant %d" % v
            if "run" in got:
                assert torch.equal(got["run"], other["run"]), "running statistics differ from variant %d" % v
        if "stats" in got and lib.sat_conv_variant_signature(v) == lib.sat_conv_variant_signature(variant):
            assert torch.equal(got["stats"], other["stats"]), "statistics bits differ from variant %d (same signature)" % v
    _ran[(geo, mode)][variant] = got

