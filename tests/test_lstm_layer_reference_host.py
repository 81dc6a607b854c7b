"""CPU: tests/lstm_layer_reference.py is validated before the GPU sweep (tests/test_gpu_lstm_layer_edges.py) trusts it -- against
float64 torch.nn.LSTM over pack_padded_sequence, torch.nn.LSTMCell and autograd; the float32 restatement's error against float64
is re-measured at every run of the sweep and compared with the frozen table the GPU tolerance is read from; each mutation of
`MUTATIONS` must exceed that tolerance at one case at least; and the conditions the case list promises hold.  Run with -s to print
the table the GPU test's docstring records."""
import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

import lstm_layer_reference as R

FINITE_RUNS = [(n, k) for n, k, bf in R.RUNS if k != "nan_row" and not bf]


def close(got, want, what, rel=1e-12):
    """equal to `rel` of the output's largest magnitude"""
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= rel * scale, (what, err, scale)


def torch_layer(name, kind):
    """the independent derivation: nn.LSTM on the padded batch + autograd; nn.LSTMCell for the per-step states; nn.LSTM with an
    identity input weight, whose input gradient is d loss / d gate pre-activations"""
    c = R.CASES[name]
    d = {k: v.double() for k, v in R.inputs(name, kind).items()}
    bs = torch.tensor(c.batch_sizes)
    padded, lens = pad_packed_sequence(PackedSequence(d["X"], bs), batch_first=True)
    padded.requires_grad_(True)
    packed = pack_padded_sequence(padded, lens, batch_first=True)
    assert torch.equal(packed.data, d["X"]) and packed.batch_sizes.tolist() == c.batch_sizes
    lstm = torch.nn.LSTM(c.In, c.H, batch_first=True).double()
    with torch.no_grad():
        for p, key in ((lstm.weight_ih_l0, "w_ih"), (lstm.weight_hh_l0, "w_hh"), (lstm.bias_ih_l0, "b_ih"), (lstm.bias_hh_l0, "b_hh")):
            p.copy_(d[key])
    out, _ = lstm(packed)
    (out.data * d["dHS"]).sum().backward()
    got = dict(HS=out.data.detach(), dw_ih=lstm.weight_ih_l0.grad, dw_hh=lstm.weight_hh_l0.grad, db=lstm.bias_ih_l0.grad,
               db_hh=lstm.bias_hh_l0.grad, dX=pack_padded_sequence(padded.grad, lens, batch_first=True).data)
    # per-step states from torch's cell
    cell = torch.nn.LSTMCell(c.In, c.H).double()
    with torch.no_grad():
        for p, key in ((cell.weight_ih, "w_ih"), (cell.weight_hh, "w_hh"), (cell.bias_ih, "b_ih"), (cell.bias_hh, "b_hh")):
            p.copy_(d[key])
        h, cc = torch.zeros(c.B, c.H, dtype=torch.float64), torch.zeros(c.B, c.H, dtype=torch.float64)
        CS, HP, off = [], [], 0
        for n in c.batch_sizes:
            HP.append(h[:n])
            hn, cn = cell(d["X"][off:off + n], (h[:n], cc[:n]))
            CS.append(cn)
            h, cc, off = torch.cat([hn, h[n:]]), torch.cat([cn, cc[n:]]), off + n
    got["CS"], got["HP"] = torch.cat(CS), torch.cat(HP)
    # DG: the x-gates as the input of an LSTM whose input weight is the identity
    xg = (d["X"] @ d["w_ih"].t() + d["b_ih"] + d["b_hh"]).requires_grad_(True)
    ident = torch.nn.LSTM(4 * c.H, c.H, batch_first=True).double()
    with torch.no_grad():
        ident.weight_ih_l0.copy_(torch.eye(4 * c.H, dtype=torch.float64))
        ident.weight_hh_l0.copy_(d["w_hh"])
        ident.bias_ih_l0.zero_()
        ident.bias_hh_l0.zero_()
    out2, _ = ident(PackedSequence(xg, bs))
    (out2.data * d["dHS"]).sum().backward()
    got["DG"] = xg.grad
    return got


@pytest.mark.parametrize("name,kind", FINITE_RUNS)
def test_reference_equals_torch_lstm_and_autograd(name, kind):
    """forward and hand-written BPTT against float64 nn.LSTM over pack_padded_sequence + autograd, 1e-12 relative"""
    ref, want = R.reference(name, kind), torch_layer(name, kind)
    for key in ("HS", "CS", "HP", "DG", "dw_ih", "dw_hh", "db", "dX"):
        assert torch.isfinite(ref[key]).all() and ref[key].dtype == torch.float64, key
        close(ref[key], want[key], (name, kind, key))
    close(ref["db"], want["db_hh"], (name, kind, "db_hh"))
    # the activated gates have no output of their own in torch: they must reproduce torch's cell states and outputs
    c, pre = R.CASES[name], R._prefix(R.CASES[name].batch_sizes)
    H = c.H
    i, f, g, o = (ref["GA"][:, k * H:(k + 1) * H] for k in range(4))
    c_prev = torch.zeros_like(want["CS"])
    for t in range(1, c.T):
        n = c.batch_sizes[t]
        c_prev[pre[t]:pre[t] + n] = want["CS"][pre[t - 1]:pre[t - 1] + n]
    close(f * c_prev + i * g, want["CS"], (name, kind, "GA: c = f c_prev + i g"))
    close(o * torch.tanh(want["CS"]), want["HS"], (name, kind, "GA: h = o tanh c"))
    assert float(ref["HP"][:c.B].abs().max()) == 0.0


def test_gemm_round_rounds_the_operands_of_the_four_batched_products_only():
    """gemm_round=bfloat16: the x-gates, dW_ih, dW_hh and dX products see bf16-rounded operands; with operands that are bf16
    already it changes nothing, and the recurrence (W_hh, biases) is never rounded"""
    name = "b9_t4_in8_h32"
    d, bs = R.inputs(name), R.CASES[name].batch_sizes
    r16 = lambda t: t.bfloat16().float()
    a = R.forward(r16(d["X"]), r16(d["w_ih"]), d["w_hh"], d["b_ih"], d["b_hh"], bs)
    b = R.forward(d["X"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"], bs, gemm_round=torch.bfloat16)
    plain = R.forward(d["X"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"], bs)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(b["HS"], plain["HS"])
    gb = R.backward(d["dHS"], d["X"], d["w_ih"], d["w_hh"], b["GA"], b["CS"], b["HP"], bs, gemm_round=torch.bfloat16)
    gp = R.backward(d["dHS"], d["X"], d["w_ih"], d["w_hh"], b["GA"], b["CS"], b["HP"], bs)
    assert torch.equal(gb["DG"], gp["DG"]) and torch.equal(gb["db"], gp["db"])
    dg16 = r16(gb["DG"]).double()
    assert torch.equal(gb["dw_ih"], dg16.t() @ r16(d["X"]).double()) and torch.equal(gb["dw_hh"], dg16.t() @ r16(b["HP"]).double())
    assert torch.equal(gb["dX"], dg16 @ r16(d["w_ih"]).double()) and not torch.equal(gb["dX"], gp["dX"])


def test_f32_restatement_error_at_every_run_of_the_sweep():
    """The figures of lstm_layer_reference.F32_ERR (and of the table in tests/test_gpu_lstm_layer_edges.py): max abs error of the
    float32 restatement against float64 per run and output, re-measured and compared with the frozen table."""
    assert set(R.F32_ERR) == set(R.RUNS)
    for name, kind, bf in R.RUNS:
        ref, _, err = R.f32_error(name, kind, bf)
        frozen = R.f32_err(name, kind, bf)
        print("    (%-20r %-12r %-5r): (%s)," % (name + ",", kind + ",", bf, ", ".join("%.3g" % err[k] for k in R.OUTPUTS if k in err)))
        assert len(R.F32_ERR[(name, kind, bf)]) == len(err)
        for k, v in err.items():
            assert np.isfinite(v), (name, kind, bf, k, v)
            if kind == "plain":         # float32 is a usable yardstick: no further from float64 than 1e-3 of the output's largest magnitude
                assert v <= 1e-3 * ref[k].abs().max().item(), (name, kind, bf, k, v)
            # the frozen table against this host's measurement: the same figure on the host that measured it; elsewhere torch's
            # float32 summation order (vector width, threads) moves it by a small factor -- 16 x is allowed
            assert (v == 0) == (frozen[k] == 0) and frozen[k] / 16 <= v <= frozen[k] * 16, (name, kind, bf, k, v, frozen[k])


def _trips(name, mutation):
    """the outputs at which the mutated reference leaves the GPU test's tolerance at this case"""
    fwd = mutation in R.FWD_MUTATIONS
    ref = R.reference(name)
    mut = R.layer(name, fwd_mutation=mutation if fwd else None, bwd_mutation=None if fwd else mutation)
    keys = R.FWD_OUTPUTS if fwd else R.BWD_OUTPUTS
    if not fwd:
        assert all(torch.equal(mut[k], ref[k]) for k in R.FWD_OUTPUTS)
    return [k for k in keys if (mut[k] - ref[k]).abs().max().item() > R.tolerance(name, "plain", False, k, ref[k])]


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_each_mutation_exceeds_the_gpu_tolerance_at_some_case(mutation):
    """a kernel with this mistake would fail tests/test_gpu_lstm_layer_edges.py: the case list is strong enough"""
    caught = [(name, _trips(name, mutation)) for name in R.SWEEP]
    caught = [(n, k) for n, k in caught if k]
    print("%s: caught at %s" % (mutation, "; ".join("%s (%s)" % (n, ", ".join(k)) for n, k in caught)))
    assert caught, "%s stays within the GPU tolerance at every case: %s" % (mutation, ", ".join(R.SWEEP))


def test_case_list_conditions():
    for name, c in R.CASES.items():
        bs = c.batch_sizes
        assert len(bs) == c.T and bs[0] == c.B and bs[-1] >= 1 and all(a >= b for a, b in zip(bs, bs[1:])), name
        assert R.inputs(name)["X"].shape == (sum(bs), c.In) and c.In % 4 == 0 and c.H % 4 == 0
    assert R.CASES["b9_t4_in8_h32"].batch_sizes == [9, 8, 8, 8] and len(R.CASES["b24_t5_in16_h256"].batch_sizes) == 5
    assert len(set(R.CASES["b24_t5_in16_h256"].batch_sizes)) >= 3                      # ragged indeed
    assert R.REUSE_SEQUENCE[0] == R.SWEEP[5] and len({sum(R.CASES[n].batch_sizes) for n in R.REUSE_SEQUENCE}) == 4
    assert [R.CASES[n].B for n in R.REUSE_SEQUENCE] == [17, 17, 17, 9] and [R.CASES[n].T for n in R.REUSE_SEQUENCE] == [6, 2, 5, 3]


def test_plan_columns_follow_the_documented_envelope_at_256_cus():
    """include/sat_hip.h: 8-row groups at H in {32, 64, 96, 128, 256, 512} while ceil(B/8) * H/16 <= CUs, else 16-row groups at
    H in {256, 512, 1024} while ceil(B/16) * H/16 <= CUs (forward only), T <= 64 -- so a typing mistake in the table shows here,
    not as a failed assertion on the device"""
    for name, c in R.CASES.items():
        fit8 = c.H in (32, 64, 96, 128, 256, 512) and -(-c.B // 8) * (c.H // 16) <= R.PLAN_CUS and c.T <= 64
        fit16 = c.H in (256, 512, 1024) and -(-c.B // 16) * (c.H // 16) <= R.PLAN_CUS and c.T <= 64
        assert c.fwd_plan == (8 if fit8 else 16 if fit16 else 0) and c.bwd_plan == int(fit8), name


def test_saturated_and_zero_w_values_are_the_extremes_they_claim():
    """saturated: c walks to +-T exactly; at T >= 10 the float32 restatement's h is +-1.0f exactly and never beyond (the extreme of
    the forward's self-tagged word: bit 30 of |h| <= 1 is free).  At the sweep's T = 4 and T = 6 tanh(T) < 1 - 1e-5 in any
    arithmetic, so h = +-1.0f is asserted at the T = 12 case.  zero_w: h = 0 exactly, sigmoid gates 0.5 exactly."""
    for name in R.VALUE_CASES + [R.SATURATED_EXACT_CASE]:
        c = R.CASES[name]
        _, f32, _ = R.f32_error(name, "saturated")
        assert f32["HS"].dtype == torch.float32 and torch.isfinite(f32["DG"]).all() and torch.isfinite(f32["dX"]).all()
        assert f32["CS"].max().item() == c.T and f32["CS"].min().item() == -c.T
        assert f32["HS"].abs().max().item() <= 1.0
        assert (f32["DG"] == 0).float().mean().item() > 0.5                                # mostly exact zeros
        if name == R.SATURATED_EXACT_CASE:
            assert (f32["HS"] == 1.0).any() and (f32["HS"] == -1.0).any()
            pre = R._prefix(c.batch_sizes)
            assert (f32["HP"][pre[c.T - 1]:] == 1.0).any() and (f32["HP"][pre[c.T - 1]:] == -1.0).any()      # ... and it is handed on
        else:
            assert f32["HS"].abs().max().item() == pytest.approx(np.tanh(c.T), abs=1e-6)
    for name in R.VALUE_CASES:
        H = R.CASES[name].H
        for out in (R.reference(name, "zero_w"), R.f32_error(name, "zero_w")[1]):
            assert float(out["HS"].abs().max()) == 0.0 and float(out["HP"].abs().max()) == 0.0 and float(out["CS"].abs().max()) == 0.0
            assert torch.equal(out["GA"][:, :2 * H], torch.full_like(out["GA"][:, :2 * H], 0.5))
            assert torch.equal(out["GA"][:, 3 * H:], torch.full_like(out["GA"][:, 3 * H:], 0.5)) and float(out["GA"][:, 2 * H:3 * H].abs().max()) == 0.0


def test_nan_row_stays_in_its_batch_row():
    for name in R.VALUE_CASES:
        c, ref = R.CASES[name], R.reference(name, "nan_row")
        pre = R._prefix(c.batch_sizes)
        assert c.batch_sizes[-1] > R.NAN_BATCH_ROW
        hit = torch.zeros(sum(c.batch_sizes), dtype=torch.bool)
        hit[[pre[t] + R.NAN_BATCH_ROW for t in range(c.T)]] = True
        for key in ("HS", "CS"):
            assert torch.isnan(ref[key][hit]).all() and torch.isfinite(ref[key][~hit]).all(), (name, key)
        assert set(ref) == set(R.FWD_OUTPUTS)
