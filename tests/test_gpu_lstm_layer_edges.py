"""GPU (MI355X): one LSTM layer over a packed batch -- `sat_lstm_fwd` / `sat_lstm_bwd` and their bf16-pipe forms -- in EVERY form the
host picks from (B, H, T), the CU count and the workspace, each through the C ABI against the float64 reference of
tests/lstm_layer_reference.py (validated on the CPU by tests/test_lstm_layer_reference_host.py, which also proves that this case
list notices seven plausible kernel mistakes).

Forms per case: forward without a workspace (one launch per step) and with it (the planned form: persistent with 8- or 16-row
groups, or per step); backward with the minimal workspace (one launch per step) and with the full one (persistent where planned,
else per step with split-K dW_ih / dX), each backward fed the tapes of the forward of its own family, as the decoder does.
`sat_lstm_fwd_plan` / `sat_lstm_bwd_plan` -- the very decision the entry points take -- are asserted against the table below BEFORE
anything is compared, so a case meant for one kernel cannot silently test another; the table is a 256-CU device's, on another CU
count the case skips with both counts in the message.

Conventions: outputs start as NaN, workspaces start NaN-filled, every status word is read back and must be 0, db_hh must be
bit-identical to db_ih, the HP rows of step 0 exactly 0, a workspace that held a backward exchange is handed to
`sat_lstm_ws_release` before it is freed.

  case (B, T, In, H)   batch_sizes            fwd bwd  reaches
  (1, 1, 4, 4)         1                       0   0   T = 1, H < 16: no persistent form, no forward workspace, one K block
  (3, 5, 20, 20)       3 2 2 1 1               0   0   H % 16 != 0, K tails in both operand pairs
  (9, 4, 8, 32)        9 8 8 8                 8   1   NKB = 2; the second group has one row and lives one step
  (8, 64, 4, 32)       8 x 64                  8   1   T = kMaxT: full prefix table, 32 phase cycles per parity, backward tags to 65
  (8, 65, 4, 32)       8 x 65                  0   0   T > kMaxT: both directions fall back
  (17, 6, 36, 96)      17 13 12 9 8 3          8   1   NKB = 6, TPW = 2, wave 3 without a tile; cuts inside a group and at a boundary
  (16, 3, 32, 128)     16 9 8                  8   1   NKB = 8; the second group drops to one row, then leaves
  (24, 5, 16, 256)     ragged, seeded          8   1   persistent backward at H = 256 (NKB = 16)
  (130, 2, 8, 256)     130 129                16   0   16-row forward by batch size (17 x 16 > 256 CUs); per-step backward, 3 chunks
  (72, 3, 16, 512)     72 65 64               16   0   16-row forward by batch size (9 x 32 > 256); last group half full, one row, gone
  (9, 12, 8, 32)       9 8 x 11                8   1   saturated only: h = +-1.0f exactly needs |c| > 9.01, i.e. T >= 10

Value kinds (at (9, 4, 8, 32) and (17, 6, 36, 96)): `saturated` -- gate biases +-40: i = o = 1, g = +-1, f = 1 or 0, c walks to +-T,
gradients mostly exact zeros and finite (h = +-1.0f exactly, the extreme of the forward's self-tagged word, is reached at
(9, 12, 8, 32)); `zero_w` -- all weights and biases 0: h = 0 exactly, the exchanged word is the bare phase bit, sigmoid gates 0.5;
`nan_row` -- X of batch row 1 at step 0 is NaN, forward only: that batch row's HS / CS are NaN from step 0 on in both forms, every
other row stays within its tolerance, the status word stays 0.

bf16 forms ((9, 4, 8, 32), (17, 6, 36, 96), (72, 3, 16, 512)): forward and DG against the reference with bf16-rounded GEMM operands;
dW_ih, dW_hh, dX against the float64 products of the bf16-rounded DEVICE DG and HP (checked one line earlier) with bf16-rounded X
and W_ih: the bf16 GEMMs alone, no bf16 ulp flip between two nearly equal DG.

Workspace reuse: ONE `sat_lstm_bwd_ws_bytes_max` buffer, NaN-filled once, serves four forward + backward pairs whose N and then B
change.

Tolerances.  An output passes within 8 x the max abs error of the float32 torch restatement of the same formulas against float64
at that case and seed (the kernels sum K in another order than torch's float32), at least 2^-23 x max |reference| (one float32
ulp: a restatement error of exactly 0).  HS may instead meet the 5e-6 absolute of
test_lstm_fwd_persistent_equals_per_step_launches.  Nothing here is set from a kernel's output.  The restatement's errors as the
host test measured them (`pytest -s tests/test_lstm_layer_reference_host.py`) and as lstm_layer_reference.F32_ERR keeps them:

  case              kind       bf16   GA       CS       HS       HP       DG       dw_ih    dw_hh    db       dX
  b1_t1_in4_h4      plain      no     3.5e-08  2.4e-08  8.4e-09  0        2.1e-09  1.6e-09  0        2.1e-09  1.5e-09
  b3_t5_in20_h20    plain      no     1.2e-07  1.5e-07  7e-08    7e-08    1.4e-08  3.7e-08  6.4e-09  2.7e-08  1.2e-08
  b9_t4_in8_h32     plain      no     7.1e-08  6.5e-08  4.2e-08  3.7e-08  1.2e-08  1.2e-07  8.7e-09  4.5e-08  1.9e-08
  b8_t64_in4_h32    plain      no     9.4e-08  8.9e-08  5.5e-08  5.5e-08  2.6e-08  6.8e-07  1.5e-07  4.8e-07  2.2e-08
  b8_t65_in4_h32    plain      no     9.3e-08  8.8e-08  6.4e-08  6.4e-08  2.1e-08  5.3e-07  1.5e-07  4.1e-07  1.8e-08
  b17_t6_in36_h96   plain      no     2e-07    1.2e-07  8.2e-08  6.1e-08  2.9e-08  2.1e-07  2e-08    1.2e-07  3.3e-08
  b16_t3_in32_h128  plain      no     1.6e-07  9.5e-08  5.2e-08  5.2e-08  1.7e-08  1.5e-07  1e-08    7.3e-08  4e-08
  b24_t5_in16_h256  plain      no     8.3e-08  5.9e-08  3.7e-08  3.4e-08  2e-08    2.5e-07  1.5e-08  1e-07    2.9e-08
  b130_t2_in8_h256  plain      no     6.2e-08  4.4e-08  2.7e-08  2.5e-08  2e-08    9.3e-07  1.6e-08  2e-07    2.8e-08
  b72_t3_in16_h512  plain      no     8.6e-08  5e-08    2.6e-08  2.6e-08  2.4e-08  8e-07    2.4e-08  2.1e-07  3e-08
  reuse_b17_t2      plain      no     1.7e-07  1e-07    6.6e-08  6.2e-08  2.1e-08  1.1e-07  8.2e-09  5.1e-08  3.7e-08
  reuse_b17_t5      plain      no     1.8e-07  1.3e-07  7.3e-08  7.3e-08  2.2e-08  2.3e-07  1.7e-08  7.8e-08  3.5e-08
  reuse_b9_t3       plain      no     1.6e-07  9.9e-08  5.3e-08  4.9e-08  2.3e-08  8.1e-08  7.7e-09  6.4e-08  3.4e-08
  b9_t4_in8_h32     plain      yes    6.8e-08  7.9e-08  4e-08    3.5e-08  1.6e-08  2.7e-08  1.9e-09  5.7e-08  8.9e-09
  b17_t6_in36_h96   plain      yes    9.3e-08  9.4e-08  5.9e-08  5.9e-08  1.9e-08  9.1e-08  7.5e-09  8.1e-08  2.5e-08
  b72_t3_in16_h512  plain      yes    6.1e-08  4e-08    2.8e-08  2.8e-08  2.2e-08  3.6e-07  1.2e-08  2.3e-07  1.3e-08
  b9_t4_in8_h32     saturated  no     1.5e-22  0        2.9e-08  2.8e-08  7.5e-24  1.7e-23  1.4e-23  1.4e-23  9.3e-25
  b9_t4_in8_h32     zero_w     no     0        0        0        0        3.7e-09  7.9e-08  0        3.6e-08  0
  b9_t4_in8_h32     nan_row    no     8.5e-08  6.5e-08  4.7e-08  3.8e-08
  b17_t6_in36_h96   saturated  no     8.4e-23  0        2.9e-08  2.9e-08  4.2e-24  2e-23    7.8e-24  8.5e-24  7.2e-25
  b17_t6_in36_h96   zero_w     no     0        0        0        0        4.8e-09  2.7e-07  0        6.1e-08  0
  b17_t6_in36_h96   nan_row    no     2e-07    1.3e-07  8.8e-08  6.7e-08
  b9_t12_in8_h32    saturated  no     7.2e-23  0        2.9e-08  2.9e-08  4.2e-24  1.1e-23  1.1e-23  1e-23    8.9e-25
"""
import importlib

import pytest
import torch

import lstm_layer_reference as R

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

NAN = float("nan")
HS_ABS = 5e-6              # test_lstm_fwd_persistent_equals_per_step_launches: the one earlier kernel-level bound (HS against fp64)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = L.load()
    prev = lib.sat_lstm_persist_enable(1)
    yield lib
    lib.sat_lstm_persist_enable(prev)


def st():
    return L.stream()


def sync():
    torch.cuda.synchronize()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def nan_bytes(nbytes):
    """a NaN-filled float32 workspace of at least nbytes (and at least 16) bytes"""
    return nans(max((nbytes + 3) // 4, 4))


def word(ws, byte_off):
    return int(ws.view(torch.int32)[byte_off // 4].item())


def assert_plan(lib, name):
    """the form the entry points will run for this case = the table's, on the device the table was written for"""
    c = R.CASES[name]
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    got = (lib.sat_lstm_fwd_plan(c.B, c.H, c.T), lib.sat_lstm_bwd_plan(c.B, c.H, c.T))
    if cus != R.PLAN_CUS:
        pytest.skip("the plan table is a %d-CU device's; this device has %d CUs (plans %r, table %r)" % (R.PLAN_CUS, cus, got, (c.fwd_plan, c.bwd_plan)))
    assert got == (c.fwd_plan, c.bwd_plan), (name, got)
    assert (lib.sat_lstm_fwd_ws_bytes(c.B, c.H) > 0) == (c.H >= 16 and c.H % 16 == 0)


def device_inputs(name, kind):
    return {k: v.cuda() for k, v in R.inputs(name, kind).items()}


def run_fwd(lib, name, d, ws=None, with_ws=True, mixed=None):
    """sat_lstm_fwd (sat_lstm_fwd_bf16 with `mixed`) -> host tapes; the status word is read back and must be 0"""
    c = R.CASES[name]
    N = sum(c.batch_sizes)
    GA, CS, HS, HP, cst = nans(N, 4 * c.H), nans(N, c.H), nans(N, c.H), nans(N, c.H), nans(c.B, c.H)
    wsb = lib.sat_lstm_fwd_ws_bytes(c.B, c.H) if with_ws else 0
    if with_ws and wsb and ws is None:
        ws = nan_bytes(wsb)
    bs = (L.C.c_int32 * c.T)(*c.batch_sizes)
    args = (d["X"].data_ptr(), d["w_ih"].data_ptr(), d["w_hh"].data_ptr(), d["b_ih"].data_ptr(), d["b_hh"].data_ptr(), bs, c.T, c.In, c.H,
            GA.data_ptr(), CS.data_ptr(), HS.data_ptr(), HP.data_ptr(), cst.data_ptr(), ws.data_ptr() if wsb else None, wsb)
    if mixed is not None:
        L.check(lib.sat_lstm_fwd_bf16(*args, mixed.data_ptr(), mixed.numel(), st()))
    else:
        L.check(lib.sat_lstm_fwd(*args, st()))
    sync()
    soff = lib.sat_lstm_fwd_status_offset(c.B, c.H)
    if wsb:
        assert 0 <= soff == wsb - 64 and word(ws, soff) == 0, "forward status word"
    else:
        assert not with_ws or soff == -1
    return dict(GA=GA, CS=CS, HS=HS, HP=HP)


def run_bwd(lib, name, d, tapes, nbytes=None, ws=None, mixed=None):
    """sat_lstm_bwd (sat_lstm_bwd_bf16 with `mixed`) on the given device tapes -> device gradients.  nbytes: the size the call is
    told; ws: a buffer the caller owns (and releases), else a fresh NaN-filled one that is released here"""
    c = R.CASES[name]
    N = sum(c.batch_sizes)
    full = lib.sat_lstm_bwd_ws_bytes_full(N, c.B, c.In, c.H)
    DG, dwi, dwh = nans(N, 4 * c.H), nans(4 * c.H, c.In), nans(4 * c.H, c.H)
    dbi, dbh, dX = nans(4 * c.H), nans(4 * c.H), nans(N, c.In)
    own = ws is None
    if own:
        ws = nan_bytes(nbytes)
    assert ws.numel() * 4 >= nbytes
    bs = (L.C.c_int32 * c.T)(*c.batch_sizes)
    args = (d["dHS"].data_ptr(), d["X"].data_ptr(), d["w_ih"].data_ptr(), d["w_hh"].data_ptr(), tapes["GA"].data_ptr(), tapes["CS"].data_ptr(),
            tapes["HP"].data_ptr(), bs, c.T, c.In, c.H, DG.data_ptr(), dwi.data_ptr(), dwh.data_ptr(), dbi.data_ptr(), dbh.data_ptr(),
            dX.data_ptr(), ws.data_ptr(), nbytes)
    try:
        if mixed is not None:
            L.check(lib.sat_lstm_bwd_bf16(*args, mixed.data_ptr(), mixed.numel(), st()))
        else:
            L.check(lib.sat_lstm_bwd(*args, st()))
        sync()
        if nbytes >= full:
            soff = lib.sat_lstm_bwd_status_offset(N, c.B, c.In, c.H)
            assert 0 <= soff < full and word(ws, soff) == 0, "backward status word"
    finally:
        if own:
            sync()
            L.check(lib.sat_lstm_ws_release(ws.data_ptr()))
    assert torch.equal(dbh.view(torch.int32), dbi.view(torch.int32)), "db_hh is not bit-identical to db_ih"
    return dict(DG=DG, dw_ih=dwi, dw_hh=dwh, db=dbi, dX=dX)


def compare(tag, name, kind, bf16, got, ref, keys):
    """every output within its tolerance of the float64 reference; the figures are printed before anything is asserted"""
    c = R.CASES[name]
    rows, bad = [], []
    for k in keys:
        g, r = got[k].cpu(), ref[k]
        assert g.shape == r.shape and g.dtype == torch.float32, (tag, k)
        same_nan = torch.equal(torch.isnan(g), torch.isnan(r))
        tol = R.tolerance(name, kind, bf16, k, r)
        if k == "HS":
            tol = max(tol, HS_ABS)
        err = R.max_err(g, r) if same_nan else float("inf")
        rows.append("%s %.3g/%.3g" % (k, err, tol))
        if not err <= tol:
            bad.append((k, err, tol))
    print("%-44s %s" % ("%s %s %s:" % (name, kind, tag), "  ".join(rows)))
    assert not bad, (name, kind, tag, bad)
    if "HP" in keys:
        assert float(got["HP"][:c.B].abs().max().item()) == 0.0, (tag, "HP rows of step 0")


def layer_forms(lib, name, kind, backward=True):
    """the four forms of one case against the float64 reference"""
    c = R.CASES[name]
    N = sum(c.batch_sizes)
    ref, d = R.reference(name, kind), device_inputs(name, kind)
    full = lib.sat_lstm_bwd_ws_bytes_full(N, c.B, c.In, c.H)
    assert lib.sat_lstm_bwd_ws_bytes(c.B, c.H) < full <= lib.sat_lstm_bwd_ws_bytes_max(N, c.B, c.In, c.H)
    for fwd_tag, bwd_tag, with_ws, nbytes in (("fwd per step", "bwd per step", False, lib.sat_lstm_bwd_ws_bytes(c.B, c.H)),
                                              ("fwd planned %d" % c.fwd_plan, "bwd full ws, planned %d" % c.bwd_plan, True, full)):
        tapes = run_fwd(lib, name, d, with_ws=with_ws)
        compare(fwd_tag, name, kind, False, tapes, ref, R.FWD_OUTPUTS)
        if backward:
            grads = run_bwd(lib, name, d, tapes, nbytes)
            compare(bwd_tag, name, kind, False, grads, ref, R.BWD_OUTPUTS)
            assert all(torch.isfinite(v).all() for v in grads.values())
    return ref


@pytest.mark.parametrize("name", R.SWEEP)
def test_lstm_layer_every_form_vs_f64(lib, name):
    """per-step and planned forward, per-step and full-workspace backward: all ten outputs of every form against float64"""
    assert_plan(lib, name)
    layer_forms(lib, name, "plain")


@pytest.mark.parametrize("name", R.VALUE_CASES + [R.SATURATED_EXACT_CASE])
def test_lstm_layer_saturated_gates(lib, name):
    """gate biases of +-40: c = +-T exactly, the gradients mostly exact zeros and finite; at T = 12 h = +-1.0f exactly travels
    through the forward's self-tagged exchange (sign bit and phase bit around an all-ones exponent pattern 0x3f800000)"""
    assert_plan(lib, name)
    c = R.CASES[name]
    ref = layer_forms(lib, name, "saturated")
    assert ref["CS"].max().item() == c.T and ref["CS"].min().item() == -c.T
    if name == R.SATURATED_EXACT_CASE:
        hs = run_fwd(lib, name, device_inputs(name, "saturated"))["HS"].cpu()
        assert (hs == 1.0).any() and (hs == -1.0).any() and hs.abs().max().item() == 1.0


@pytest.mark.parametrize("name", R.VALUE_CASES)
def test_lstm_layer_zero_weights(lib, name):
    """h = 0 exactly: the exchanged word is the bare phase bit; sigmoid gates exactly 0.5"""
    assert_plan(lib, name)
    ref = layer_forms(lib, name, "zero_w")
    assert float(ref["HS"].abs().max()) == 0.0 and float(ref["GA"].max()) == 0.5      # (tolerance 2^-23 x 0 = 0: the device's are exact too)


@pytest.mark.parametrize("name", R.VALUE_CASES)
def test_lstm_layer_nan_row_stays_a_nan_row(lib, name):
    """a diverged run stays a diverged run, and stays in its batch row: NaN in X of batch row 1 at step 0 -> that row's HS / CS are
    NaN at every step in the persistent form (the NaN travels as the pattern of 1.5) exactly as per step; every other row within
    its tolerance; status word 0 (run_fwd)"""
    assert_plan(lib, name)
    c = R.CASES[name]
    assert c.fwd_plan == 8
    ref = layer_forms(lib, name, "nan_row", backward=False)        # compare() demands the same NaN entries as the reference's
    pre = R._prefix(c.batch_sizes)
    hit = [pre[t] + R.NAN_BATCH_ROW for t in range(c.T)]
    assert torch.isnan(ref["HS"][hit]).all() and torch.isnan(ref["CS"][hit]).all() and int(torch.isnan(ref["HS"]).sum()) == c.T * c.H


@pytest.mark.parametrize("name", R.BF16_CASES)
def test_lstm_layer_bf16_pipe_vs_f64_of_the_same_bf16_operands(lib, name):
    """sat_lstm_fwd_bf16 / sat_lstm_bwd_bf16 against float64 arithmetic on bf16-rounded GEMM operands (see the module docstring)"""
    assert_plan(lib, name)
    c = R.CASES[name]
    N = sum(c.batch_sizes)
    ref, d = R.reference(name, "plain", True), device_inputs(name, "plain")
    mb = lib.sat_lstm_mixed_ws_bytes(N, c.In, c.H)
    assert mb > 0
    mixed = torch.full((mb,), 0xFF, dtype=torch.uint8, device="cuda")           # bf16 0xffff = NaN
    tapes = run_fwd(lib, name, d, mixed=mixed)
    compare("bf16 fwd planned %d" % c.fwd_plan, name, "plain", True, tapes, ref, R.FWD_OUTPUTS)
    grads = run_bwd(lib, name, d, tapes, lib.sat_lstm_bwd_ws_bytes_full(N, c.B, c.In, c.H), mixed=mixed)
    compare("bf16 bwd recurrence", name, "plain", True, grads, ref, ("DG", "db"))
    host = R.inputs(name, "plain")
    prod = R.batched_products(grads["DG"].cpu(), tapes["HP"].cpu(), host["X"], host["w_ih"], gemm_round=torch.bfloat16)
    compare("bf16 bwd products of the device tapes", name, "plain", True, grads, prod, ("dw_ih", "dw_hh", "dX"))


def test_lstm_bwd_one_workspace_serves_calls_of_changing_n_and_b(lib):
    """production hands ONE sat_lstm_bwd_ws_bytes_max buffer to calls whose N changes every step (decoder.py LstmWorkspaces): the
    exchange is cleared once per address and never again, granules carry epoch tags.  Four forward + backward pairs on one
    NaN-filled buffer: B = 17 with T = 6, 2, 5 (N = 62, 27, 57), then B = 9, T = 3 (another exchange layout in the same bytes)."""
    first = R.CASES[R.REUSE_SEQUENCE[0]]
    nbytes = lib.sat_lstm_bwd_ws_bytes_max(first.B * first.T, first.B, first.In, first.H)
    bws = nan_bytes(nbytes)
    fws = nan_bytes(lib.sat_lstm_fwd_ws_bytes(first.B, first.H))
    offsets = []
    try:
        for name in R.REUSE_SEQUENCE:
            assert_plan(lib, name)
            c = R.CASES[name]
            N = sum(c.batch_sizes)
            assert (c.In, c.H) == (first.In, first.H) and lib.sat_lstm_bwd_ws_bytes_full(N, c.B, c.In, c.H) <= nbytes
            ref, d = R.reference(name), device_inputs(name, "plain")
            tapes = run_fwd(lib, name, d, ws=fws)
            compare("reuse fwd", name, "plain", False, tapes, ref, R.FWD_OUTPUTS)
            grads = run_bwd(lib, name, d, tapes, nbytes, ws=bws)                 # told the whole buffer: >= full, so persistent
            compare("reuse bwd", name, "plain", False, grads, ref, R.BWD_OUTPUTS)
            offsets.append(lib.sat_lstm_bwd_status_offset(N, c.B, c.In, c.H))
        assert offsets[0] == offsets[1] == offsets[2] and len({sum(R.CASES[n].batch_sizes) for n in R.REUSE_SEQUENCE}) == 4
    finally:
        sync()
        L.check(lib.sat_lstm_ws_release(bws.data_ptr()))
