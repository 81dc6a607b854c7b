"""CPU reference of one LSTM layer over a packed batch (`sat_lstm_fwd` / `sat_lstm_bwd`, models.py:52 `self.lstm(packed)` and its
backward, train.py:144): the forward recurrence and explicit back-propagation through time written out by hand over PACKED rows,
in float64 -- or in another `dtype`, which makes the same code the float32 restatement whose error against float64 sets the GPU
sweep's tolerance (tests/test_gpu_lstm_layer_edges.py).  No GPU import.  tests/test_lstm_layer_reference_host.py validates it
against torch.nn.LSTM + autograd, re-measures `F32_ERR`, and proves that the case list below notices each of `MUTATIONS`.

Packed layout (torch's pack_padded_sequence, batch_first): step t owns the rows [prefix[t], prefix[t] + batch_sizes[t]), row r of a
step is batch row r, batch_sizes never grow.  Gate order i, f, g, o.  Tapes as the kernels write them: GA activated gates [N, 4H],
CS cell states, HS outputs, HP the previous hidden state of every row (zeros for step 0)."""
import collections

import torch

TOL_FACTOR = 8.0            # GPU tolerance = TOL_FACTOR x the f32 restatement's error: the kernels sum K in another order than torch
FLOOR_ULP = 2.0 ** -23      # ... and never below one float32 ulp of the output's largest magnitude (a restatement error of exactly 0)

FWD_OUTPUTS = ("GA", "CS", "HS", "HP")
BWD_OUTPUTS = ("DG", "dw_ih", "dw_hh", "db", "dX")
OUTPUTS = FWD_OUTPUTS + BWD_OUTPUTS

Case = collections.namedtuple("Case", "B T In H batch_sizes fwd_plan bwd_plan")


def batch_sizes_of(lengths):
    assert list(lengths) == sorted(lengths, reverse=True) and lengths[-1] >= 1
    return [sum(1 for l in lengths if l > t) for t in range(lengths[0])]


def _ragged(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = sorted((int(x) for x in torch.randint(1, T + 1, (B,), generator=g)), reverse=True)
    lengths[0] = T
    return batch_sizes_of(lengths)


# name -> case.  The plan columns are what sat_lstm_fwd_plan / sat_lstm_bwd_plan answer on a 256-CU device (rows per group of the
# persistent forward: 0, 8, 16; persistent backward: 0, 1) -- the GPU test asserts them before it compares anything.
PLAN_CUS = 256
CASES = collections.OrderedDict([
    # T = 1, H < 16: no persistent form, no forward workspace, one K block
    ("b1_t1_in4_h4", Case(1, 1, 4, 4, batch_sizes_of([1]), 0, 0)),
    # H % 16 != 0, K tails in both operand pairs
    ("b3_t5_in20_h20", Case(3, 5, 20, 20, batch_sizes_of([5, 3, 1]), 0, 0)),
    # NKB = 2; the second group has one row and lives one step: leaves at t = 1 forward, joins at t = 0 backward, never exchanges
    ("b9_t4_in8_h32", Case(9, 4, 8, 32, batch_sizes_of([4] * 8 + [1]), 8, 1)),
    # T = kMaxT: the full prefix table, 32 phase cycles per parity buffer, backward tags up to step 65
    ("b8_t64_in4_h32", Case(8, 64, 4, 32, [8] * 64, 8, 1)),
    # T > kMaxT: both directions fall back to one launch per step
    ("b8_t65_in4_h32", Case(8, 65, 4, 32, [8] * 65, 0, 0)),
    # NKB = 6, TPW = 2, wave 3 without a tile; three groups, the last with one row; cuts inside a group (13, 12, 3) and exactly at
    # a group boundary (8); In % 16 != 0
    ("b17_t6_in36_h96", Case(17, 6, 36, 96, [17, 13, 12, 9, 8, 3], 8, 1)),
    # NKB = 8; the second group drops to one row, then leaves
    ("b16_t3_in32_h128", Case(16, 3, 32, 128, [16, 9, 8], 8, 1)),
    # persistent backward at H = 256 (NKB = 16)
    ("b24_t5_in16_h256", Case(24, 5, 16, 256, _ragged(24, 5, 24 * 5 + 256), 8, 1)),
    # 16-row forward chosen by batch size (17 x 16 > 256 CUs), <16, 16>; last group with 2, then 1, live rows of 16; per-step
    # backward with three 64-row chunks
    ("b130_t2_in8_h256", Case(130, 2, 8, 256, [130, 129], 16, 0)),
    # 16-row forward chosen by batch size (9 x 32 > 256), <32, 16>; last group half full, then one row, then gone; per-step
    # backward with a second 64-row chunk of 8, then 1, rows
    ("b72_t3_in16_h512", Case(72, 3, 16, 512, [72, 65, 64], 16, 0)),
    # the calls that share ONE backward workspace with b17_t6_in36_h96 (N, then B, change from call to call)
    ("reuse_b17_t2", Case(17, 2, 36, 96, [17, 10], 8, 1)),
    ("reuse_b17_t5", Case(17, 5, 36, 96, [17, 16, 16, 7, 1], 8, 1)),
    ("reuse_b9_t3", Case(9, 3, 36, 96, [9, 8, 2], 8, 1)),
    # tanh(c) rounds to 1.0f only for |c| > 9.01 and |c_t| <= t + 1, so h = +-1.0f exactly needs T >= 10 -- no T of the table above
    # gets there (tanh(6) = 1 - 1.2e-5): the extreme of the forward's self-tag has this case of its own (value kind "saturated")
    ("b9_t12_in8_h32", Case(9, 12, 8, 32, batch_sizes_of([12] * 8 + [1]), 8, 1)),
])
SWEEP = list(CASES)[:10]
REUSE_SEQUENCE = ["b17_t6_in36_h96", "reuse_b17_t2", "reuse_b17_t5", "reuse_b9_t3"]
BF16_CASES = ["b9_t4_in8_h32", "b17_t6_in36_h96", "b72_t3_in16_h512"]
VALUE_CASES = ["b9_t4_in8_h32", "b17_t6_in36_h96"]
VALUE_KINDS = ["saturated", "zero_w", "nan_row"]
SATURATED_EXACT_CASE = "b9_t12_in8_h32"
NAN_BATCH_ROW = 1

# every (case, value kind, bf16 GEMM operands) the GPU test runs = the keys of F32_ERR
RUNS = ([(n, "plain", False) for n in SWEEP] + [(n, "plain", False) for n in REUSE_SEQUENCE[1:]] + [(n, "plain", True) for n in BF16_CASES]
        + [(n, k, False) for n in VALUE_CASES for k in VALUE_KINDS] + [(SATURATED_EXACT_CASE, "saturated", False)])


def inputs(name, kind="plain"):
    """float32 inputs of one case, deterministic per (case, kind): X [N, In], w_ih, w_hh, b_ih, b_hh, dHS [N, H]"""
    c = CASES[name]
    N = sum(c.batch_sizes)
    g = torch.Generator().manual_seed(1000 * list(CASES).index(name) + 17 * (["plain"] + VALUE_KINDS).index(kind) + 3)
    k = 1.0 / c.H ** 0.5
    u = lambda *s: torch.empty(*s).uniform_(-k, k, generator=g)
    d = dict(X=torch.randn(N, c.In, generator=g), w_ih=u(4 * c.H, c.In), w_hh=u(4 * c.H, c.H), b_ih=u(4 * c.H), b_hh=u(4 * c.H),
             dHS=torch.randn(N, c.H, generator=g) * 0.1)
    H = c.H
    if kind == "saturated":
        # i = o = 1; g = +-1 alternating by unit; f = 1 on the units 0, 1 of every four (c walks to +T and to -T, h to tanh(+-T)),
        # f = 0 on the units 2, 3 (c = +-1 every step).  (f = 0 on every ODD unit would stop all the units with g = -1: no c = -T.)
        unit = torch.arange(H)
        g_sign = 1.0 - 2.0 * (unit % 2).float()
        f_sign = 1.0 - 2.0 * ((unit % 4) >= 2).float()
        d["b_ih"] = torch.cat([torch.full((H,), 40.0), 40.0 * f_sign, 40.0 * g_sign, torch.full((H,), 40.0)])
    elif kind == "zero_w":
        for key in ("w_ih", "w_hh", "b_ih", "b_hh"):
            d[key] = torch.zeros_like(d[key])
    elif kind == "nan_row":
        d["X"][NAN_BATCH_ROW] = float("nan")          # packed row 1 = batch row 1 at step 0
    else:
        assert kind == "plain"
    return d


def _rnd(t, gemm_round):
    """operand rounding of the bf16-pipe form: round to nearest even into `gemm_round`, computed on in t's dtype"""
    return t if gemm_round is None else t.to(torch.float32).to(gemm_round).to(t.dtype)


def _prefix(batch_sizes):
    p = [0]
    for n in batch_sizes:
        p.append(p[-1] + n)
    return p


MUTATIONS = ("dc_carry_for_ended_rows", "dh_carry_dropped_for_last_row_of_group", "c_t_for_c_prev_in_forget_gradient",
             "hp_from_wrong_parity", "b_hh_omitted", "last_packed_row_left_out_of_dw_hh", "rows_8_15_given_rows_0_7_h")
FWD_MUTATIONS = ("hp_from_wrong_parity", "b_hh_omitted", "rows_8_15_given_rows_0_7_h")


def forward(X, w_ih, w_hh, b_ih, b_hh, batch_sizes, dtype=torch.float64, gemm_round=None, mutation=None):
    """-> dict GA, CS, HS, HP.  `mutation`: one of MUTATIONS (the host test's proof that the case list notices it)"""
    X, w_ih, w_hh, b_ih, b_hh = (t.to(dtype) for t in (X, w_ih, w_hh, b_ih, b_hh))
    H, B, pre = w_hh.shape[1], batch_sizes[0], _prefix(batch_sizes)
    N = pre[-1]
    xg = _rnd(X, gemm_round) @ _rnd(w_ih, gemm_round).t() + b_ih
    if mutation != "b_hh_omitted":
        xg = xg + b_hh
    GA, CS, HS, HP = (torch.zeros(N, w, dtype=dtype) for w in (4 * H, H, H, H))
    h_hist = [torch.zeros(B, H, dtype=dtype)]                    # h_hist[t] = h_{t-1} of every batch row (rows that ended keep theirs)
    c = torch.zeros(B, H, dtype=dtype)
    for t, n in enumerate(batch_sizes):
        rows = slice(pre[t], pre[t] + n)
        h_prev = h_hist[t]
        if mutation == "hp_from_wrong_parity" and t > 0:
            h_prev = h_hist[t - 1]                               # the other parity buffer: h of two steps ago
        h_prev = h_prev[:n].clone()
        if mutation == "rows_8_15_given_rows_0_7_h":
            for r in range(n):
                if r % 16 >= 8:
                    h_prev[r] = h_hist[t][r - 8]
        HP[rows] = h_prev
        z = xg[rows] + h_prev @ w_hh.t()
        i, f, gg, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
        c_new = f * c[:n] + i * gg
        h_new = o * torch.tanh(c_new)
        GA[rows], CS[rows], HS[rows] = torch.cat([i, f, gg, o], 1), c_new, h_new
        c = torch.cat([c_new, c[n:]])
        h_hist.append(torch.cat([h_new, h_hist[t][n:]]))
    return dict(GA=GA, CS=CS, HS=HS, HP=HP)


def backward(dHS, X, w_ih, w_hh, GA, CS, HP, batch_sizes, dtype=torch.float64, gemm_round=None, mutation=None):
    """explicit BPTT over packed rows -> dict DG (d loss / d gate pre-activations), dw_ih, dw_hh, db (= db_ih = db_hh), dX.
    The carries live per PACKED row: row r of step t takes dh and dc from packed row prefix[t+1] + r, and only while r < n_next."""
    dHS, X, w_ih, w_hh, GA, CS, HP = (t.to(dtype) for t in (dHS, X, w_ih, w_hh, GA, CS, HP))
    H, pre, T = w_hh.shape[1], _prefix(batch_sizes), len(batch_sizes)
    N = pre[-1]
    DG = torch.zeros(N, 4 * H, dtype=dtype)
    DC = torch.zeros(N, H, dtype=dtype)                           # dc_t * f_t: what row (t, r) hands to row (t-1, r)
    for t in range(T - 1, -1, -1):
        n = batch_sizes[t]
        n_next = batch_sizes[t + 1] if t + 1 < T else 0
        rows = slice(pre[t], pre[t] + n)
        dh = dHS[rows].clone()
        dc_in = torch.zeros(n, H, dtype=dtype)
        for r in range(n_next):
            src = pre[t + 1] + r
            last_of_group = r % 8 == 7 or r == n_next - 1
            if not (mutation == "dh_carry_dropped_for_last_row_of_group" and last_of_group):
                dh[r] += DG[src] @ w_hh
            dc_in[r] = DC[src]
        if mutation == "dc_carry_for_ended_rows" and t + 1 < T:
            for r in range(n_next, n):                            # a row that ended at t: its "next" packed row belongs to step t+2
                if pre[t + 1] + r < N:
                    dc_in[r] = DC[pre[t + 1] + r]
        i, f, gg, o = GA[rows, :H], GA[rows, H:2 * H], GA[rows, 2 * H:3 * H], GA[rows, 3 * H:]
        tc = torch.tanh(CS[rows])
        c_prev = CS[pre[t - 1]:pre[t - 1] + n] if t > 0 else torch.zeros(n, H, dtype=dtype)
        if mutation == "c_t_for_c_prev_in_forget_gradient":
            c_prev = CS[rows]
        d_o = dh * tc
        dc = dh * o * (1.0 - tc * tc) + dc_in
        DG[rows] = torch.cat([dc * gg * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - gg * gg), d_o * o * (1.0 - o)], 1)
        DC[rows] = dc * f
    out = dict(DG=DG, db=DG.sum(0))
    out.update(batched_products(DG, HP, X, w_ih, dtype=dtype, gemm_round=gemm_round,
                                drop_last_row_of_dw_hh=mutation == "last_packed_row_left_out_of_dw_hh"))
    return out


def batched_products(DG, HP, X, w_ih, dtype=torch.float64, gemm_round=None, drop_last_row_of_dw_hh=False):
    """the three batched products behind the backward recurrence, from the given tapes: dw_ih = DG^T X, dw_hh = DG^T HP,
    dX = DG W_ih, every operand rounded to `gemm_round` first.  (The GPU test of the bf16-pipe form feeds it the DEVICE's DG and HP:
    that isolates the bf16 GEMMs from bf16 ulp flips between two nearly equal DG.)"""
    dgr, hp, x, w = (_rnd(t.to(dtype), gemm_round) for t in (DG, HP, X, w_ih))
    m = DG.shape[0] - (1 if drop_last_row_of_dw_hh else 0)
    return dict(dw_ih=dgr.t() @ x, dw_hh=dgr[:m].t() @ hp[:m], dX=dgr @ w)


def layer(name, kind="plain", dtype=torch.float64, gemm_round=None, fwd_mutation=None, bwd_mutation=None):
    """forward + backward of one case on its own tapes (as the decoder feeds them) -> dict over OUTPUTS"""
    d, bs = inputs(name, kind), CASES[name].batch_sizes
    out = forward(d["X"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"], bs, dtype=dtype, gemm_round=gemm_round, mutation=fwd_mutation)
    if kind != "nan_row":                                         # nan_row is a forward-only case
        out.update(backward(d["dHS"], d["X"], d["w_ih"], d["w_hh"], out["GA"], out["CS"], out["HP"], bs, dtype=dtype,
                            gemm_round=gemm_round, mutation=bwd_mutation))
    return out


_cache = {}


def reference(name, kind="plain", bf16=False):
    """the float64 outputs of one run, computed once per process; treat as read-only"""
    key = (name, kind, bf16)
    if key not in _cache:
        _cache[key] = layer(name, kind, gemm_round=torch.bfloat16 if bf16 else None)
    return _cache[key]


def max_err(got, ref):
    """max |got - ref| over the entries where ref is a number; the NaN entries must be the same ones"""
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "NaN pattern differs"
    return (got.double() - ref)[~nan].abs().max().item() if (~nan).any() else 0.0


def f32_error(name, kind="plain", bf16=False):
    """max abs error of the float32 restatement against float64, per output (the figures frozen in F32_ERR)"""
    ref = reference(name, kind, bf16)
    f32 = layer(name, kind, dtype=torch.float32, gemm_round=torch.bfloat16 if bf16 else None)
    if bf16:
        # the three bf16 products are compared on the SAME rounded tapes (see batched_products): their restatement is the float32
        # accumulation of the float64 reference's rounded tapes, so that it measures the product and no bf16 ulp flip of an operand
        d = inputs(name, kind)
        f32.update(batched_products(ref["DG"], ref["HP"], d["X"], d["w_ih"], dtype=torch.float32, gemm_round=torch.bfloat16))
    return ref, f32, {k: max_err(f32[k], ref[k]) for k in ref}


def tolerance(name, kind, bf16, output, ref):
    """what the GPU test allows for one output: TOL_FACTOR x the frozen restatement error, at least one f32 ulp of max |ref|"""
    frozen = f32_err(name, kind, bf16)[output]
    finite = ref[~torch.isnan(ref)]
    return max(TOL_FACTOR * frozen, FLOOR_ULP * (finite.abs().max().item() if finite.numel() else 0.0))


# The float32 restatement's max abs error against float64 at every run of the sweep, as test_lstm_layer_reference_host.py measured
# it (3 digits; torch 2.x CPU).  FROZEN: torch's float32 summation order depends on the host, so the GPU test reads its tolerance
# from here, not from the machine it happens to run on; the host test re-measures and compares.
# (case, kind, bf16 GEMM operands): OUTPUTS order -- GA, CS, HS, HP, DG, dw_ih, dw_hh, db, dX (forward only for nan_row)
F32_ERR = {
    ("b1_t1_in4_h4", "plain", False): (3.47e-08, 2.42e-08, 8.36e-09, 0, 2.07e-09, 1.56e-09, 0, 2.07e-09, 1.54e-09),
    ("b3_t5_in20_h20", "plain", False): (1.15e-07, 1.49e-07, 6.96e-08, 6.96e-08, 1.35e-08, 3.74e-08, 6.39e-09, 2.73e-08, 1.21e-08),
    ("b9_t4_in8_h32", "plain", False): (7.07e-08, 6.51e-08, 4.22e-08, 3.73e-08, 1.23e-08, 1.16e-07, 8.67e-09, 4.51e-08, 1.92e-08),
    ("b8_t64_in4_h32", "plain", False): (9.42e-08, 8.94e-08, 5.49e-08, 5.49e-08, 2.55e-08, 6.75e-07, 1.49e-07, 4.77e-07, 2.19e-08),
    ("b8_t65_in4_h32", "plain", False): (9.25e-08, 8.77e-08, 6.38e-08, 6.38e-08, 2.11e-08, 5.3e-07, 1.51e-07, 4.07e-07, 1.78e-08),
    ("b17_t6_in36_h96", "plain", False): (1.96e-07, 1.23e-07, 8.22e-08, 6.08e-08, 2.91e-08, 2.08e-07, 1.95e-08, 1.16e-07, 3.3e-08),
    ("b16_t3_in32_h128", "plain", False): (1.61e-07, 9.46e-08, 5.22e-08, 5.2e-08, 1.7e-08, 1.49e-07, 1.01e-08, 7.3e-08, 4e-08),
    ("b24_t5_in16_h256", "plain", False): (8.3e-08, 5.93e-08, 3.66e-08, 3.42e-08, 2.02e-08, 2.47e-07, 1.48e-08, 1.04e-07, 2.88e-08),
    ("b130_t2_in8_h256", "plain", False): (6.22e-08, 4.35e-08, 2.7e-08, 2.47e-08, 2.04e-08, 9.33e-07, 1.6e-08, 2.02e-07, 2.8e-08),
    ("b72_t3_in16_h512", "plain", False): (8.57e-08, 5.03e-08, 2.63e-08, 2.63e-08, 2.36e-08, 7.96e-07, 2.37e-08, 2.13e-07, 3e-08),
    ("reuse_b17_t2", "plain", False): (1.66e-07, 1.01e-07, 6.64e-08, 6.23e-08, 2.14e-08, 1.1e-07, 8.19e-09, 5.09e-08, 3.67e-08),
    ("reuse_b17_t5", "plain", False): (1.83e-07, 1.29e-07, 7.32e-08, 7.32e-08, 2.17e-08, 2.29e-07, 1.65e-08, 7.83e-08, 3.49e-08),
    ("reuse_b9_t3", "plain", False): (1.56e-07, 9.9e-08, 5.27e-08, 4.89e-08, 2.32e-08, 8.1e-08, 7.72e-09, 6.37e-08, 3.41e-08),
    ("b9_t4_in8_h32", "plain", True): (6.78e-08, 7.91e-08, 3.96e-08, 3.45e-08, 1.56e-08, 2.68e-08, 1.86e-09, 5.7e-08, 8.88e-09),
    ("b17_t6_in36_h96", "plain", True): (9.32e-08, 9.39e-08, 5.89e-08, 5.89e-08, 1.89e-08, 9.13e-08, 7.45e-09, 8.13e-08, 2.52e-08),
    ("b72_t3_in16_h512", "plain", True): (6.05e-08, 4.01e-08, 2.78e-08, 2.78e-08, 2.2e-08, 3.61e-07, 1.22e-08, 2.31e-07, 1.31e-08),
    ("b9_t4_in8_h32", "saturated", False): (1.51e-22, 0, 2.88e-08, 2.78e-08, 7.45e-24, 1.71e-23, 1.41e-23, 1.41e-23, 9.31e-25),
    ("b9_t4_in8_h32", "zero_w", False): (0, 0, 0, 0, 3.73e-09, 7.89e-08, 0, 3.56e-08, 0),
    ("b9_t4_in8_h32", "nan_row", False): (8.47e-08, 6.54e-08, 4.65e-08, 3.81e-08),
    ("b17_t6_in36_h96", "saturated", False): (8.43e-23, 0, 2.88e-08, 2.88e-08, 4.21e-24, 1.96e-23, 7.79e-24, 8.49e-24, 7.19e-25),
    ("b17_t6_in36_h96", "zero_w", False): (0, 0, 0, 0, 4.83e-09, 2.7e-07, 0, 6.09e-08, 0),
    ("b17_t6_in36_h96", "nan_row", False): (2.04e-07, 1.31e-07, 8.83e-08, 6.74e-08),
    ("b9_t12_in8_h32", "saturated", False): (7.15e-23, 0, 2.91e-08, 2.91e-08, 4.17e-24, 1.1e-23, 1.08e-23, 1.02e-23, 8.87e-25),
}


def f32_err(name, kind="plain", bf16=False):
    """the frozen errors of one run as a dict by output name"""
    return dict(zip(OUTPUTS, F32_ERR[(name, kind, bf16)]))
