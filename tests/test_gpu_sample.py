"""GPU (MI355X): the filtered draw `sat_sample_filtered` (temperature, top-k, nucleus) against the float64 reference
tests/sample_reference.py -- a sweep over row lengths, strides, row counts and filter settings, planted rows (ties at both cuts,
+-0.0, -inf columns, poisoned pad columns), determinism -- and the two decode loops built on it, `DecoderRNN.sample_stochastic`
(`sat_sample_decode`) and `ShowAttendTellModel.sample_stochastic_features`, replayed step by step from their own logits.

Excuses (both of the sweep, both bounded at 1 % of its cases, both counted on the reference BEFORE the device result is read):
a nucleus decision whose clearance from top_p * Z is under 1e-6 may differ by the one boundary token; a draw whose two best
perturbed scores are closer than 1e-4 (tests/test_gpu_ss.py's bound for the f32 noise) may differ."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import sample_reference as R
import scst_attend_reference as SA

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
from oracle import attend as OA  # noqa: E402

BAND, CLOSE = 1e-6, 1e-4
LOGP_TOL = 2.0 ** -22                 # one rounding to f32 (2^-24 relative), fourfold
PAD = 1e30                            # what the sweep's pad columns hold: a candidate there would win every draw


def pad4(v):
    return (v + 3) // 4 * 4


def device(x, ldl, R_, tau, k, p, seed, t, rank, pad=PAD, want_logp=True, want_kept=True):
    """one sat_sample_filtered call on the first R_ rows of x [*, V] laid out with row stride ldl: (ids i64, kept i32, logp f32)"""
    lib = L.load()
    V = x.shape[1]
    buf = torch.full((R_, ldl), float(pad), dtype=torch.float32)
    buf[:, :V] = torch.as_tensor(x[:R_])
    buf = buf.cuda()
    ids = torch.full((R_,), -7, dtype=torch.int64, device="cuda")
    kept = torch.full((R_,), -7, dtype=torch.int32, device="cuda")
    logp = torch.full((R_,), 7.0, device="cuda")
    wsb = lib.sat_sample_filtered_ws_bytes(R_, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    L.check(lib.sat_sample_filtered(buf.data_ptr(), ldl, R_, V, tau, k, p, seed, t, rank, ids.data_ptr(), 1,
                                    logp.data_ptr() if want_logp else None, kept.data_ptr() if want_kept else None, ws.data_ptr(), wsb,
                                    L.stream()), "sat_sample_filtered")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), kept.cpu().numpy(), logp.cpu().numpy()


def reference(row, tau, k, p, seed, t, rank, r):
    """(n, clearance, token, margin, logp, order) of one row"""
    order, n, clr = R.kept_prefix(row, tau, k, p)
    tok, margin = R.draw(row, tau, order[:n], seed, rank, r, t)
    return n, clr, tok, margin, R.logp(row, tau, order[:n], tok), order


def judge(row, tau, ref, seed, t, rank, r, got_id, got_kept, got_logp):
    """one device result against its reference under the two excuses; returns the logp error in units of the tolerance"""
    n, clr, tok, margin, lp, order = ref
    assert 0 <= got_id < len(row)
    if got_kept != n:
        assert clr < BAND and abs(int(got_kept) - n) == 1 and got_kept >= 1, (got_kept, n, clr)
        n = int(got_kept)                                     # the boundary token went the other way: replay the draw on that set
        tok, margin = R.draw(row, tau, order[:n], seed, rank, r, t)
    if got_id != tok:
        assert margin < CLOSE and got_id in order[:n], (got_id, tok, margin)
    lp = R.logp(row, tau, order[:n], int(got_id))
    err = abs(float(got_logp) - lp) / max(1.0, abs(lp))
    assert err <= LOGP_TOL, (float(got_logp), lp)
    return err / LOGP_TOL


# ---- 1: the sweep ------------------------------------------------------------------------------------------------------------------
VS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 12288, 12289]
TAUS, PS, RS = [0.5, 1.0, 1.7], [1.0, 0.9, 0.35], [1, 3, 65]
CHECKED = {1: [0], 3: [0, 2], 65: [0, 2, 64]}               # the rows compared with the reference, by R
GEN_SEED, SEED, T, RANK = 2024, 0x1234567890ABCDEF, 3, 1


def ks_of(V):
    return [0, 1, 5, 64, V, V + 1]


def ldls_of(V):
    return [V, pad4(V), pad4(V) + 4]


@functools.lru_cache(maxsize=None)
def sweep_rows(V):
    return np.random.default_rng(GEN_SEED + V).normal(0.0, 2.5, (65, V)).astype(np.float32)


def sweep_cases():
    """(V, ldl, R, tau, k, p): every (V, tau, k, p); the nine (ldl, R) pairs of a V taken in turn, so that each pair meets six
    settings"""
    out = []
    for V in VS:
        pairs = [(ldl, R_) for ldl in ldls_of(V) for R_ in RS]
        i = 0
        for tau in TAUS:
            for k in ks_of(V):
                for p in PS:
                    ldl, R_ = pairs[i % 9]
                    out.append((V, ldl, R_, tau, k, p))
                    i += 1
    return out


def test_sweep_against_the_reference():
    cases = sweep_cases()
    assert len(cases) == 810 and {c[:3] for c in cases} == {(V, ldl, R_) for V in VS for ldl in ldls_of(V) for R_ in RS}
    refs = {}
    for (V, ldl, R_, tau, k, p) in cases:
        for r in CHECKED[R_]:
            key = (V, r, tau, k, p)
            if key not in refs:
                refs[key] = reference(sweep_rows(V)[r], tau, k, p, SEED, T, RANK, r)
    total = sum(len(CHECKED[c[2]]) for c in cases)
    band = sum(refs[(c[0], r, c[3], c[4], c[5])][1] < BAND for c in cases for r in CHECKED[c[2]])
    close = sum(refs[(c[0], r, c[3], c[4], c[5])][3] < CLOSE for c in cases for r in CHECKED[c[2]])
    print("sweep: %d launches, %d rows checked; reference alone: %d in the rounding band, %d close draws" % (len(cases), total, band, close))
    assert 100 * band <= total and 100 * close <= total       # the excuses cover at most 1 % each -- before any device result
    worst = 0.0
    for (V, ldl, R_, tau, k, p) in cases:
        x = sweep_rows(V)
        ids, kept, logp = device(x, ldl, R_, tau, k, p, SEED, T, RANK)
        for r in CHECKED[R_]:
            worst = max(worst, judge(x[r], tau, refs[(V, r, tau, k, p)], SEED, T, RANK, r, ids[r], kept[r], logp[r]))
    print("largest logp error: %.3f of the tolerance 2^-22 max(1, |logp|)" % worst)


# ---- 2: planted rows ---------------------------------------------------------------------------------------------------------------
def exact(x, ldl, tau, k, p, seed=SEED, t=T, rank=RANK, pad=PAD, seeds=4):
    """device == reference on every row, no excuse taken (the planted rows are built to need none), over a few seeds; returns the
    results of the last seed and the references"""
    x = np.asarray(x, dtype=np.float32)
    for s in range(seeds):
        ids, kept, logp = device(x, ldl, x.shape[0], tau, k, p, seed + s, t, rank, pad=pad)
        refs = [reference(x[r], tau, k, p, seed + s, t, rank, r) for r in range(x.shape[0])]
        for r, ref in enumerate(refs):
            assert ref[1] >= BAND
            assert kept[r] == ref[0], (r, kept[r], ref[0])
            if ref[3] >= CLOSE:
                assert ids[r] == ref[2], (r, ids[r], ref[2])
            assert ids[r] in ref[5][:ref[0]]
            lp = R.logp(x[r], tau, ref[5][:ref[0]], int(ids[r]))
            assert abs(float(logp[r]) - lp) <= LOGP_TOL * max(1.0, abs(lp))
    return ids, kept, logp, refs


@pytest.mark.parametrize("V", [37, 64, 1025])
def test_all_equal_row(V):
    x = np.full((2, V), -1.25, dtype=np.float32)
    for ldl in (V, pad4(V) + 4):
        for k in (0, 1, 5, V, V + 3):
            nk = V if k == 0 else min(k, V)
            for p in (1.0, 0.35):
                ids, kept, _, _ = exact(x, ldl, 1.7, k, p, seeds=3)
                pz = float(np.float32(p)) * nk
                n = nk if p == 1.0 else int(np.ceil(pz))
                assert abs(pz - round(pz)) > 1e-3 or p == 1.0   # the count cut clears the band
                assert (kept == n).all() and (ids < n).all()      # the lowest indexes stay


def test_tie_group_straddles_the_top_k_cut():
    rng = np.random.default_rng(1)
    V = 1030
    x = rng.normal(-4.0, 1.0, (3, V)).astype(np.float32).clip(max=-1.0)
    ties = [7, 130, 258, 600, 1029]                           # columns of different threads, chunks and the V % 4 tail
    x[:, ties] = 3.0
    x[:, 400] = 5.0
    for ldl in (V, pad4(V)):
        ids, kept, _, refs = exact(x, ldl, 1.0, 3, 1.0, seeds=6)
        assert (kept == 3).all() and set(refs[0][5][:3].tolist()) == {400, 7, 130}
        assert all(i in (400, 7, 130) for i in ids)
        ids, kept, _, _ = exact(x, ldl, 0.5, 5, 1.0, seeds=2)
        assert (kept == 5).all()


def test_tie_group_straddles_the_nucleus_cut():
    V = 517
    x = np.full((2, V), -np.inf, dtype=np.float32)
    ties = [3, 64, 255, 256, 516]
    x[:, ties] = np.float32(np.log(0.5))
    x[:, 100] = 0.0
    # w = 1, then five of 0.5: Z = 3.5; 0.6 Z = 2.1 needs the 1 and three ties (2.5 >= 2.1 > 2.0): clearance 0.1 / 3.5
    for ldl in (V, pad4(V), pad4(V) + 4):
        ids, kept, _, refs = exact(x, ldl, 1.0, 0, 0.6, seeds=6)
        assert (kept == 4).all() and refs[0][5][:4].tolist() == [100, 3, 64, 255] and refs[0][1] > 0.02
        assert all(i in (100, 3, 64, 255) for i in ids)
    # behind a top-k cut through the same group: four survivors, Z = 2.5, 0.9 Z = 2.25 needs all four
    ids, kept, _, _ = exact(x, pad4(V), 1.0, 4, 0.9, seeds=3)
    assert (kept == 4).all()
    ids, kept, _, _ = exact(x, pad4(V), 1.0, 4, 0.7, seeds=3)  # 1.75: the 1 and two ties
    assert (kept == 3).all() and all(i in (100, 3, 64) for i in ids)


def test_signed_zeros_tie():
    V = 261
    x = np.full((2, V), -2.0, dtype=np.float32)
    zeros = [2, 9, 70, 131, 260]
    x[:, zeros] = [-0.0, 0.0, -0.0, 0.0, -0.0]
    x[1, zeros] = [0.0, -0.0, 0.0, -0.0, 0.0]
    for ldl in (V, pad4(V)):
        ids, kept, logp, refs = exact(x, ldl, 1.0, 3, 1.0, seeds=6)
        assert (kept == 3).all() and refs[0][5][:3].tolist() == [2, 9, 70] and refs[1][5][:3].tolist() == [2, 9, 70]
        assert all(i in (2, 9, 70) for i in ids)
        np.testing.assert_allclose(logp, np.log(1.0 / 3.0), rtol=1e-6)
        ids, kept, _, _ = exact(x, ldl, 1.0, 1, 1.0, seeds=2)
        assert (ids == 2).all()


def test_minus_inf_columns_are_no_candidates():
    V = 70
    x = np.full((2, V), -np.inf, dtype=np.float32)
    x[:, [1, 33, 66, 68, 69]] = [0.5, 1.5, -2.0, 1.5, 0.0]
    for ldl in (V, pad4(V)):
        ids, kept, _, _ = exact(x, ldl, 1.0, 64, 1.0, seeds=4)   # fewer finite columns than top_k
        assert (kept == 5).all() and all(i in (1, 33, 66, 68, 69) for i in ids)
        ids, kept, _, _ = exact(x, ldl, 1.0, 0, 1.0, seeds=2)
        assert (kept == 5).all()
        ids, kept, _, _ = exact(x, ldl, 1.0, 2, 1.0, seeds=4)
        assert (kept == 2).all() and all(i in (33, 68) for i in ids)


@pytest.mark.parametrize("V,col", [(1025, 1024), (1024, 1023), (1026, 1025), (5, 4), (4, 3), (259, 255), (12289, 12288), (12288, 12287)])
def test_maximum_in_edge_columns(V, col):
    """the last column (the V % 4 tail or the last 16-byte chunk), next to the pad, and a column with v % 4 == 3"""
    x = np.random.default_rng(V).normal(0, 1, (2, V)).astype(np.float32)
    x[:, col] = 9.0
    for ldl in ldls_of(V):
        ids, kept, logp = device(x, ldl, 2, 0.5, 1, 1.0, SEED, T, RANK)
        assert (ids == col).all() and (kept == 1).all() and (logp == 0).all()
        exact(x, ldl, 1.0, 5, 0.9, seeds=1)


@pytest.mark.parametrize("pad", [np.inf, np.nan])
def test_poisoned_pad_columns_are_not_read_as_candidates(pad):
    for V in (5, 63, 1023, 4099):
        x = sweep_rows(V)[:3]
        base = device(x, V, 3, 1.0, 0, 0.9, SEED, T, RANK)
        for ldl in (pad4(V), pad4(V) + 4):
            got = device(x, ldl, 3, 1.0, 0, 0.9, SEED, T, RANK, pad=pad)
            for a, b in zip(base, got):
                assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)
        exact(x, pad4(V) + 4, 1.0, 5, 1.0, pad=pad, seeds=1)


# ---- 3: top_k = 1 ------------------------------------------------------------------------------------------------------------------
def test_top_k_1_is_the_first_maximum_for_every_seed():
    V = 1025
    x = sweep_rows(V)[:5].copy()
    x[1, [900, 17, 333]] = 20.0                               # a repeated maximum: the first column wins
    x[2, [1024, 1023]] = 20.0
    want = np.array([int(np.argmax(row)) for row in x])
    assert want[1] == 17 and want[2] == 1023
    for s in range(16):
        for ldl in (V, pad4(V)):
            ids, kept, logp = device(x, ldl, 5, [0.5, 1.0, 1.7][s % 3], 1, [1.0, 0.35][s % 2], 1000 + s, s, s % 3)
            assert np.array_equal(ids, want) and (kept == 1).all() and (logp == 0).all()


# ---- 4: determinism ----------------------------------------------------------------------------------------------------------------
def test_results_depend_on_the_row_and_its_position_only():
    V = 4099
    y = sweep_rows(V)[7]
    outs = []
    for (R_, ldl) in ((5, V), (5, pad4(V)), (65, pad4(V) + 4), (65, V)):
        x = sweep_rows(V)[:R_].copy()
        x[4] = y                                              # the same content at row 4 of different batches and strides
        x[0] = y                                              # ... and at row 0: another counter, another draw
        for (tau, k, p) in ((1.0, 0, 1.0), (0.7, 50, 0.9)):
            a = device(x, ldl, R_, tau, k, p, SEED, T, RANK)
            b = device(x, ldl, R_, tau, k, p, SEED, T, RANK)
            for u, v in zip(a, b):                            # two identical calls: equal bits
                assert np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u, v.view(np.int32) if v.dtype == np.float32 else v)
            for r in (0, 4):
                ref = reference(y, tau, k, p, SEED, T, RANK, r)
                assert ref[1] >= BAND and ref[3] >= CLOSE
                assert a[0][r] == ref[2] and a[1][r] == ref[0]
            outs.append(((tau, k, p), a[0][4], a[1][4], a[2][4].view(np.int32), a[0][0]))
    for o in outs:
        first = next(q for q in outs if q[0] == o[0])
        assert o[1:] == first[1:]
    # without the optional outputs: the same tokens
    x = sweep_rows(V)[:5]
    a = device(x, pad4(V), 5, 0.7, 50, 0.9, SEED, T, RANK)
    b = device(x, pad4(V), 5, 0.7, 50, 0.9, SEED, T, RANK, want_logp=False, want_kept=False)
    assert np.array_equal(a[0], b[0]) and (b[1] == -7).all() and (b[2] == 7.0).all()


def test_unfiltered_draw_is_the_one_of_sat_vocab_sample():
    """(temperature, top_k, top_p) = (1, 0, 1): s(r, t) of the existing entry point on the same logits"""
    lib = L.load()
    g = torch.Generator().manual_seed(3)
    B, H, V = 5, 64, 203
    h = torch.randn(B, H, generator=g).cuda()
    w = (torch.randn(V, H, generator=g) * 0.3).cuda()
    b = torch.randn(V, generator=g).cuda()
    ldl = pad4(V)
    logits = torch.zeros(B, ldl, device="cuda")
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    wsb = lib.sat_ss_decoder_fwd_ws_bytes(B, V)
    ws = torch.empty(wsb // 4 + 1, device="cuda")
    for t in range(4):
        L.check(lib.sat_vocab_sample(h.data_ptr(), w.data_ptr(), b.data_ptr(), B, H, V, logits.data_ptr(), ldl, 1.0, SEED, t, RANK, None, 0,
                                     ids.data_ptr(), 1, None, 0, None, ws.data_ptr(), wsb, L.stream()), "sat_vocab_sample")
        torch.cuda.synchronize()
        got = device(logits.cpu().numpy()[:, :V], ldl, B, 1.0, 0, 1.0, SEED, t, RANK)
        assert np.array_equal(got[0], ids.cpu().numpy()) and (got[1] == V).all()


# ---- 5: DecoderRNN.sample_stochastic -----------------------------------------------------------------------------------------------
E5, H5, V5 = 32, 64, 203


def replay(logits, ids, logp, kept, tau, k, p, seed, rank):
    """every step's token, kept and logp from the returned logits [steps, R, V] through the reference, under the sweep's excuses"""
    steps, R_, V = logits.shape
    n_band = n_close = 0
    for t in range(steps):
        for r in range(R_):
            ref = reference(logits[t, r], tau, k, p, seed, t, rank, r)
            n_band += ref[1] < BAND
            n_close += ref[3] < CLOSE
            judge(logits[t, r], tau, ref, seed, t, rank, r, ids[r, t], kept[r, t], logp[r, t])
    assert 100 * n_band <= steps * R_ + 99 and 100 * n_close <= steps * R_ + 99
    return n_band, n_close


def step_by_step(dec, features, ids, states=None, steps=20, pick=None):
    """`steps` steps, one entry point at a time: (logits [steps, R, V], h, c) of `sat_lstm_step` / `sat_vocab_logits_fwd`.  pick
    None: fed the ids given.  pick "argmax" (`sat_vocab_argmax`; no logits) or dict(tau, k, p, seed, rank) (`sat_sample_filtered`
    with t = the step): the tokens are picked here, written to `ids` and fed through `sat_embed_rows`."""
    lib, st = L.load(), L.stream()
    R_, nl = features.shape[0], dec.num_layers
    h = torch.zeros(nl, R_, H5, device="cuda") if states is None else states[0].clone()
    c = torch.zeros(nl, R_, H5, device="cuda") if states is None else states[1].clone()
    ldl = pad4(V5)
    out = torch.zeros(steps, R_, ldl, device="cuda")
    lin_w, lin_b = dec.linear.weight.data_ptr(), dec.linear.bias.data_ptr()
    wsb = max(lib.sat_vocab_argmax_ws_bytes(R_, V5), lib.sat_sample_filtered_ws_bytes(R_, V5))
    ws, ws_ptr = L.workspace256(wsb, "cuda")
    x = features.contiguous()
    for t in range(steps):
        inp = x
        for l in range(nl):
            w_ih, w_hh, b_ih, b_hh = dec.lstm.layer(l)
            h2 = torch.empty(R_, H5, device="cuda")
            L.check(lib.sat_lstm_step(inp.data_ptr(), h[l].data_ptr(), c[l].data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
                                      b_hh.data_ptr(), R_, inp.shape[1], H5, h2.data_ptr(), st), "sat_lstm_step")
            h[l].copy_(h2)
            inp = h2
        col = ids[:, t]
        if pick == "argmax":
            L.check(lib.sat_vocab_argmax(inp.data_ptr(), lin_w, lin_b, R_, H5, V5, col.data_ptr(), ids.stride(0), ws_ptr, wsb, st),
                    "sat_vocab_argmax")
        else:
            L.check(lib.sat_vocab_logits_fwd(inp.data_ptr(), lin_w, lin_b, R_, H5, V5, out[t].data_ptr(), ldl, st), "sat_vocab_logits_fwd")
        if pick is None:
            x = dec.embed.weight[col].contiguous()
            continue
        if pick != "argmax":
            L.check(lib.sat_sample_filtered(out[t].data_ptr(), ldl, R_, V5, pick["tau"], pick["k"], pick["p"], pick["seed"], t, pick["rank"],
                                            col.data_ptr(), ids.stride(0), None, None, ws_ptr, wsb, st), "sat_sample_filtered")
        x = torch.empty(R_, E5, device="cuda")
        L.check(lib.sat_embed_rows(dec.embed.weight.data_ptr(), col.data_ptr(), ids.stride(0), R_, E5, V5, x.data_ptr(), st), "sat_embed_rows")
    return out[:, :, :V5], h, c


@pytest.mark.parametrize("steps", [3, 4])
@pytest.mark.parametrize("layers", [1, 2])
def test_decode_calls_return_the_ids_and_the_state_of_their_single_steps(layers, steps):
    """`sat_greedy_decode` and `sat_sample_decode` called directly, from a non-zero (h, c): ids and the final h and c are, bit for
    bit, those of the same steps issued one entry point at a time.  An even step count ends with every layer's live h in the
    caller's tensor, an odd one in the scratch: only then does the copy-back run.  (What h_tmp holds afterwards is not checked.)"""
    lib, st, B = L.load(), L.stream(), 3
    torch.manual_seed(100 * layers + steps)
    dec = sat.DecoderRNN(E5, H5, V5, layers).cuda().eval()
    dec.linear.weight.data.uniform_(-0.6, 0.6)
    feats = torch.randn(B, E5).cuda()
    h0, c0 = torch.randn(layers, B, H5).cuda() * 0.5, torch.randn(layers, B, H5).cuda() * 0.5
    draw = dict(tau=0.8, k=20, p=0.9, seed=SEED, rank=RANK)
    for pick in ("argmax", draw):
        want_ids = torch.full((B, steps), -7, dtype=torch.int64, device="cuda")
        _, want_h, want_c = step_by_step(dec, feats, want_ids, (h0, c0), steps, pick)
        h, c, h_tmp, xe = h0.clone(), c0.clone(), torch.empty_like(h0), torch.empty(B, E5, device="cuda")
        ids = torch.full((B, steps), -7, dtype=torch.int64, device="cuda")
        common = (feats.data_ptr(), dec.embed.weight.data_ptr(), dec._lstm_ptrs(), layers, dec.linear.weight.data_ptr(),
                  dec.linear.bias.data_ptr(), B, E5, H5, V5, steps)
        state = (h.data_ptr(), c.data_ptr(), h_tmp.data_ptr(), xe.data_ptr(), ids.data_ptr(), ids.stride(0))
        if pick == "argmax":
            wsb = lib.sat_vocab_argmax_ws_bytes(B, V5)
            ws, ws_ptr = L.workspace256(wsb, "cuda")
            L.check(lib.sat_greedy_decode(*common, *state, ws_ptr, wsb, st), "sat_greedy_decode")
        else:
            wsb = lib.sat_sample_decode_ws_bytes(B, E5, H5, V5, layers)
            ws, ws_ptr = L.workspace256(wsb, "cuda")
            L.check(lib.sat_sample_decode(*common, draw["tau"], draw["k"], draw["p"], draw["seed"], draw["rank"], *state, None, None, None,
                                          0, ws_ptr, wsb, st), "sat_sample_decode")
        torch.cuda.synchronize()
        assert (want_ids >= 0).all() and (want_ids < V5).all()
        assert torch.equal(ids, want_ids), pick
        assert torch.equal(h, want_h) and torch.equal(c, want_c), pick
        assert not torch.equal(h, h0) and not torch.equal(c, c0)


def test_decoder_rows_per_image_are_plain_repetition():
    """num_samples = 2 is the num_samples = 1 decode of every feature row and state column repeated twice, under the same seed: the
    kernels see the same rows and the same counters (row b * S + s)."""
    torch.manual_seed(21)
    layers, B = 2, 3
    dec = sat.DecoderRNN(E5, H5, V5, layers).cuda().eval()
    dec.linear.weight.data.uniform_(-0.6, 0.6)
    feats = torch.randn(B, E5).cuda()
    h0, c0 = torch.randn(layers, B, H5).cuda() * 0.5, torch.randn(layers, B, H5).cuda() * 0.5
    ids = dec.sample_stochastic(feats, (h0, c0), num_samples=2, seed=31, top_k=20, top_p=0.9)
    flat = dec.sample_stochastic(feats.repeat_interleave(2, 0), (h0.repeat_interleave(2, 1), c0.repeat_interleave(2, 1)),
                                 num_samples=1, seed=31, top_k=20, top_p=0.9)
    assert ids.shape == (B, 2, 20) and flat.shape == (2 * B, 20)
    assert torch.equal(ids.view(2 * B, 20), flat)


@pytest.mark.parametrize("layers,B,S", [(1, 1, 1), (1, 5, 3), (2, 5, 1), (2, 1, 3)])
def test_decoder_sample_stochastic(layers, B, S):
    torch.manual_seed(10 * layers + B + S)
    dec = sat.DecoderRNN(E5, H5, V5, layers).cuda().eval()
    dec.linear.weight.data.uniform_(-0.6, 0.6)
    dec.ss_rank = 2
    feats = torch.randn(B, E5).cuda()
    tau, k, p = 0.7, 20, 0.9
    torch.manual_seed(77)
    ids, lp, logits = dec.sample_stochastic(feats, temperature=tau, top_k=k, top_p=p, num_samples=S, return_logprobs=True, return_logits=True)
    seed = dec.last_sample_seed
    torch.manual_seed(77)
    assert seed == sat.models.draw_ss_seed()
    shape = (B, S, 20) if S > 1 else (B, 20)
    assert ids.shape == shape and ids.dtype == torch.int64 and lp["logp"].shape == shape and lp["kept"].shape == shape
    assert lp["kept"].dtype == torch.int32 and logits.shape == (20, B * S, V5)
    R_ = B * S
    ids2 = ids.reshape(R_, 20)
    nb, nc = replay(logits.cpu().numpy(), ids2.cpu().numpy(), lp["logp"].reshape(R_, 20).cpu().numpy(),
                    lp["kept"].reshape(R_, 20).cpu().numpy(), tau, k, p, seed, 2)
    print("replayed %d draws: %d in the band, %d close" % (20 * R_, nb, nc))
    # the tokens fed are the tokens drawn: a step-by-step run on the ids returned reproduces every step's logits
    want, _, _ = step_by_step(dec, feats.repeat_interleave(S, 0), ids2)
    assert torch.equal(want, logits)
    # same seed, same ids (with or without the optional outputs); another seed differs somewhere
    again = dec.sample_stochastic(feats, temperature=tau, top_k=k, top_p=p, num_samples=S, seed=seed)
    assert torch.equal(again, ids) and dec.last_sample_seed == seed
    other = dec.sample_stochastic(feats, temperature=tau, top_k=k, top_p=p, num_samples=S, seed=seed + 1)
    assert other.shape == shape and not torch.equal(other, ids)
    if S > 1:                                                  # the samples of one image are different captions
        assert not torch.equal(ids[:, 0], ids[:, 1])
    # top_k = 1 takes every step's first maximum; no squeeze ([20] at batch 1 is `sample`'s shape, not this method's)
    one, lg = dec.sample_stochastic(feats, top_k=1, temperature=1.7, return_logits=True)
    assert one.shape == (B, 20) and torch.equal(one, lg.argmax(-1).t())


def test_decoder_sample_stochastic_honours_states():
    torch.manual_seed(5)
    layers, B = 2, 3
    dec = sat.DecoderRNN(E5, H5, V5, layers).cuda().train()    # train mode decodes too: no tapes either way
    feats = torch.randn(B, E5).cuda()
    h0, c0 = torch.randn(layers, B, H5).cuda() * 0.5, torch.randn(layers, B, H5).cuda() * 0.5
    ids, logits = dec.sample_stochastic(feats, (h0, c0), temperature=1.0, top_k=0, top_p=0.95, seed=9, return_logits=True)
    want, _, _ = step_by_step(dec, feats, ids, (h0, c0))
    assert torch.equal(want, logits)
    zero, _, _ = step_by_step(dec, feats, ids)
    assert not torch.equal(zero, logits)
    assert not logits.requires_grad and dec.last_sample_seed == 9


# ---- 6: ShowAttendTellModel.sample_stochastic_features -----------------------------------------------------------------------------
DIMS6 = dict(P=9, C=16, E=12, H=28, V=101)


def make_attend():
    d = DIMS6
    params = SA.params(OA, 0, d)
    model = sat.ShowAttendTellModel(d["H"], d["C"], d["V"], d["E"], None, feature_size=(d["P"], d["C"]), compute_dtype="f32",
                                    vgg_cfg=[8, "M", d["C"]])
    model.load_state_dict(params, strict=False)
    model.classifier.weight.data.mul_(4.0)                     # spread the logits: fewer near ties
    return model.cuda().eval()


def test_attend_sample_stochastic_features():
    d, B = DIMS6, 3
    model = make_attend()
    model.ss_rank = 1
    feats = SA.features(B, 1, d).cuda()
    # no state leaks: the other decodes before and after
    before = (model.sample_features(feats), model.sample_beam_features(feats, 3))
    model.train()
    torch.manual_seed(4)
    rb = model.rollout(feats, feats.mean(1), 6)
    model.eval()
    tau, k, p = 0.8, 30, 0.9
    ids, lp, logits, alphas = model.sample_stochastic_features(feats, temperature=tau, top_k=k, top_p=p, seed=123, return_logprobs=True,
                                                               return_logits=True, return_alphas=True)
    assert ids.shape == (B, 20) and logits.shape == (20, B, d["V"]) and alphas.shape == (B, 20, d["P"]) and model.last_sample_seed == 123
    np.testing.assert_allclose(alphas.sum(-1).cpu().numpy(), 1.0, rtol=0, atol=1e-5)
    nb, nc = replay(logits.cpu().numpy(), ids.cpu().numpy(), lp["logp"].cpu().numpy(), lp["kept"].cpu().numpy(), tau, k, p, 123, 1)
    print("replayed %d draws: %d in the band, %d close" % (20 * B, nb, nc))
    again = model.sample_stochastic_features(feats, temperature=tau, top_k=k, top_p=p, seed=123)
    assert torch.equal(again, ids)
    assert not torch.equal(model.sample_stochastic_features(feats, temperature=tau, top_k=k, top_p=p, seed=124), ids)
    many, am = model.sample_stochastic_features(feats, temperature=tau, top_k=k, top_p=p, seed=123, num_samples=2, return_alphas=True)
    assert many.shape == (B, 2, 20) and am.shape == (B, 2, 20, d["P"]) and not torch.equal(many[:, 0], many[:, 1])
    # top_k = 1 decodes what `sample` decodes wherever the top two logits of a step differ by more than 1e-4
    one, lg = model.sample_stochastic_features(feats, top_k=1, temperature=1.7, return_logits=True)
    top2 = lg.topk(2, dim=-1).values
    clear = ((top2[..., 0] - top2[..., 1]) > 1e-4).t().cumprod(1).bool().cpu()   # [B, 20]: up to a row's first near tie
    assert clear[:, 0].all() and torch.equal(one.cpu()[clear], before[0].cpu()[clear])
    after = (model.sample_features(feats), model.sample_beam_features(feats, 3))
    model.train()
    torch.manual_seed(4)
    ra = model.rollout(feats, feats.mean(1), 6)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert torch.equal(rb[0], ra[0]) and torch.equal(rb[1].detach(), ra[1].detach())


def test_attend_rows_per_image_are_plain_repetition():
    """`sample_stochastic_features` at the smallest legal dims (tests/test_gpu_attend.py's: E 4, C 8, H 12, P 5, V 11; B 3) from a
    non-zero (h, c): num_samples = 2 is the num_samples = 1 decode of the features and states repeated twice per image under the
    same seed, ids and attention maps bit for bit; the caller's h and c are not written."""
    torch.manual_seed(179)
    B, P, C, E, H, V = 3, 5, 8, 4, 12, 11
    model = sat.ShowAttendTellModel(H, C, V, E, None, feature_size=(P, C), compute_dtype="f32", vgg_cfg=[C]).cuda().eval()
    feats = torch.randn(B, P, C).cuda()
    h, c = torch.randn(B, H).cuda(), torch.randn(B, H).cuda()
    h_was, c_was = h.clone(), c.clone()
    ids, alphas = model.sample_stochastic_features(feats, (h, c), num_samples=2, seed=31, top_k=20, top_p=0.9, return_alphas=True)
    flat, flat_alphas = model.sample_stochastic_features(feats.repeat_interleave(2, 0), (h.repeat_interleave(2, 0), c.repeat_interleave(2, 0)),
                                                         num_samples=1, seed=31, top_k=20, top_p=0.9, return_alphas=True)
    assert ids.shape == (B, 2, 20) and alphas.shape == (B, 2, 20, P) and flat.shape == (2 * B, 20) and flat_alphas.shape == (2 * B, 20, P)
    assert torch.equal(ids.view(2 * B, 20), flat) and torch.equal(alphas.view(2 * B, 20, P), flat_alphas)
    assert torch.equal(h, h_was) and torch.equal(c, c_was)


# ---- 7: argument errors of the two C entry points ----------------------------------------------------------------------------------
def test_c_argument_errors_come_back_without_a_launch():
    lib = L.load()
    B, E, H, V, steps = 3, E5, H5, V5, 4
    ldl = pad4(V)
    logits = torch.randn(B, ldl, device="cuda")
    ids = torch.full((B, steps), -7, dtype=torch.int64, device="cuda")
    wsb = lib.sat_sample_filtered_ws_bytes(B, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

    def filt(**kw):
        a = dict(logits=logits.data_ptr(), ldl=ldl, R=B, V=V, tau=1.0, k=0, p=1.0, t=0, rank=0, ids=ids.data_ptr(), ws=ws.data_ptr(), wsb=wsb)
        a.update(kw)
        return lib.sat_sample_filtered(a["logits"], a["ldl"], a["R"], a["V"], a["tau"], a["k"], a["p"], 5, a["t"], a["rank"], a["ids"],
                                       steps, None, None, a["ws"], a["wsb"], L.stream())

    bad = [dict(logits=None), dict(ids=None), dict(ws=None), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")),
           dict(p=0.0), dict(p=1.5), dict(k=-1), dict(ldl=V - 1), dict(R=0), dict(V=0), dict(t=-1), dict(rank=-1)]
    for kw in bad:
        assert filt(**kw) == 1001, kw
    assert filt(wsb=wsb - 1) == 1002
    assert filt(V=40000, ldl=40000) == 1003

    dec = sat.DecoderRNN(E, H, V, 1).cuda()
    feats = torch.randn(B, E, device="cuda")
    h, c, ht = torch.zeros(1, B, H, device="cuda"), torch.zeros(1, B, H, device="cuda"), torch.zeros(1, B, H, device="cuda")
    xe = torch.zeros(B, E, device="cuda")
    dwsb = lib.sat_sample_decode_ws_bytes(B, E, H, V, 1)
    dws = torch.empty(dwsb + 256, dtype=torch.uint8, device="cuda")
    dptr = dws.data_ptr() + (-dws.data_ptr()) % 256

    def decode(**kw):
        a = dict(features=feats.data_ptr(), ids=ids.data_ptr(), ws=dptr, wsb=dwsb, tau=1.0, k=0, p=1.0, rank=0, steps=steps, ldl=ldl,
                 logits_out=None, h=h.data_ptr())
        a.update(kw)
        return lib.sat_sample_decode(a["features"], dec.embed.weight.data_ptr(), dec._lstm_ptrs(), 1, dec.linear.weight.data_ptr(),
                                     dec.linear.bias.data_ptr(), B, E, H, V, a["steps"], a["tau"], a["k"], a["p"], 5, a["rank"], a["h"],
                                     c.data_ptr(), ht.data_ptr(), xe.data_ptr(), a["ids"], steps, None, None, a["logits_out"], a["ldl"],
                                     a["ws"], a["wsb"], L.stream())

    for kw in bad[:10] + [dict(steps=0), dict(rank=-1), dict(h=None), dict(logits_out=logits.data_ptr(), ldl=V - 1)]:
        kw = {("features" if k_ == "logits" else k_): v for k_, v in kw.items()}
        assert decode(**kw) == 1001, kw
    assert decode(wsb=dwsb - 1) == 1002
    torch.cuda.synchronize()
    assert (ids == -7).all() and not h.any() and not xe.any()  # nothing ran
    assert decode() == 0                                       # and the same call with good arguments does
    torch.cuda.synchronize()
    assert (ids >= 0).all() and (ids < V).all()
