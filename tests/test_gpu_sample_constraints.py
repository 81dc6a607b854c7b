"""GPU (MI355X): constrained sampling -- `sat_sample_filtered_ex` / `sat_sample_decode_ex` and the constraint keywords of the
`sample_stochastic` methods (banned ids, min_length, n-gram blocking, block_repeat, repetition penalty).

Two oracles.  (a) the UNCHANGED `sat_sample_filtered` on rows transformed on the host (tests/sample_constraints_reference.py): ids,
kept and logp agree bit for bit, for bans and penalties alike -- the contract is "sat_sample_filtered applied to x'".  (b) the numpy
reference, under the two excuses of tests/test_gpu_sample.py (a nucleus decision closer than 1e-6 to top_p * Z; a draw whose two
best perturbed scores are closer than 1e-4), each capped at 1 % of the sweep's checked rows ON THE REFERENCE, before any device
result (tests/test_sample_constraints_host.py asserts the same caps without a GPU)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import sample_constraints_reference as SC
import sample_reference as R

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

ARG, WORKSPACE, UNSUPPORTED = 1001, 1002, 1003
LOGP_TOL = 2.0 ** -22                 # one rounding to f32 (2^-24 relative), fourfold: tests/test_gpu_sample.py's
PAD = 1e30                            # what pad columns hold: a candidate there would win every draw
SEED, RANK = SC.SEED, SC.RANK
pad4 = SC.pad4


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


def c_struct(rules):
    """(sat_sample_constraints, the device tensor it points to) of a reference `Rules`; None stays None"""
    if rules is None:
        return None, None
    sup = torch.tensor(list(rules.suppress_ids), dtype=torch.int64).cuda() if rules.suppress_ids else None
    return L.SatSampleConstraints(sup.data_ptr() if sup is not None else None, len(rules.suppress_ids), rules.min_length,
                                  rules.no_repeat_ngram, int(rules.block_repeat), rules.repetition_penalty,
                                  -1 if rules.end_id is None else rules.end_id), sup


def logits_buffer(x, ldl, R_, pad=PAD):
    buf = torch.full((R_, ldl), float(pad), dtype=torch.float32)
    buf[:, :x.shape[1]] = torch.as_tensor(x[:R_])
    return buf.cuda()


def outputs(R_):
    return (torch.full((R_,), -7, dtype=torch.int64, device="cuda"), torch.full((R_,), -7, dtype=torch.int32, device="cuda"),
            torch.full((R_,), 7.0, device="cuda"))


def read(ids, kept, logp):
    torch.cuda.synchronize()
    return ids.cpu().numpy(), kept.cpu().numpy(), logp.cpu().numpy()


def plain(x, ldl, R_, tau, k, p, seed, t, rank, pad=PAD):
    """the unchanged sat_sample_filtered on the first R_ rows of x [*, V]: (ids, kept, logp)"""
    lib, V = L.load(), x.shape[1]
    buf, (ids, kept, logp) = logits_buffer(x, ldl, R_, pad), outputs(R_)
    wsb = lib.sat_sample_filtered_ws_bytes(R_, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    L.check(lib.sat_sample_filtered(buf.data_ptr(), ldl, R_, V, tau, k, p, seed, t, rank, ids.data_ptr(), 1, logp.data_ptr(), kept.data_ptr(),
                                    ws.data_ptr(), wsb, L.stream()), "sat_sample_filtered")
    return read(ids, kept, logp)


def constrained(x, ldl, R_, tau, k, p, seed, t, rank, rules, prefixes, pad=PAD):
    """sat_sample_filtered_ex on the first R_ rows of x under `rules` (a reference Rules, or None for c == NULL); prefixes i64
    [>= R_, stride] or None for a NULL prefix: (ids, kept, logp).  The logits must come back untouched."""
    lib, V = L.load(), x.shape[1]
    buf, (ids, kept, logp) = logits_buffer(x, ldl, R_, pad), outputs(R_)
    was = buf.clone()
    cs, keep = c_struct(rules)
    pre = torch.as_tensor(np.ascontiguousarray(prefixes[:R_])).cuda() if prefixes is not None else None
    wsb = lib.sat_sample_filtered_ws_bytes(R_, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    L.check(lib.sat_sample_filtered_ex(buf.data_ptr(), ldl, R_, V, tau, k, p, seed, t, rank, ids.data_ptr(), 1, logp.data_ptr(),
                                       kept.data_ptr(), C.byref(cs) if cs is not None else None, pre.data_ptr() if pre is not None else None,
                                       pre.stride(0) if pre is not None else 0, ws.data_ptr(), wsb, L.stream()), "sat_sample_filtered_ex")
    out = read(ids, kept, logp)
    assert torch.equal(buf.view(torch.int32), was.view(torch.int32))            # the kernel never writes the row
    del keep
    return out


def judge(xp, tau, ref, seed, t, rank, r, got_id, got_kept, got_logp):
    """one device result against the reference of its TRANSFORMED row under the two excuses; the logp error in units of the tolerance"""
    n, clr, tok, margin, lp, order = ref
    if len(order) == 0:                                                         # no candidate: id 0, kept 0, logp -inf
        assert got_id == 0 and got_kept == 0 and got_logp == -np.inf, (got_id, got_kept, got_logp)
        return 0.0
    assert 0 <= got_id < len(xp)
    if got_kept != n:
        assert clr < SC.BAND and abs(int(got_kept) - n) == 1 and got_kept >= 1, (got_kept, n, clr)
        n = int(got_kept)
        tok, margin = R.draw(xp, tau, order[:n], seed, rank, r, t)
    if got_id != tok:
        assert margin < SC.CLOSE and got_id in order[:n], (got_id, tok, margin)
    lp = R.logp(xp, tau, order[:n], int(got_id))
    err = abs(float(got_logp) - lp) / max(1.0, abs(lp))
    assert err <= LOGP_TOL, (float(got_logp), lp)
    return err / LOGP_TOL


# ---- 1: the single-step sweep ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SC.VS)
def test_sweep(V):
    total, band, close, empty = SC.sweep_excuses()                              # the whole sweep's, computed once per process
    assert 100 * band <= total and 100 * close <= total and empty > 0           # the caps -- before any device result
    refs = SC.sweep_references()
    x, prefixes = SC.sweep_rows(V), SC.sweep_prefixes(V)
    worst, changed = 0.0, 0
    for (V_, ldl, R_, t, name, rules, (tau, k, p)) in SC.sweep_cases():
        if V_ != V:
            continue
        xp = SC.sweep_transformed(V, t, name, rules)
        got = constrained(x, ldl, R_, tau, k, p, SEED, t, RANK, rules, prefixes if t > 0 else None)
        want = plain(xp, ldl, R_, tau, k, p, SEED, t, RANK)
        assert same_bits(got, want), (V, ldl, R_, t, name, tau, k, p, got, want)                     # oracle (a), every row
        changed += int(not np.array_equal(bits(xp[:R_]), bits(x[:R_])))
        for r in SC.CHECKED[R_]:                                                                     # oracle (b)
            worst = max(worst, judge(xp[r], tau, refs[(V, t, name, (tau, k, p), r)], SEED, t, RANK, r, got[0][r], got[1][r], got[2][r]))
    assert changed >= 100                                                       # most cases do constrain something
    print("V = %d: largest logp error %.3f of the tolerance; %d of 252 cases transform a row" % (V, worst, changed))


# ---- 2: planted edges ------------------------------------------------------------------------------------------------------------
def agree(x, prefixes, t, rules, ldl, tau=1.0, k=0, p=1.0, seed=SEED, rank=RANK, pad=PAD):
    """device under rules == unchanged kernel on the host-transformed rows (bits) == numpy reference, no excuse taken"""
    x = np.asarray(x, dtype=np.float32)
    R_ = x.shape[0]
    xp = SC.transform_rows(x, None if prefixes is None else np.asarray(prefixes)[:, :t], rules)
    got = constrained(x, ldl, R_, tau, k, p, seed, t, rank, rules, prefixes, pad=pad)
    assert same_bits(got, plain(xp, ldl, R_, tau, k, p, seed, t, rank, pad=pad))
    for r in range(R_):
        n, clr, tok, margin, lp, order = SC.reference(xp[r], tau, k, p, seed, t, rank, r)
        assert clr >= SC.BAND
        assert got[1][r] == n, (r, got[1][r], n)
        if len(order) == 0:
            assert got[0][r] == 0 and got[2][r] == -np.inf
            continue
        if margin >= SC.CLOSE:
            assert got[0][r] == tok, (r, got[0][r], tok)
        assert got[0][r] in order[:n]
        lp = R.logp(xp[r], tau, order[:n], int(got[0][r]))
        assert abs(float(got[2][r]) - lp) <= LOGP_TOL * max(1.0, abs(lp))
    return got, xp


def prefix_buffer(rows, width=64, fill=0):
    out = np.full((len(rows), width), fill, dtype=np.int64)
    for r, row in enumerate(rows):
        out[r, :len(row)] = row
    return out


@pytest.mark.parametrize("V", [4, 5, 1023, 1025])
def test_banned_column_is_the_row_maximum_and_sits_on_every_edge(V):
    """the maximum is banned (the arg-max of x' is the runner-up); bans at bitmap word edges (31, 32, 63, 64), at the ends of the last
    whole 16-byte chunk and in the V % 4 tail; every way a ban can come about"""
    rng = np.random.default_rng(V)
    x = rng.normal(0, 1, (3, V)).astype(np.float32)
    edges = sorted(set(c for c in (0, 31, 32, 63, 64, (V >> 2) * 4 - 4, (V >> 2) * 4 - 1, (V >> 2) * 4, V - 1) if 0 <= c < V))
    for ldl in SC.ldls_of(V):
        for col in edges:
            x2 = x.copy()
            x2[:, col] = 9.0                                                    # the banned column would win
            for rules, pre, t in ((SC.Rules(suppress_ids=(col,)), None, 0),
                                  (SC.Rules(min_length=3, end_id=col), prefix_buffer([[0, 0]] * 3), 2),
                                  (SC.Rules(block_repeat=True), prefix_buffer([[0, col]] * 3), 2),
                                  (SC.Rules(no_repeat_ngram=1), prefix_buffer([[col, 0, 0]] * 3), 3),
                                  (SC.Rules(no_repeat_ngram=2), prefix_buffer([[1, col, 2, 1]] * 3), 4)):
                (ids, kept, logp), xp = agree(x2, pre, t, rules, ldl, k=1)
                runner_up = [int(np.argmax(row)) for row in xp]                 # the first maximum of x'
                assert np.isneginf(xp[:, col]).all() and col not in runner_up
                assert ids.tolist() == runner_up and (kept == 1).all() and (logp == 0).all(), (V, ldl, col, ids, runner_up)
        (ids, kept, _), xp = agree(x, None, 0, SC.Rules(suppress_ids=tuple(edges)), ldl, tau=0.7, k=0, p=0.9)   # all edges at once
        assert not set(ids.tolist()) & set(edges) and (kept <= V - len(edges)).all() and (kept >= 1).all()


@pytest.mark.parametrize("V", [4, 5, 1023, 1025])
def test_every_column_banned(V):
    x = np.random.default_rng(V).normal(0, 1, (2, V)).astype(np.float32)
    pre = prefix_buffer([list(range(min(V, 63)))] * 2)
    for ldl in SC.ldls_of(V):
        if V <= 256:
            for (tau, k, p) in SC.SETTINGS:
                ids, kept, logp = constrained(x, ldl, 2, tau, k, p, SEED, 0, RANK, SC.Rules(suppress_ids=tuple(range(V))), None)
                assert (ids == 0).all() and (kept == 0).all() and (logp == -np.inf).all()
        if V <= 63:                                                             # ... by the prefix: no token twice
            got, xp = agree(x, pre, V, SC.Rules(no_repeat_ngram=1), ldl, tau=0.7, k=5, p=0.9)
            assert np.isneginf(xp).all() and (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == -np.inf).all()
        # everything but 256 suppressed ids is -inf in the row itself: the 256 bans leave nothing
        x3 = np.full((2, V), -np.inf, dtype=np.float32)
        cols = np.random.default_rng(V + 1).permutation(V)[:256]
        x3[:, cols] = x[:, cols]
        ids, kept, logp = constrained(x3, ldl, 2, 1.0, 0, 0.9, SEED, 0, RANK, SC.Rules(suppress_ids=tuple(int(c) for c in cols)), None)
        assert (ids == 0).all() and (kept == 0).all() and (logp == -np.inf).all()
        # and with one of them left: that one
        left = int(cols[-1])
        ids, kept, logp = constrained(x3, ldl, 2, 1.0, 0, 0.9, SEED, 0, RANK, SC.Rules(suppress_ids=tuple(int(c) for c in cols[:-1])), None)
        assert (ids == left).all() and (kept == 1).all() and (logp == 0).all()


def test_prefix_tokens_outside_the_vocabulary_are_ignored():
    V = 261
    x = np.random.default_rng(3).normal(0, 2.5, (3, V)).astype(np.float32)
    rules = SC.Rules(block_repeat=True, no_repeat_ngram=2, repetition_penalty=1.3)
    clean = prefix_buffer([[5, 9, 5, 260], [7, 7, 7, 7], [1, 2, 3, 4]])
    for ldl in (V, pad4(V)):
        base, _ = agree(x, clean, 4, rules, ldl)
        dirty = clean.copy()
        dirty[:, 4:] = [[-1, V, 2 ** 40, -2 ** 40] * 15] * 3                      # behind the prefix: never read as tokens
        assert same_bits(constrained(x, ldl, 3, 1.0, 0, 1.0, SEED, 4, RANK, rules, dirty), base)
        # inside the prefix: no bit is set for them (and nothing is read or written out of bounds); the reference maps them to
        # "no token"
        inside = prefix_buffer([[5, -1, 5, V], [V, 7, -1, 7], [2 ** 40, 2, -2 ** 40, 2]])
        for t in (1, 2, 3, 4):
            agree(x, inside, t, rules, ldl)
            agree(x, inside, t, SC.Rules(no_repeat_ngram=1), ldl, k=5)
    # suppressed ids outside [0, V) likewise (the C entry point takes them; the Python validator refuses them earlier)
    lib = L.load()
    sup = torch.tensor([-1, V, 2 ** 40, 4], dtype=torch.int64).cuda()
    cs = L.SatSampleConstraints(sup.data_ptr(), 4, 0, 0, 0, 1.0, -1)
    buf, (ids, kept, logp) = logits_buffer(x, pad4(V), 3), outputs(3)
    ws = torch.empty(lib.sat_sample_filtered_ws_bytes(3, V), dtype=torch.uint8, device="cuda")
    L.check(lib.sat_sample_filtered_ex(buf.data_ptr(), pad4(V), 3, V, 1.0, 0, 1.0, SEED, 0, RANK, ids.data_ptr(), 1, logp.data_ptr(),
                                       kept.data_ptr(), C.byref(cs), None, 0, ws.data_ptr(), ws.numel(), L.stream()), "sat_sample_filtered_ex")
    assert same_bits(read(ids, kept, logp), plain(SC.transform_rows(x, None, SC.Rules(suppress_ids=(4,))), pad4(V), 3, 1.0, 0, 1.0, SEED, 0, RANK))


def test_step_0_takes_a_null_prefix_and_rules_that_do_nothing_are_the_plain_kernel():
    V = 1025
    x = SC.sweep_rows(V)[:5]
    everything = SC.Rules(suppress_ids=(0, 1, 3), min_length=5, end_id=2, no_repeat_ngram=3, block_repeat=True, repetition_penalty=1.3)
    for ldl in SC.ldls_of(V):
        agree(x, None, 0, everything, ldl, tau=0.7, k=50, p=0.9)                # t = 0: only the suppressed ids and end_id act
        base = plain(x, ldl, 5, 0.7, 50, 0.9, SEED, 3, RANK)
        off = SC.Rules()                                                        # every field off, and c == NULL
        assert same_bits(constrained(x, ldl, 5, 0.7, 50, 0.9, SEED, 3, RANK, off, None), base)
        assert same_bits(constrained(x, ldl, 5, 0.7, 50, 0.9, SEED, 3, RANK, None, None), base)
        assert same_bits(constrained(x, ldl, 5, 0.7, 50, 0.9, SEED, 3, RANK, off, SC.sweep_prefixes(V)), base)
        # rules that are on but change nothing at this step: n > t, min_length <= t, t = 0 for the prefix readers
        assert same_bits(constrained(x, ldl, 5, 0.7, 50, 0.9, SEED, 3, RANK, SC.Rules(no_repeat_ngram=4, min_length=3, end_id=2), None), base)
        base0 = plain(x, ldl, 5, 0.7, 50, 0.9, SEED, 0, RANK)
        assert same_bits(constrained(x, ldl, 5, 0.7, 50, 0.9, SEED, 0, RANK, SC.Rules(no_repeat_ngram=1, block_repeat=True,
                                                                                      repetition_penalty=1.5), None), base0)


def test_a_row_depends_on_its_own_prefix_only():
    V = 4099
    x = SC.sweep_rows(V)[:9]
    pre = SC.sweep_prefixes(V)[:9].copy()
    rules = SC.Rules(no_repeat_ngram=2, block_repeat=True, repetition_penalty=1.3)
    for ldl in (V, pad4(V)):
        a = constrained(x, ldl, 9, 1.0, 0, 0.9, SEED, 19, RANK, rules, pre)
        other = pre.copy()
        other[[0, 1, 2, 3, 5, 6, 7, 8]] = pre[[8, 7, 6, 5, 3, 2, 1, 0]]            # every row but row 4 gets another row's prefix
        b = constrained(x, ldl, 9, 1.0, 0, 0.9, SEED, 19, RANK, rules, other)
        assert all(bits(u)[4] == bits(v)[4] for u, v in zip(a, b))
        assert not same_bits(a, b)                                              # (the others did change)
        wide = np.full((9, 70), -5, dtype=np.int64)                             # another row stride, junk behind the prefix
        wide[:, :19] = pre[:, :19]
        assert same_bits(constrained(x, ldl, 9, 1.0, 0, 0.9, SEED, 19, RANK, rules, wide), a)


def test_top_k_1_takes_the_first_maximum_of_the_transformed_row():
    V = 1025
    x = SC.sweep_rows(V)[:4].copy()
    x[:, [17, 333, 900, 1024]] = 20.0                                           # a repeated maximum
    x[1, 17] = 26.0                                                             # penalised to 20 = a tie with 333: the lower column wins
    x[2, 17] = 25.0                                                             # penalised below 20: 333 is first
    pre = prefix_buffer([[5, 6], [17, 6], [17, 17], [17, 333]])
    want = [17, 17, 333, 900]                                                   # row 3: 17 and 333 both penalised
    th = 1.3
    assert np.float32(26.0) / np.float32(th) == np.float32(20.0) and np.float32(25.0) / np.float32(th) < 20.0
    for s in range(6):
        for ldl in (V, pad4(V)):
            (ids, kept, logp), xp = agree(x, pre, 2, SC.Rules(repetition_penalty=th), ldl, tau=[0.5, 1.0, 1.7][s % 3], k=1, seed=1000 + s)
            assert ids.tolist() == want == [int(np.argmax(row)) for row in xp] and (kept == 1).all() and (logp == 0).all()


def test_penalty_is_the_correctly_rounded_division_on_both_signs():
    """penalised columns spread over registers, chunks and the tail; theta values whose reciprocal is inexact"""
    V = 4099
    x = SC.sweep_rows(V)[:3].copy()
    x[:, 7] = 0.0
    x[:, 8] = -0.0
    cols = [0, 7, 8, 31, 32, 1023, 1024, 2047, 4095, 4096, 4098]
    pre = prefix_buffer([cols + cols[:5]] * 3)                                  # 16 tokens, five of them twice
    for theta in (1.3, 0.8, 3.0, 1.0000001, 7.77):
        for ldl in (V, pad4(V)):
            got, xp = agree(x, pre, 16, SC.Rules(repetition_penalty=theta), ldl, tau=0.9, k=0, p=1.0)
            assert (got[1] == V).all()
            th = np.float32(theta)
            assert all(xp[r, c] == (x[r, c] / th if x[r, c] > 0 else x[r, c] * th) for r in range(3) for c in cols)


# ---- 3: the decode loop ------------------------------------------------------------------------------------------------------------
E3 = H3 = 32
V3 = 67
LOOP_RULES = SC.Rules(suppress_ids=(0, 1, 3), min_length=5, end_id=2, no_repeat_ngram=2, block_repeat=True, repetition_penalty=1.3)


def make_decoder(layers, seed, V=V3):
    torch.manual_seed(seed)
    dec = sat.DecoderRNN(E3, H3, V, layers).cuda().eval()
    dec.linear.weight.data.uniform_(-0.9, 0.9)
    return dec


def chain(dec, feats, steps, draw, rules):
    """the loop one entry point at a time: sat_lstm_step per layer, sat_vocab_logits_fwd, sat_sample_filtered_ex with the ids so far
    as the prefix, sat_embed_rows.  -> ids [B, steps], logp, kept, logits [steps, B, V]"""
    lib, st = L.load(), L.stream()
    B, nl, V = feats.shape[0], dec.num_layers, dec.vocab_size
    h, c = torch.zeros(nl, B, H3, device="cuda"), torch.zeros(nl, B, H3, device="cuda")
    ldl = pad4(V)
    out = torch.zeros(steps, B, ldl, device="cuda")
    ids = torch.full((B, steps), -7, dtype=torch.int64, device="cuda")
    logp, kept = torch.full((B, steps), 7.0, device="cuda"), torch.full((B, steps), -7, dtype=torch.int32, device="cuda")
    lp1, kp1 = torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    wsb = lib.sat_sample_filtered_ws_bytes(B, V)
    ws, ws_ptr = L.workspace256(wsb, "cuda")
    cs, keep = c_struct(rules)
    x = feats.contiguous()
    for t in range(steps):
        inp = x
        for l in range(nl):
            w_ih, w_hh, b_ih, b_hh = dec.lstm.layer(l)
            h2 = torch.empty(B, H3, device="cuda")
            L.check(lib.sat_lstm_step(inp.data_ptr(), h[l].data_ptr(), c[l].data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
                                      b_hh.data_ptr(), B, inp.shape[1], H3, h2.data_ptr(), st), "sat_lstm_step")
            h[l].copy_(h2)
            inp = h2
        L.check(lib.sat_vocab_logits_fwd(inp.data_ptr(), dec.linear.weight.data_ptr(), dec.linear.bias.data_ptr(), B, H3, V, out[t].data_ptr(),
                                         ldl, st), "sat_vocab_logits_fwd")
        col = ids[:, t]
        L.check(lib.sat_sample_filtered_ex(out[t].data_ptr(), ldl, B, V, draw["tau"], draw["k"], draw["p"], draw["seed"], t, draw["rank"],
                                           col.data_ptr(), ids.stride(0), lp1.data_ptr(), kp1.data_ptr(),
                                           C.byref(cs) if cs is not None else None, ids.data_ptr(), ids.stride(0), ws_ptr, wsb, st),
                "sat_sample_filtered_ex")
        logp[:, t], kept[:, t] = lp1, kp1
        x = torch.empty(B, E3, device="cuda")
        L.check(lib.sat_embed_rows(dec.embed.weight.data_ptr(), col.data_ptr(), ids.stride(0), B, E3, V, x.data_ptr(), st), "sat_embed_rows")
    torch.cuda.synchronize()
    del keep
    return ids, logp, kept, out[:, :, :V]


def decode_call(dec, feats, steps, draw, rules, ex=True):
    """sat_sample_decode_ex (ex) or sat_sample_decode called directly -> ids, logp, kept"""
    lib = L.load()
    B, nl, V = feats.shape[0], dec.num_layers, dec.vocab_size
    h, c, ht = (torch.zeros(nl, B, H3, device="cuda") for _ in range(3))
    xe = torch.empty(B, E3, device="cuda")
    ids = torch.full((B, steps), -7, dtype=torch.int64, device="cuda")
    logp, kept = torch.full((B, steps), 7.0, device="cuda"), torch.full((B, steps), -7, dtype=torch.int32, device="cuda")
    wsb = lib.sat_sample_decode_ex_ws_bytes(B, E3, H3, V, nl)
    ws, ws_ptr = L.workspace256(wsb, "cuda")
    cs, keep = c_struct(rules)
    head = (feats.data_ptr(), dec.embed.weight.data_ptr(), dec._lstm_ptrs(), nl, dec.linear.weight.data_ptr(), dec.linear.bias.data_ptr(), B,
            E3, H3, V, steps, draw["tau"], draw["k"], draw["p"], draw["seed"], draw["rank"], h.data_ptr(), c.data_ptr(), ht.data_ptr(),
            xe.data_ptr(), ids.data_ptr(), ids.stride(0), logp.data_ptr(), kept.data_ptr(), None, 0)
    if ex:
        L.check(lib.sat_sample_decode_ex(*head, C.byref(cs) if cs is not None else None, ws_ptr, wsb, L.stream()), "sat_sample_decode_ex")
    else:
        L.check(lib.sat_sample_decode(*head, ws_ptr, wsb, L.stream()), "sat_sample_decode")
    torch.cuda.synchronize()
    del keep
    return ids, logp, kept


@pytest.mark.parametrize("steps", [4, 20])
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("B", [1, 5])
def test_decode_ex_is_the_chain_of_its_single_steps(B, layers, steps):
    dec = make_decoder(layers, 100 * layers + 10 * B + steps)
    feats = torch.randn(B, E3).cuda()
    draw = dict(tau=0.9, k=30, p=0.95, seed=SEED, rank=RANK)
    want = chain(dec, feats, steps, draw, LOOP_RULES)
    got = decode_call(dec, feats, steps, draw, LOOP_RULES)
    assert (want[0] >= 0).all() and (want[0] < V3).all()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)) and torch.equal(got[2], want[2])
    assert SC.check_properties(got[0].cpu().numpy(), LOOP_RULES, V3) == B * steps
    # with c off (NULL, or every field at its "off" value): sat_sample_decode, bit for bit
    base = decode_call(dec, feats, steps, draw, None, ex=False)
    for rules in (None, SC.Rules()):
        off = decode_call(dec, feats, steps, draw, rules)
        assert torch.equal(off[0], base[0]) and torch.equal(off[1].view(torch.int32), base[1].view(torch.int32)) and torch.equal(off[2], base[2])
    if steps == 20 and B == 5:
        assert not torch.equal(base[0], got[0])                                 # the rules do bind somewhere


# ---- 4: the models -----------------------------------------------------------------------------------------------------------------
MODEL_KW = dict(suppress_ids=[0, 1, 3], min_length=5, end_id=2, no_repeat_ngram_size=2, block_repeat=True, repetition_penalty=1.3)
MODEL_RULES = SC.Rules(suppress_ids=(0, 1, 3), min_length=5, end_id=2, no_repeat_ngram=2, block_repeat=True, repetition_penalty=1.3)


def replay(logits, ids, logp, kept, tau, k, p, seed, rank, rules):
    """every step on the host: the returned RAW logits [steps, R, V] -> reference transform with ids[:, :t] -> the unchanged
    sat_sample_filtered == ids[:, t], logp[:, t], kept[:, t], bit for bit"""
    steps, R_, V = logits.shape
    changed = 0
    for t in range(steps):
        xp = SC.transform_rows(logits[t], ids[:, :t], rules)
        changed += int(not np.array_equal(bits(xp), bits(logits[t])))
        want = plain(xp, pad4(V), R_, tau, k, p, seed, t, rank)
        assert same_bits((ids[:, t], kept[:, t], logp[:, t]), want), t
    assert changed >= steps - 1
    return SC.check_properties(ids, rules, V)


def test_decoder_sample_stochastic_under_constraints():
    B, S = 3, 2
    dec = make_decoder(2, 7)
    dec.ss_rank = 2
    feats = torch.randn(B, E3).cuda()
    tau, k, p = 0.8, 30, 0.9
    ids, lp, logits = dec.sample_stochastic(feats, temperature=tau, top_k=k, top_p=p, num_samples=S, seed=99, return_logprobs=True,
                                            return_logits=True, **MODEL_KW)
    assert ids.shape == (B, S, 20) and logits.shape == (20, B * S, V3)
    n = replay(logits.cpu().numpy(), ids.reshape(B * S, 20).cpu().numpy(), lp["logp"].reshape(B * S, 20).cpu().numpy(),
               lp["kept"].reshape(B * S, 20).cpu().numpy(), tau, k, p, 99, 2, MODEL_RULES)
    assert n == 20 * B * S
    again = dec.sample_stochastic(feats, temperature=tau, top_k=k, top_p=p, num_samples=S, seed=99, **MODEL_KW)
    assert torch.equal(again, ids)
    # the defaults, spelt out, are the call without the keywords -- and not the constrained ids
    bare = dec.sample_stochastic(feats, temperature=tau, top_k=k, top_p=p, num_samples=S, seed=99)
    spelt = dec.sample_stochastic(feats, temperature=tau, top_k=k, top_p=p, num_samples=S, seed=99, suppress_ids=None, min_length=0,
                                  no_repeat_ngram_size=0, block_repeat=False, repetition_penalty=1.0, end_id=None)
    assert torch.equal(bare, spelt) and not torch.equal(bare, ids)
    # each rule alone keeps its promise over the 20 steps
    for kw, rules in ((dict(no_repeat_ngram_size=1), SC.Rules(no_repeat_ngram=1)), (dict(block_repeat=True), SC.Rules(block_repeat=True)),
                      (dict(min_length=20, end_id=2), SC.Rules(min_length=20, end_id=2)), (dict(suppress_ids=[4, 5, 6]), SC.Rules(suppress_ids=(4, 5, 6)))):
        one = dec.sample_stochastic(feats, temperature=1.5, seed=5, **kw)
        assert SC.check_properties(one.cpu().numpy(), rules, V3) == 20 * B
    assert len(set(dec.sample_stochastic(feats, temperature=1.5, seed=5, no_repeat_ngram_size=1)[0].tolist())) == 20


def test_attend_sample_stochastic_under_constraints():
    torch.manual_seed(11)
    B, P, C_, E, H, V = 3, 16, 32, 16, 48, 67                                   # (the LSTMCell input is cat[embedding, context])
    model = sat.ShowAttendTellModel(H, C_, V, E, None, feature_size=(P, C_), compute_dtype="f32", vgg_cfg=[C_]).cuda().eval()
    model.classifier.weight.data.mul_(4.0)
    model.ss_rank = 1
    feats = torch.randn(B, P, C_).cuda()
    tau, k, p = 0.8, 30, 0.9
    ids, lp, logits = model.sample_stochastic_features(feats, temperature=tau, top_k=k, top_p=p, seed=123, return_logprobs=True,
                                                       return_logits=True, **MODEL_KW)
    assert ids.shape == (B, 20) and logits.shape == (20, B, V)
    n = replay(logits.cpu().numpy(), ids.cpu().numpy(), lp["logp"].cpu().numpy(), lp["kept"].cpu().numpy(), tau, k, p, 123, 1, MODEL_RULES)
    assert n == 20 * B
    assert torch.equal(model.sample_stochastic_features(feats, temperature=tau, top_k=k, top_p=p, seed=123, **MODEL_KW), ids)
    bare = model.sample_stochastic_features(feats, temperature=tau, top_k=k, top_p=p, seed=123)
    spelt = model.sample_stochastic_features(feats, temperature=tau, top_k=k, top_p=p, seed=123, suppress_ids=None, min_length=0,
                                             no_repeat_ngram_size=0, block_repeat=False, repetition_penalty=1.0, end_id=None)
    assert torch.equal(bare, spelt) and not torch.equal(bare, ids)
    many = model.sample_stochastic_features(feats, temperature=tau, seed=123, num_samples=2, steps=7, **MODEL_KW)
    assert many.shape == (B, 2, 7) and SC.check_properties(many.cpu().numpy(), MODEL_RULES, V) == 7 * 2 * B


def test_show_and_tell_forwards_the_constraints():
    torch.manual_seed(3)
    E, H, V, B = 32, 64, 67, 2
    model = sat.ShowAndTell(E, H, V, 1, arch=dict(layers=(1, 1, 1, 1), width=8), compute_dtype="f32").cuda().eval()
    model.decoder.linear.weight.data.uniform_(-0.9, 0.9)
    images = torch.randn(B, 3, 64, 64).cuda()
    ids = model.sample_stochastic(images, temperature=1.2, seed=17, **MODEL_KW)
    want = model.decoder.sample_stochastic(model.encoder(images), temperature=1.2, seed=17, **MODEL_KW)
    assert ids.shape == (B, 20) and torch.equal(ids, want)
    assert SC.check_properties(ids.cpu().numpy(), MODEL_RULES, V) == 20 * B
    assert torch.equal(model.sample_stochastic(images, temperature=1.2, seed=17),
                       model.sample_stochastic(images, temperature=1.2, seed=17, repetition_penalty=1.0, block_repeat=False))


def test_decode_samples_forwards_the_constraints():
    dec = make_decoder(1, 5)
    feats = torch.randn(3, E3).cuda()
    rng = np.random.Generator(np.random.PCG64(71))
    refs = [[[int(t) for t in rng.integers(3, V3, rng.integers(3, 12))] for _ in range(2)] for _ in range(10)]
    rr = sat.ConsensusReranker(sat.CiderScorer(refs), end_id=2)
    picked = rr.decode_samples(dec, feats, num_samples=4, seed=1234, temperature=1.3, **MODEL_KW)
    want = dec.sample_stochastic(feats, num_samples=4, seed=1234, temperature=1.3, **MODEL_KW)
    assert tuple(picked.shape) == (3, 20) and torch.equal(rr.last_ids, want)
    assert SC.check_properties(rr.last_ids.cpu().numpy(), MODEL_RULES, V3) == 3 * 4 * 20


# ---- 5: argument errors of the two C entry points ----------------------------------------------------------------------------------
def test_c_argument_errors_come_back_without_a_launch():
    lib = L.load()
    B, V, steps = 3, V3, 4
    ldl = pad4(V)
    logits = torch.randn(B, ldl, device="cuda")
    ids = torch.full((B, steps), -7, dtype=torch.int64, device="cuda")
    logp, kept = torch.full((B,), 7.0, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")
    pre = torch.zeros(B, 64, dtype=torch.int64, device="cuda")
    sup = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    wsb = lib.sat_sample_filtered_ws_bytes(B, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

    def cons(**kw):
        kw.setdefault("repetition_penalty", 1.0)
        kw.setdefault("end_id", -1)
        return L.SatSampleConstraints(**kw)

    good = cons(suppress_ids=sup.data_ptr(), n_suppress=2, min_length=3, no_repeat_ngram=2, block_repeat=1, repetition_penalty=1.2, end_id=2)

    def filt(c=good, t=1, V=V, ldl=ldl, prefix=pre.data_ptr(), wsb=wsb):
        return lib.sat_sample_filtered_ex(logits.data_ptr(), ldl, B, V, 1.0, 0, 1.0, 5, t, 0, ids.data_ptr(), steps, logp.data_ptr(),
                                          kept.data_ptr(), C.byref(c), prefix, 64, ws.data_ptr(), wsb, L.stream())

    for bad in (dict(n_suppress=-1), dict(min_length=-1, end_id=2), dict(no_repeat_ngram=-1), dict(block_repeat=2),
                dict(n_suppress=257, suppress_ids=sup.data_ptr()), dict(n_suppress=1), dict(repetition_penalty=0.0),
                dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")), dict(min_length=1)):
        assert filt(c=cons(**bad)) == ARG, bad
    assert filt(prefix=None) == ARG and filt(ldl=V - 1) == ARG
    assert filt(t=64) == UNSUPPORTED and filt(c=cons(repetition_penalty=1.5), t=64) == UNSUPPORTED
    assert filt(V=32769, ldl=32769) == UNSUPPORTED and filt(wsb=wsb - 1) == WORKSPACE

    dec = make_decoder(1, 1)
    feats = torch.randn(B, E3, device="cuda")
    h, c, ht = (torch.zeros(1, B, H3, device="cuda") for _ in range(3))
    xe = torch.zeros(B, E3, device="cuda")
    dwsb = lib.sat_sample_decode_ex_ws_bytes(B, E3, H3, V, 1)
    dws, dptr = L.workspace256(dwsb, "cuda")

    def decode(cs=good, steps_=steps, wsb_=dwsb):
        return lib.sat_sample_decode_ex(feats.data_ptr(), dec.embed.weight.data_ptr(), dec._lstm_ptrs(), 1, dec.linear.weight.data_ptr(),
                                        dec.linear.bias.data_ptr(), B, E3, H3, V, steps_, 1.0, 0, 1.0, 5, 0, h.data_ptr(), c.data_ptr(),
                                        ht.data_ptr(), xe.data_ptr(), ids.data_ptr(), steps_, None, None, None, 0, C.byref(cs), dptr, wsb_,
                                        L.stream())

    for bad in (dict(min_length=-1, end_id=2), dict(n_suppress=300, suppress_ids=sup.data_ptr()), dict(min_length=2),
                dict(repetition_penalty=-1.0), dict(block_repeat=3)):
        assert decode(cs=cons(**bad)) == ARG, bad
    assert decode(steps_=65, wsb_=1 << 40) == UNSUPPORTED and decode(wsb_=dwsb - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert (ids == -7).all() and (logp == 7.0).all() and (kept == -7).all() and not h.any() and not xe.any()       # nothing ran
    assert filt(t=0, prefix=None) == 0 and decode() == 0                        # and the same calls with good arguments do
    torch.cuda.synchronize()
    assert (ids >= 0).all() and (ids < V).all() and (kept > 0).all()
