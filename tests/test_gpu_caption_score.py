"""GPU: scoring given captions (csrc/sat_score.hip, show-and-tell_amd/score.py) against the f64 reference
(tests/caption_score_reference.py).

Bounds.  `sat_vocab_logp` is held to the error of the route the library already had on the SAME inputs: `sat_gemm_f32x3` (fast
path) or `sat_vocab_logits_fwd` (general path) into stored logits, then `sat_ce_rows`.  Its maximum absolute error against f64 may
be at most twice that route's, with a floor of 1e-6 * max |logit| (both are printed).  `DecoderRNN.score_captions` is held the same
way (`_route_bound`): the route the library had for the same rows is `forward` on sorted (hand-repeated) inputs, its stored f32
logits taken through log_softmax and gather in f64.  A token may miss f64 by twice that route's per-token error plus one ulp of the
largest |token log-probability| in f32 (2^-23 |x|): the new route returns the token as an f32 number, which the f64 gather of the
old one does not round to.  A caption's sum may miss by that times its length.  Where the expected values are the GOLDENS (f32
logits of the imported reference, another implementation) the bound is the suite's for device logits against them, 2e-5
(tests/test_gpu_attend.py, tests/test_gpu_parity.py): a token's log-probability moves by at most twice the logit error (its own
logit and the log-sum-exp); the policy smoke tests use it too."""
import importlib

import numpy as np
import pytest
import torch

import caption_score_reference as R
from oracle import decoder as OD
from test_gpu_kernels import cu, st, sync
from test_oracle_golden import load, params_from_seed

pytestmark = pytest.mark.gpu
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

TOKEN_TOL = 2 * 2e-5
N_ALL = 257
N_CASES = (1, 63, 64, 65, 129, 130, 257)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    return L.load()


def _logp_inputs(H, V, N, scale=1.0, dead_col=None):
    g = torch.Generator().manual_seed(1000 * H + V)
    lda = H + 4
    hs = torch.full((N, lda), float("nan"))
    hs[:, :H] = torch.randn(N, H, generator=g)
    hs[:, H:] = 1e30                                   # the pad of a wider row must never be read
    w = torch.randn(V, H, generator=g) * 0.1 * scale
    b = torch.randn(V, generator=g)
    tgt = torch.randint(0, V, (N,), generator=g)
    plant = [0, min(127, V - 1), min(128, V - 1), V - 1]
    for n in range(N):
        if n % 8 < 4:
            tgt[n] = plant[n % 8]
    if N > 6:
        tgt[5], tgt[6] = -3, V + 5                     # clamped to 0 and V - 1, as sat_ce_rows clamps them
    if dead_col is not None:
        b[dead_col] = -1e30
        tgt[tgt == dead_col] = dead_col + 1
    x = hs[:, :H].double() @ w.double().t() + b.double()
    tc = tgt.clamp(0, V - 1)
    lse = torch.logsumexp(x, 1)
    ref = x.gather(1, tc.view(-1, 1)).view(-1) - lse
    return hs, lda, w, b, tgt, x, ref, lse


def _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N, H, V, packed=None, ws_bytes=None, want_lse=True):
    need = lib.sat_vocab_logp_ws_bytes(N, H, V) if ws_bytes is None else ws_bytes
    assert need > 0
    ws, ws_ptr = L.workspace256(need, "cuda")
    tok = torch.full((N,), float("nan"), device="cuda")
    lse = torch.full((N,), float("nan"), device="cuda") if want_lse else None
    L.check(lib.sat_vocab_logp(hs_d.data_ptr(), lda, w_d.data_ptr(), L.ptr(packed), b_d.data_ptr(), tgt_d.data_ptr(), N, H, V,
                               tok.data_ptr(), L.ptr(lse), ws_ptr, need, st()), "sat_vocab_logp")
    sync()
    return tok, lse


def _existing_route(lib, hs_d, lda, w_d, b_d, tgt_d, N, H, V, fast):
    """the route the library had: stored logits [N, pad4(V)], then sat_ce_rows -> (-row_loss, row_loss + logit[target])"""
    ldl = L.pad4(V)
    logits = torch.zeros(N, ldl, device="cuda")
    if fast:
        packed = torch.empty(lib.sat_gemm_f32x3_packed_bytes(V, H), dtype=torch.uint8, device="cuda")
        L.check(lib.sat_gemm_f32x3_pack(w_d.data_ptr(), V, H, packed.data_ptr(), st()), "pack")
        L.check(lib.sat_gemm_f32x3(hs_d.data_ptr(), lda, packed.data_ptr(), b_d.data_ptr(), logits.data_ptr(), ldl, N, V, H, st()), "x3")
    else:
        L.check(lib.sat_gemm_f32(0, 0, hs_d.data_ptr(), lda, w_d.data_ptr(), H, logits.data_ptr(), ldl, b_d.data_ptr(), None, N, V, H,
                                 st()), "sat_vocab_logits_fwd's GEMM on strided rows")
    row_loss = torch.empty(N, device="cuda")
    L.check(lib.sat_ce_rows(logits.data_ptr(), ldl, tgt_d.data_ptr(), N, V, 1.0, 0, row_loss.data_ptr(), None, st()), "sat_ce_rows")
    sync()
    tc = tgt_d.clamp(0, V - 1)
    xt = logits.gather(1, tc.view(-1, 1)).view(-1)
    return -row_loss, row_loss.double() + xt.double()


def _check_against_existing(lib, H, V, scale, dead_col, fast, run_new, label, n_all=N_ALL, n_cases=N_CASES):
    """the new kernel on the first N rows against the stored-logits route on the SAME N rows, for every N"""
    hs, lda, w, b, tgt, x, ref, lse_ref = _logp_inputs(H, V, n_all, scale, dead_col)
    hs_d, w_d, b_d, tgt_d = cu(hs), cu(w), cu(b), cu(tgt)
    old_tok, old_lse = _existing_route(lib, hs_d, lda, w_d, b_d, tgt_d, n_all, H, V, fast)      # once; its error is taken over [:N]
    old_tok_err = (old_tok.cpu().double() - ref).abs()
    old_lse_err = (old_lse.cpu() - lse_ref).abs()
    for N in n_cases:
        err_old, err_old_lse = old_tok_err[:N].max().item(), old_lse_err[:N].max().item()
        xn = x[:N]
        floor = 1e-6 * xn[xn.abs() < 1e29].abs().max().item()
        tok, lse = run_new(hs_d, lda, w_d, b_d, tgt_d, N)
        assert torch.isfinite(tok).all() and torch.isfinite(lse).all()
        err = (tok.cpu().double() - ref[:N]).abs().max().item()
        err_lse = (lse.cpu().double() - lse_ref[:N]).abs().max().item()
        print("%s H=%d V=%d N=%d scale=%g: logp err %.3e (stored-logits route %.3e), lse err %.3e (%.3e), floor %.3e"
              % (label, H, V, N, scale, err, err_old, err_lse, err_old_lse, floor))
        assert err <= max(2 * err_old, floor), (N, err, err_old, floor)
        assert err_lse <= max(2 * err_old_lse, floor), (N, err_lse, err_old_lse, floor)


@pytest.mark.parametrize("H,V,scale,dead_col", [(H, V, 1.0, None) for H in (256, 384) for V in (4, 124, 128, 132, 1004)]
                         + [(256, 1004, 15.0, None), (256, 132, 1.0, 130)])
def test_vocab_logp_fast_path_against_f64(lib, H, V, scale, dead_col):
    """one tile, the tile edge +- 4, a ragged last tile of many; the row-tile edges of the 64-row form, which all of these sizes
    run (the 128-row form: test_vocab_logp_tall_row_tiles_against_f64_and_the_short_ones); lda = H + 4; targets at
    columns 0, 127, 128, V - 1; logits of about +-100 (a sum of exp without the maximum overflows); a column of bias -1e30"""
    assert lib.sat_gemm_f32x3_packed_bytes(V, H) > 0

    def run(hs_d, lda, w_d, b_d, tgt_d, N):
        return _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N, H, V)
    if scale > 1:
        assert _logp_inputs(H, V, N_ALL, scale)[5].abs().max().item() > 89          # exp(89) is past f32
    _check_against_existing(lib, H, V, scale, dead_col, True, run, "fast")


@pytest.mark.parametrize("H,V", [(64, 500), (64, 501), (256, 1002)])
def test_vocab_logp_general_path_against_f64(lib, H, V):
    """shapes the split GEMM does not take (H = 64 of the goldens, odd V): chunks of 16 rows, so that 63 .. 257 rows cross chunk
    edges; and the chunk height changes no bit"""
    def run(hs_d, lda, w_d, b_d, tgt_d, N):
        small = lib.sat_vocab_logp_ws_bytes_rows(N, H, V, 16)
        assert small == (min(N, 16) * L.pad4(V) * 4 + 255) // 256 * 256
        tok, lse = _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N, H, V, ws_bytes=small)
        tok2, lse2 = _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N, H, V)
        assert torch.equal(tok, tok2) and torch.equal(lse, lse2)
        return tok, lse
    _check_against_existing(lib, H, V, 1.0, None, False, run, "general")


def test_vocab_logp_is_deterministic_and_row_independent(lib):
    H, V = 256, 1004
    hs, lda, w, b, tgt, x, ref, lse_ref = _logp_inputs(H, V, N_ALL)
    hs_d, w_d, b_d, tgt_d = cu(hs), cu(w), cu(b), cu(tgt)
    tok, lse = _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N_ALL, H, V)
    tok2, lse2 = _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N_ALL, H, V)
    assert torch.equal(tok, tok2) and torch.equal(lse, lse2)
    # a caller's packed copy of the weights gives the bits of the call that packs for itself; lse is optional
    packed = torch.empty(lib.sat_gemm_f32x3_packed_bytes(V, H), dtype=torch.uint8, device="cuda")
    L.check(lib.sat_gemm_f32x3_pack(w_d.data_ptr(), V, H, packed.data_ptr(), st()), "pack")
    tok3, none = _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N_ALL, H, V, packed=packed, want_lse=False)
    assert none is None and torch.equal(tok, tok3)
    # row n alone (one 64-row tile with 63 empty rows) and in the batch of 257
    for n in (0, 63, 64, 200, 256):
        one, one_lse = _vocab_logp(lib, hs_d[n:n + 1].contiguous(), lda, w_d, b_d, tgt_d[n:n + 1].contiguous(), 1, H, V)
        assert torch.equal(one, tok[n:n + 1]) and torch.equal(one_lse, lse[n:n + 1]), n


def test_vocab_logp_tall_row_tiles_against_f64_and_the_short_ones(lib):
    """The 128-row form of the kernel (one workgroup per CU: two pair slots per lane, 128 rows of LDS exchange), which the
    launcher takes when the rows are whole 128-row tiles and there are at least 512 of those: 8192 rows x 1004 columns = 64 x 8.
    Held to the same bound as the 64-row form, and a row gives the same bits in it, in a 257-row batch of 64-row tiles, and
    alone."""
    H, V, N = 256, 1004, 8192
    assert N % 128 == 0 and (N // 128) * ((V + 127) // 128) >= 512             # x3_tall_tiles (sat_gemm_x3_tile.h)
    assert not (N_ALL % 128 == 0)                                               # the 257-row batch runs 64-row tiles
    kept = {}

    def run(hs_d, lda, w_d, b_d, tgt_d, n):
        kept["args"] = (hs_d, lda, w_d, b_d, tgt_d)
        kept["out"] = _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, n, H, V)
        return kept["out"]
    _check_against_existing(lib, H, V, 1.0, None, True, run, "fast, 128-row tiles", n_all=N, n_cases=(N,))
    tok, lse = kept["out"]
    hs_d, lda, w_d, b_d, tgt_d = kept["args"]
    tok2, lse2 = _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N, H, V)
    assert torch.equal(tok, tok2) and torch.equal(lse, lse2)
    short, short_lse = _vocab_logp(lib, hs_d, lda, w_d, b_d, tgt_d, N_ALL, H, V)
    assert torch.equal(short, tok[:N_ALL]) and torch.equal(short_lse, lse[:N_ALL])
    for n in (0, 127, 128, 4095, 4096, 8191):                                   # tile edges; the first, a middle and the last tile
        one, one_lse = _vocab_logp(lib, hs_d[n:n + 1].contiguous(), lda, w_d, b_d, tgt_d[n:n + 1].contiguous(), 1, H, V)
        assert torch.equal(one, tok[n:n + 1]) and torch.equal(one_lse, lse[n:n + 1]), n
    # rows 8000 .. 8191 as a batch of their own: other tiles of the grid, other rows within a tile
    part, part_lse = _vocab_logp(lib, hs_d[8000:].contiguous(), lda, w_d, b_d, tgt_d[8000:].contiguous(), 192, H, V)
    assert torch.equal(part, tok[8000:]) and torch.equal(part_lse, lse[8000:])


def test_caption_logp_sum_is_the_ordered_f64_loop(lib):
    T, R_, bs = 5, 4, [4, 4, 3, 1, 1]
    prefix = [0]
    for n in bs:
        prefix.append(prefix[-1] + n)
    N = prefix[-1]
    g = torch.Generator().manual_seed(3)
    tokv = -(torch.randint(1, 4000, (N,), generator=g).float() / 64.0)          # multiples of 1/64: any order of the f64 sum is exact
    want, want_len, want_tok = [0.0] * R_, [0] * R_, [[0.0] * (T + 2) for _ in range(R_)]
    for t in range(T):
        for r in range(bs[t]):
            v = float(tokv[prefix[t] + r])
            want[r] += v
            want_len[r] += 1
            want_tok[r][t] = v
    logp = torch.full((R_,), float("nan"), dtype=torch.float64, device="cuda")
    length = torch.full((R_,), -1, dtype=torch.int32, device="cuda")
    tok_out = torch.full((R_, T + 2), float("nan"), device="cuda")
    prefix_d = torch.tensor(prefix, dtype=torch.int32, device="cuda")
    L.check(lib.sat_caption_logp_sum(cu(tokv).data_ptr(), prefix_d.data_ptr(), T, R_, logp.data_ptr(), length.data_ptr(),
                                     tok_out.data_ptr(), T + 2, st()), "sat_caption_logp_sum")
    sync()
    assert logp.cpu().tolist() == want and length.cpu().tolist() == want_len == [5, 3, 3, 2]
    got = tok_out.cpu()
    assert got[:, :T].tolist() == [row[:T] for row in want_tok]
    assert torch.isnan(got[:, T:]).all()                                         # the pad of a wider row is not written
    beyond = torch.tensor([[t >= l for t in range(T)] for l in want_len])
    assert (got[:, :T][beyond] == 0).all() and not torch.signbit(got[:, :T][beyond]).any()      # +0.0
    # without the token matrix
    logp2 = torch.empty_like(logp)
    L.check(lib.sat_caption_logp_sum(cu(tokv).data_ptr(), prefix_d.data_ptr(), T, R_, logp2.data_ptr(), length.data_ptr(), None, 0, st()))
    sync()
    assert torch.equal(logp, logp2)


def _decoder(E, H, V, Lh, seed):
    params = OD.init_decoder_params(E, H, V, Lh, generator=torch.Generator().manual_seed(seed))
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    return dec.cuda().eval(), params


_SCORE_CASE = {}


def _score_case(Lh):
    """model, inputs and the f64 reference (paired and cross) at E = H = 256, V = 1004: computed once per layer count"""
    if Lh not in _SCORE_CASE:
        E, H, V = 256, 256, 1004
        dec, params = _decoder(E, H, V, Lh, 40 + Lh)
        g = torch.Generator().manual_seed(7 + Lh)
        lengths = [3, 7, 1, 7, 4]
        caps = torch.randint(3, V, (5, 7), generator=g)
        caps[:, 0] = 1
        feats = torch.randn(5, E, generator=g)
        ref, ref_tok = R.decoder_score(params, feats, caps, lengths, Lh)
        cross, cross_tok = R.decoder_score(params, feats[:3], caps, lengths, Lh, cross=True)
        _SCORE_CASE[Lh] = (dec, params, feats, caps, lengths, ref, ref_tok, cross, cross_tok)
    return _SCORE_CASE[Lh]


def _route_bound(dec, feats, caps, lengths, ref_tok):
    """(bound, the old route's per-token error, its token matrix) for paired rows in the caller's order: `forward` on the rows
    sorted by length, its f32 logits through log_softmax and gather in f64; bound = 2 x its maximum per-token error against f64 +
    one f32 ulp of the largest |token log-probability| (the module docstring says why)"""
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    ls = [lengths[i] for i in order]
    logits = dec(cu(feats[order]), cu(caps[order]), ls)
    _, tok_sorted = R.packed_sums(logits.detach().cpu(), OD.pack_time_major(caps[order], ls), ls)
    fwd_tok = torch.zeros_like(tok_sorted)
    fwd_tok[order] = tok_sorted
    err_fwd = (fwd_tok - ref_tok).abs().max().item()
    return 2 * err_fwd + 2.0 ** -23 * ref_tok.abs().max().item(), err_fwd, fwd_tok


@pytest.mark.parametrize("Lh", [1, 2])
def test_decoder_score_captions_paired(lib, Lh):
    dec, params, feats, caps, lengths, ref, ref_tok, _, _ = _score_case(Lh)
    res = dec.score_captions(cu(feats), cu(caps), lengths, return_tokens=True)
    sync()
    assert res.logp.dtype == torch.float64 and res.length.dtype == torch.int32 and res.token_logp.shape == (5, 7)
    assert res.length.cpu().tolist() == lengths and res.score is res.logp
    lens = torch.tensor(lengths, dtype=torch.float64)
    err_tok = (res.token_logp.cpu().double() - ref_tok).abs().max().item()
    err = ((res.logp.cpu() - ref).abs() / lens).max().item()
    bound, err_fwd, fwd_tok = _route_bound(dec, feats, caps, lengths, ref_tok)
    diff = (res.token_logp.cpu().double() - fwd_tok).abs().max().item()
    print("layers %d: per-token err %.3e, per-caption err / length %.3e; forward route per token %.3e; bound %.3e; routes differ by "
          "%.3e" % (Lh, err_tok, err, err_fwd, bound, diff))
    assert err_tok <= bound and err <= bound
    assert diff <= err_tok + err_fwd
    length_norm = dec.score_captions(cu(feats), cu(caps), lengths, normalize="length")
    assert length_norm.token_logp is None and torch.equal(length_norm.logp, res.logp)
    assert torch.equal(length_norm.score, res.logp / res.length.double())
    with pytest.raises(ValueError):
        dec.score_captions(cu(feats[:3]), cu(caps), lengths)                      # paired needs one feature row per caption
    with pytest.raises(ValueError):
        dec.score_captions(cu(feats), cu(caps), [3, 7, 0, 7, 4])
    with pytest.raises(ValueError):
        dec.score_captions(cu(feats), cu(caps), lengths, normalize="tokens")


@pytest.mark.parametrize("Lh", [1, 2])
def test_decoder_score_captions_cross(lib, Lh):
    dec, params, feats, caps, lengths, ref, _, cross, cross_tok = _score_case(Lh)
    f3 = cu(feats[:3])
    res = dec.score_captions(f3, cu(caps), lengths, cross=True, return_tokens=True)
    sync()
    assert res.logp.shape == (3, 5) and res.token_logp.shape == (3, 5, 7) and res.length.cpu().tolist() == lengths
    lens = torch.tensor(lengths, dtype=torch.float64)
    err = ((res.logp.cpu() - cross).abs() / lens).max().item()
    err_tok = (res.token_logp.cpu().double() - cross_tok).abs().max().item()
    # the route the library had for these 15 pairs: forward on hand-repeated inputs
    bound, err_fwd, _ = _route_bound(dec, feats[:3].repeat_interleave(5, 0), caps.repeat(3, 1), lengths * 3, cross_tok.view(15, 7))
    print("layers %d cross: per-token err %.3e, per-caption err / length %.3e; forward route per token %.3e; bound %.3e"
          % (Lh, err_tok, err, err_fwd, bound))
    assert err <= bound and err_tok <= bound
    # the same pairs, repeated by hand and scored as pairs
    paired = dec.score_captions(f3.repeat_interleave(5, 0), cu(caps).repeat(3, 1), lengths * 3)
    assert ((paired.logp.view(3, 5).cpu() - res.logp.cpu()).abs() / lens).max().item() <= bound
    # the token matrix sums to logp (f64 sums of at most 7 f32 numbers: exact in any order)
    assert torch.equal(res.token_logp.double().sum(-1), res.logp)
    # one image per library call: the same bits
    old = sat.set_workspace_budget(1)
    try:
        one = dec.score_captions(f3, cu(caps), lengths, cross=True, return_tokens=True)
    finally:
        sat.set_workspace_budget(old)
    assert torch.equal(one.logp, res.logp) and torch.equal(one.token_logp, res.token_logp) and torch.equal(one.length, res.length)


def test_decoder_score_captions_at_the_golden_shapes(lib, golden_dir):
    """E 32, H 64, V 500: the general path.  G8's own logits (eval.py:91-95) give the sums; G2's captions with every length
    against the f64 reference, shuffled"""
    g = load(golden_dir, "G8_dec_eval_unshifted.npz")
    params, (E, H, V, Lh, B, T) = params_from_seed(g)
    assert lib.sat_gemm_f32x3_packed_bytes(V, H) == 0
    dec = sat.DecoderRNN(E, H, V, Lh)
    dec.load_state_dict(params)
    dec.cuda().train()                                    # train mode, dropout configured: the same distribution is scored
    dec.dropout_p = 0.5
    lengths = [int(x) for x in g["lengths"]]
    want, want_tok = R.packed_sums(g["logits"], g["targets"], lengths)
    res = dec.score_captions(cu(torch.from_numpy(g["features"])), cu(torch.from_numpy(g["captions"])), lengths, return_tokens=True)
    sync()
    assert (res.token_logp.cpu().double() - want_tok).abs().max().item() <= TOKEN_TOL
    assert ((res.logp.cpu() - want).abs() / torch.tensor(lengths, dtype=torch.float64)).max().item() <= TOKEN_TOL
    g2 = load(golden_dir, "G2_dec_varlen_small.npz")
    params2, _ = params_from_seed(g2)
    dec.load_state_dict(params2)
    perm = [2, 0, 3, 1]
    feats, caps = torch.from_numpy(g2["features"])[perm], torch.from_numpy(g2["captions"])[perm]
    l2 = [int(g2["lengths"][i]) for i in perm]
    ref, ref_tok = R.decoder_score(params2, feats, caps, l2, 1)
    got = dec.score_captions(cu(feats), cu(caps), l2)
    bound, err_fwd, _ = _route_bound(dec.eval(), feats, caps, l2, ref_tok)
    err = ((got.logp.cpu() - ref).abs() / torch.tensor(l2, dtype=torch.float64)).max().item()
    print("G2 shapes, general path: per-caption err / length %.3e; forward route per token %.3e; bound %.3e" % (err, err_fwd, bound))
    assert err <= bound


def test_attend_score_captions_at_the_golden_shape(lib, golden_dir):
    from test_gpu_attend import _model_from_golden
    g = load(golden_dir, "G6_attend_small.npz")
    model, params, dims = _model_from_golden(g)
    model.eval()
    lengths = [int(x) for x in g["lengths"]]
    l1 = [l - 1 for l in lengths]
    want, want_tok = R.packed_sums(g["logits"], g["targets"], l1)
    feats, caps = cu(torch.from_numpy(g["features"])), cu(torch.from_numpy(g["captions"]))
    res = model.score_captions_features(feats, feats.mean(1), caps, lengths, return_tokens=True)
    sync()
    assert res.length.cpu().tolist() == l1
    tok = res.token_logp.cpu()
    beyond = torch.tensor([[t >= l for t in range(max(l1))] for l in l1])
    assert beyond.any() and (tok[beyond] == 0).all() and not torch.signbit(tok[beyond]).any()      # +0.0 beyond a caption's length
    assert (tok[~beyond] < 0).all()
    # with dropout and scheduled sampling configured, train mode scores the same distribution: the same bits
    model.train()
    model.dropout_p, model.ss_prob = 0.5, 0.25
    noisy = model.score_captions_features(feats, feats.mean(1), caps, lengths, return_tokens=True)
    model.dropout_p, model.ss_prob = 0.0, 0
    assert model.training
    model.eval()
    assert torch.equal(noisy.logp, res.logp) and torch.equal(noisy.token_logp, res.token_logp)
    assert (res.token_logp.cpu().double() - want_tok).abs().max().item() <= TOKEN_TOL
    assert ((res.logp.cpu() - want).abs() / torch.tensor(l1, dtype=torch.float64)).max().item() <= TOKEN_TOL
    perm = [3, 1, 0, 2]
    idx = cu(torch.tensor(perm))
    shuffled = model.score_captions_features(feats[idx], feats[idx].mean(1), caps[idx], [lengths[i] for i in perm], normalize="length")
    assert ((shuffled.logp.cpu() - want[perm]).abs() / torch.tensor([l1[i] for i in perm], dtype=torch.float64)).max().item() <= TOKEN_TOL
    assert torch.equal(shuffled.score, shuffled.logp / shuffled.length.double())
    with pytest.raises(NotImplementedError):
        model.score_captions_features(feats, feats.mean(1), caps, lengths, cross=True)
    with pytest.raises(NotImplementedError):
        model.score_captions(torch.zeros(4, 3, 16, 16, device="cuda"), caps, lengths, cross=True)


def _tiny_show_and_tell():
    from oracle import encoder as OE
    arch = dict(layers=(1, 1, 1, 1), width=8)
    E, H, V, Lh = 32, 64, 200, 1
    gen = torch.Generator().manual_seed(1)
    ep, eb = OE.init_encoder_params(E, arch, generator=gen, randomize_bn=True)
    dp = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    model = sat.ShowAndTell(E, H, V, Lh, arch=arch, compute_dtype="f32")
    sd = dict(ep)
    sd.update(eb)
    model.encoder.load_state_dict(sd)
    model.decoder.load_state_dict(dp)
    return model.cuda().eval(), dp, gen, V


def test_show_and_tell_scores_from_images_and_validation_step_reports_them(lib):
    model, dp, gen, V = _tiny_show_and_tell()
    images = cu(torch.randn(2, 3, 64, 64, generator=gen))
    caps = torch.randint(4, V, (2, 9), generator=gen)
    caps[:, 0] = 1
    lengths = [9, 6]
    res = model.score_captions(images, cu(caps), lengths)
    feats = model.encoder(images)
    direct = model.decoder.score_captions(feats, cu(caps), lengths)
    ref, _ = R.decoder_score(dp, feats.cpu(), caps, lengths, 1)
    sync()
    assert torch.equal(res.logp, direct.logp)
    assert ((res.logp.cpu() - ref).abs() / torch.tensor(lengths, dtype=torch.float64)).max().item() <= TOKEN_TOL
    plain = sat.validation_step(model, images, cu(caps), lengths)
    assert sorted(plain) == ["ids", "kept", "loss"]
    out = sat.validation_step(model, images, cu(caps), lengths, caption_logp=True)
    assert sorted(out) == ["caption_logp", "caption_token_count", "ids", "kept", "loss"]
    assert out["caption_logp"].dtype == torch.float64 and out["caption_token_count"].cpu().tolist() == lengths
    assert torch.equal(out["loss"], plain["loss"])
    # the rows of the validation forward are the rows score_captions scores
    assert ((out["caption_logp"] - res.logp).abs().cpu() / torch.tensor(lengths, dtype=torch.float64)).max().item() <= TOKEN_TOL
    mean = (-out["caption_logp"].sum() / sum(lengths)).item()
    loss = out["loss"].item()
    # f32 mean of 15 f32 row losses: each partial sum rounds once (15 * 2^-24 relative), plus the rounding of the result
    assert abs(mean - loss) <= 16 * 2.0 ** -24 * abs(loss), (mean, loss)


def test_retrieval_metrics_on_the_device_equal_the_double_loop(lib):
    g = torch.Generator().manual_seed(11)
    scores = torch.randint(0, 6, (6, 14), generator=g).double()                  # many ties
    caption_image = torch.tensor([0, 0, 1, 1, 1, 2, 3, 3, 4, 4, 4, 5, 5, 2])
    want = R.retrieval_metrics(scores.numpy(), caption_image.tolist())
    got = sat.retrieval_metrics(cu(scores), cu(caption_image))
    for k in want:
        assert got[k].is_cuda and got[k].item() == want[k], k


def test_rescore_ranks_candidates_by_the_reference_likelihood(lib):
    dec, params = _decoder(256, 256, 1004, 1, 77)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 256, generator=g)
    greedy = dec.sample(cu(feats)).view(2, 20)
    ids = torch.randint(3, 1004, (2, 3, 20), generator=g)
    ids[:, 1] = greedy.cpu()
    ids[0, 0, 6], ids[0, 1, 9], ids[1, 2, 0] = 2, 2, 2                           # planted <end>; the rest run to T
    caps, lengths = R.candidate_captions(ids.view(6, 20).tolist())
    ref, _ = R.decoder_score(params, feats.repeat_interleave(3, 0), caps, lengths, 1)
    lens = torch.tensor(lengths, dtype=torch.float64)
    for normalize, want in (("none", ref), ("length", ref / lens)):
        best, score = sat.rescore(dec, cu(feats), cu(ids), end_id=2, normalize=normalize)
        sync()
        assert score.shape == (2, 3) and best.shape == (2,)
        scale = lens if normalize == "none" else torch.ones(6, dtype=torch.float64)
        assert ((score.cpu().view(6) - want).abs() / scale).max().item() <= TOKEN_TOL
        srt = want.view(2, 3).sort(1, descending=True)[0]
        if (srt[:, 0] - srt[:, 1]).min().item() > 2 * TOKEN_TOL * 21:
            assert torch.equal(best.cpu(), want.view(2, 3).argmax(1))
    # (the property "greedy ranks at least as high as a candidate sharing its first differing prefix" holds per step, not for
    # whole-sequence sums from arbitrary seeds: not asserted)
