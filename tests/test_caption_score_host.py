"""CPU: scoring given captions (show-and-tell_amd/score.py, csrc/sat_score.hip) -- the f64 reference module pinned by the goldens
of the imported reference decoders, the ordering contract, `retrieval_metrics` against a double loop, the C ABI of the new
entry points, the workspace bound that no design with stored logits can meet, argument errors before any launch, and the
candidate -> caption convention of `rescore`."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import caption_score_reference as R
from oracle import attend as OA
from oracle import decoder as OD
from test_oracle_attend_golden import setup as attend_setup
from test_oracle_golden import load, params_from_seed

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

LOGIT_ATOL = 2e-6           # tests/test_oracle_golden.py: the oracle's logits against the reference's


def golden_sums(g, lengths):
    """the reference's own logits and targets -> sum of log_softmax(logits)[target] per caption, f64"""
    return R.packed_sums(g["logits"], g["targets"], lengths)


@pytest.mark.parametrize("name", ["G1_dec_fwd_bwd_small.npz", "G2_dec_varlen_small.npz", "G5_dec_L2.npz"])
def test_reference_decoder_sums_match_the_goldens_training_rows(golden_dir, name):
    """G1 / G2 / G5 (train.py:134-139): the decoder fed [features, captions[:, :l-2]] against captions[:, 1:], lengths - 1"""
    g = load(golden_dir, name)
    params, (E, H, V, Lh, B, T) = params_from_seed(g)
    caps = torch.from_numpy(g["captions"])
    l1 = [int(x) - 1 for x in g["lengths"]]
    want, want_tok = golden_sums(g, l1)
    got, got_tok = R.decoder_sorted(params, torch.from_numpy(g["features"]), caps[:, :-1], caps[:, 1:], l1, Lh)
    # a token's log-probability moves by at most twice the largest logit error (its own logit and the log-sum-exp)
    np.testing.assert_allclose(got_tok.numpy(), want_tok.numpy(), rtol=0, atol=2 * LOGIT_ATOL)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2 * LOGIT_ATOL * max(l1))


def test_reference_decoder_sums_match_the_unshifted_eval_golden(golden_dir):
    """G8 (eval.py:91-95): captions unshifted, lengths full -- the rows `score_captions` scores"""
    g = load(golden_dir, "G8_dec_eval_unshifted.npz")
    params, (E, H, V, Lh, B, T) = params_from_seed(g)
    lengths = [int(x) for x in g["lengths"]]
    want, want_tok = golden_sums(g, lengths)
    got, got_tok = R.decoder_score(params, torch.from_numpy(g["features"]), torch.from_numpy(g["captions"]), lengths, Lh)
    np.testing.assert_allclose(got_tok.numpy(), want_tok.numpy(), rtol=0, atol=2 * LOGIT_ATOL)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2 * LOGIT_ATOL * max(lengths))


def test_reference_attend_sums_match_the_golden(golden_dir):
    g = load(golden_dir, "G6_attend_small.npz")
    params, dims = attend_setup(g)
    lengths = [int(x) for x in g["lengths"]]
    l1 = [l - 1 for l in lengths]
    want, want_tok = golden_sums(g, l1)
    got, got_tok = R.attend_score(params, torch.from_numpy(g["features"]), torch.from_numpy(g["captions"]), lengths)
    np.testing.assert_allclose(got_tok.numpy(), want_tok.numpy(), rtol=0, atol=2 * LOGIT_ATOL)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2 * LOGIT_ATOL * max(l1))


def test_shuffled_captions_give_the_shuffled_result(golden_dir):
    g = load(golden_dir, "G8_dec_eval_unshifted.npz")
    params, (E, H, V, Lh, B, T) = params_from_seed(g)
    feats, caps = torch.from_numpy(g["features"]), torch.from_numpy(g["captions"])
    lengths = [int(x) for x in g["lengths"]]
    base, base_tok = R.decoder_score(params, feats, caps, lengths, Lh)
    perm = [2, 0, 3, 1]
    got, got_tok = R.decoder_score(params, feats[perm], caps[perm], [lengths[i] for i in perm], Lh)
    np.testing.assert_allclose(got.numpy(), base[perm].numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_tok.numpy(), base_tok[perm].numpy(), rtol=0, atol=1e-12)
    # cross: row b of the matrix is image b under every caption; its diagonal is the paired result
    cross, _ = R.decoder_score(params, feats, caps, lengths, Lh, cross=True)
    assert cross.shape == (B, B)
    np.testing.assert_allclose(torch.diagonal(cross).numpy(), base.numpy(), rtol=0, atol=1e-12)
    cross_p, _ = R.decoder_score(params, feats, caps[perm], [lengths[i] for i in perm], Lh, cross=True)
    np.testing.assert_allclose(cross_p.numpy(), cross[:, perm].numpy(), rtol=0, atol=1e-12)


def test_retrieval_metrics_equal_the_double_loop_with_ties():
    scores = torch.tensor([[3., 1., 3., 0., 2., 2., 5., 5., 1.],
                           [0., 4., 4., 4., 1., 0., 2., 2., 2.],
                           [3., 1., 3., 7., 7., 2., 0., 5., 1.],
                           [3., 4., 3., 0., 1., 2., 5., 5., 6.]], dtype=torch.float64)
    caption_image = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 3])
    want = R.retrieval_metrics(scores.numpy(), caption_image.tolist(), ks=(1, 2, 5))
    got = sat.retrieval_metrics(scores, caption_image, ks=(1, 2, 5))
    assert sorted(got) == sorted(want) == sorted(["%s_r@%d" % (d, k) for d in ("i2s", "s2i") for k in (1, 2, 5)] + ["i2s_medr", "s2i_medr"])
    for k in want:
        assert got[k].dtype == torch.float64 and got[k].dim() == 0
        assert got[k].item() == want[k], k
    # by hand: image 0's captions 0, 1 score 3, 1 behind the two 5s: rank 3; images 1 and 2 tie with an earlier caption: rank 2;
    # image 3's caption 8 leads its row: rank 1
    assert want["i2s_r@1"] == 0.25 and want["i2s_r@2"] == 0.75 and want["i2s_medr"] == 2.0
    with pytest.raises(ValueError):
        sat.retrieval_metrics(scores, caption_image[:-1])


def test_new_symbols_are_exported_with_their_signatures():
    lib = L.load()
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    want = {
        "sat_vocab_logp_ws_bytes": (i64, [i, i, i]),
        "sat_vocab_logp": (i, [vp, i64, vp, vp, vp, vp, i, i, i, vp, vp, vp, i64, vp]),
        "sat_caption_logp_sum": (i, [vp, vp, i, i, vp, vp, vp, i64, vp]),
        "sat_score_captions_ws_bytes": (i64, [i, i, i, i, i, i, i]),
        "sat_score_captions": (i, [vp, vp, C.POINTER(vp), i, vp, vp, vp, i64, i, vp, vp, C.POINTER(C.c_int32), vp, i, i, i, i, i, i, i, vp, vp,
                                   vp, i64, vp, i64, vp]),
    }
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert name in L.ADDED_WITHIN_ABI
    assert lib.sat_version() == 18                       # added within the ABI: the committed tune table stays valid


def test_workspace_is_far_below_the_logits():
    lib = L.load()
    B_img, Cn, T, E, H, V = 64, 320, 20, 256, 512, 10000
    R_, N = B_img * Cn, B_img * Cn * 12
    logits_bytes = N * V * 4
    for layers in (1, 2):
        ws = lib.sat_score_captions_ws_bytes(B_img, R_, N, E, H, V, layers)
        assert 0 < ws < logits_bytes // 10, (layers, ws, logits_bytes)
        assert ws >= N * H * 4                           # the hidden states of every scored row are there
    # the projection alone: 8 bytes per row and 128-column tile, the target logit, the packed weights
    assert lib.sat_vocab_logp_ws_bytes(N, H, V) < N * (8 * 79 + 4) + 79 * 128 * H * 6 + 4096
    # general path (H = 64: no packed form): a bounded scratch, whatever N
    assert lib.sat_vocab_logp_ws_bytes(1 << 20, 64, 501) == lib.sat_vocab_logp_ws_bytes(1 << 22, 64, 501) <= (64 << 20) + 256
    assert lib.sat_vocab_logp_ws_bytes_rows(1000, 64, 501, 7) == (7 * 504 * 4 + 255) // 256 * 256
    assert lib.sat_score_captions_ws_bytes(4, 4, 3, 32, 64, 500, 1) == 0 and lib.sat_score_captions_ws_bytes(4, 4, 8, 32, 64, 500, 9) == 0


def test_argument_errors_return_before_any_launch():
    """no GPU here: an entry point that launched anything would fail with a HIP error instead of SAT_ERR_ARG"""
    lib = L.load()
    p = 0x1000                   # non-NULL, aligned, never dereferenced: the checks below fail first
    assert lib.sat_vocab_logp(None, 256, p, None, p, p, 4, 256, 1004, p, None, p, 1 << 30, None) == 1001
    assert lib.sat_vocab_logp(p, 256, p, None, p, None, 4, 256, 1004, p, None, p, 1 << 30, None) == 1001
    assert lib.sat_vocab_logp(p, 256, p, None, p, p, 0, 256, 1004, p, None, p, 1 << 30, None) == 1001         # N < 1
    assert lib.sat_vocab_logp(p, 252, p, None, p, p, 4, 256, 1004, p, None, p, 1 << 30, None) == 1001         # lda < H
    assert lib.sat_vocab_logp(p, 256, p, None, p, p, 4, 256, 1004, p, None, p, 1024, None) == 1001            # workspace too small
    assert lib.sat_vocab_logp(p, 64, p, None, p, p, 4, 64, 501, p, None, p, 2000, None) == 1001               # less than one row of logits
    assert lib.sat_vocab_logp(p, 256, p, None, p, p, 4, 256, 1004, p, None, None, 1 << 30, None) == 1001
    assert lib.sat_caption_logp_sum(None, p, 5, 4, p, p, None, 0, None) == 1001
    assert lib.sat_caption_logp_sum(p, p, 0, 4, p, p, None, 0, None) == 1001
    assert lib.sat_caption_logp_sum(p, p, 5, 4, p, p, p, 4, None) == 1001                                     # tok_stride < T
    w = (C.c_void_p * 4)(p, p, p, p)
    bs = (C.c_int32 * 3)(4, 3, 1)

    def score(features=p, lstm_w=w, layers=1, batch_sizes=bs, R_=4, N=8, ws=p, ws_bytes=1 << 30, E=32):
        return lib.sat_score_captions(features, p, lstm_w, layers, p, p, p, 3, 4, p, p, batch_sizes, p, 3, 4, R_, N, E, 64, 500, p, p,
                                      None, 0, ws, ws_bytes, None)
    assert score(features=None) == 1001
    assert score(layers=9) == 1001
    assert score(lstm_w=(C.c_void_p * 4)(p, None, p, p)) == 1001
    assert score(batch_sizes=(C.c_int32 * 3)(4, 5, 1)) == 1001          # not non-increasing
    assert score(batch_sizes=(C.c_int32 * 3)(3, 3, 2)) == 1001          # batch_sizes[0] != R
    assert score(N=9) == 1001                                           # sum(batch_sizes) != N
    assert score(E=30) == 1001
    assert score(ws_bytes=4096) == 1001
    assert score(ws=p + 16) == 1001                                     # workspace not 256-byte aligned
    with pytest.raises(ValueError):
        sat.set_workspace_budget(0)
    with pytest.raises(RuntimeError):                                   # host tensors: refused before anything else
        sat.DecoderRNN(32, 64, 500, 1).score_captions(torch.zeros(2, 32), torch.zeros(2, 5, dtype=torch.int64), [5, 3])


def test_candidate_convention_with_a_planted_end(golden_dir):
    """`rescore`: <start> in front, the first <end> is the last scored token, a row without one keeps its T ids"""
    g = load(golden_dir, "G8_dec_eval_unshifted.npz")
    params, (E, H, V, Lh, B, T) = params_from_seed(g)
    ids = [[7, 9, 2, 11, 2, 5], [2, 8, 8, 8, 8, 8], [7, 9, 4, 11, 6, 5], [7, 9, 4, 11, 6, 2]]
    caps, lengths = R.candidate_captions(ids, end_id=2, start_id=1)
    assert lengths == [4, 2, 7, 7] and caps.shape == (4, 7)
    assert caps[:, 0].tolist() == [1] * 4 and caps[0, 1:].tolist() == ids[0]
    feats = torch.from_numpy(g["features"])
    lp, tok = R.decoder_score(params, feats, caps, lengths, Lh)
    # what follows the first <end> does not count: another tail, the same score
    ids2 = [row[:] for row in ids]
    ids2[0][3:] = [400, 401, 402]
    caps2, lengths2 = R.candidate_captions(ids2, end_id=2, start_id=1)
    assert lengths2 == lengths
    lp2, _ = R.decoder_score(params, feats, caps2, lengths2, Lh)
    assert torch.equal(lp, lp2)
    assert (tok[0, 4:] == 0).all() and (tok[0, :4] < 0).all() and (tok[2] < 0).all()
    # length normalisation divides by the scored tokens, <start> and <end> included
    assert torch.allclose(lp / torch.tensor(lengths, dtype=torch.float64), tok.sum(1) / torch.tensor([4., 2., 7., 7.], dtype=torch.float64))
