"""CPU: dropout's host side -- the library exports `sat_dropout_f32` and rejects bad arguments before any launch,
the attributes default to 0, bad probabilities and the combinations that are not built raise on the host without drawing from
torch's generator, and the numpy restatement of the mask (tests/dropout_reference.py) has the statistics and the stream
separation the contract in include/sat_hip.h promises."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import dropout_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
TINY = dict(layers=(1, 1, 1, 1), width=8)


def decoder(num_layers=2):
    return sat.DecoderRNN(8, 16, 50, num_layers).train()


def attend_model():
    return sat.ShowAttendTellModel(20, 8, 29, 12, None, feature_size=(6, 8), compute_dtype="f32", vgg_cfg=[8]).train()


DEC_ARGS = (torch.zeros(2, 8), torch.zeros(2, 5, dtype=torch.long), [6, 4])
ATT_ARGS = (torch.zeros(2, 6, 8), torch.zeros(2, 8), torch.zeros(2, 5, dtype=torch.long), [5, 3])


def test_library_exports_and_header_declares_sat_dropout_f32():
    lib = L.load()
    assert hasattr(lib, "sat_dropout_f32") and "sat_dropout_f32" in L.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert re.search(r"\bint sat_dropout_f32\(const float\* x, int64_t ldx, float\* y, int64_t ldy, int rows, int cols,\s*float p, "
                     r"uint64_t seed, int rank, int site,\s*sat_stream_t stream\);", hdr)
    assert "0x80000000 | site" in hdr and "16777216.0" in hdr              # the contract paragraph


def test_bad_arguments_are_rejected_before_any_launch():
    """no GPU here: every one of these returns before the library touches the device"""
    lib = L.load()
    x = torch.zeros(4, 8)
    a = x.data_ptr()                                                         # (a host address: never dereferenced)
    for p in (-0.1, 1.0, float("nan"), float("inf"), 1.5):
        assert lib.sat_dropout_f32(a, 8, a, 8, 4, 8, p, 1, 0, 0, None) == 1001, p
    assert lib.sat_dropout_f32(a, 8, a, 8, -1, 8, 0.5, 1, 0, 0, None) == 1001
    assert lib.sat_dropout_f32(a, 8, a, 8, 4, -1, 0.5, 1, 0, 0, None) == 1001
    assert lib.sat_dropout_f32(a, 7, a, 8, 4, 8, 0.5, 1, 0, 0, None) == 1001        # ldx < cols
    assert lib.sat_dropout_f32(a, 8, a, 7, 4, 8, 0.5, 1, 0, 0, None) == 1001        # ldy < cols
    assert lib.sat_dropout_f32(a, 8, a, 8, 4, 8, 0.5, 1, -1, 0, None) == 1001       # rank
    assert lib.sat_dropout_f32(a, 8, a, 8, 4, 8, 0.5, 1, 0, -1, None) == 1001       # site
    assert lib.sat_dropout_f32(None, 8, a, 8, 4, 8, 0.5, 1, 0, 0, None) == 1001
    assert lib.sat_dropout_f32(a, 8, None, 8, 4, 8, 0.5, 1, 0, 0, None) == 1001
    assert lib.sat_dropout_f32(a, 8, a, 8, 0, 8, 0.5, 1, 0, 0, None) == 0           # nothing to do: no launch
    assert lib.sat_dropout_f32(a, 8, a, 8, 4, 0, 0.5, 1, 0, 0, None) == 0
    assert lib.sat_dropout_f32(a, 8, a, 8, 4, 8, 0.0, 1, 0, 0, None) == 0           # p = 0 in place: returns without a launch
    assert float(x.abs().sum()) == 0


def test_attribute_defaults_are_zero():
    dec, m = decoder(), attend_model()
    assert dec.dropout_p == 0 and dec.lstm_dropout_p == 0 and dec.last_dropout_seed is None
    assert m.dropout_p == 0 and m.last_dropout_seed is None
    assert dec.dropout_plan() is None and m.dropout_plan() is None


@pytest.mark.parametrize("bad", [-0.1, 1.0, float("nan"), "x"])
def test_bad_probability_raises_value_error_naming_the_attribute(bad):
    dec, m = decoder(), attend_model()                # (building a model initialises its weights from torch's generator)
    state = torch.get_rng_state()
    for mode in (True, False):
        for attr in ("dropout_p", "lstm_dropout_p"):
            dec.train(mode)
            dec.dropout_p = dec.lstm_dropout_p = 0.0
            setattr(dec, attr, bad)
            with pytest.raises(ValueError, match=attr):
                dec(*DEC_ARGS)
        m.train(mode)
        m.dropout_p = bad
        with pytest.raises(ValueError, match="dropout_p"):
            m.decode(*ATT_ARGS)
        with pytest.raises(ValueError, match="dropout_p"):
            m(torch.zeros(2, 3, 16, 16), ATT_ARGS[2], ATT_ARGS[3])
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="dropout_p"):
        sat.models.check_dropout_p(True, "dropout_p")
    assert sat.models.check_dropout_p(0.5, "dropout_p") == 0.5 and sat.models.check_dropout_p(0, "dropout_p") == 0.0
    with pytest.raises(ValueError):
        sat.models.check_dropout_p(1.0 - 2.0 ** -30, "dropout_p")           # 1.0 as the float32 the kernel receives


def test_combinations_that_are_not_built_raise_before_anything_is_drawn():
    dec, one, model, m = decoder(), decoder(num_layers=1), sat.ShowAndTell(8, 16, 50, 1, arch=TINY, compute_dtype="f32").train(), attend_model()
    state = torch.get_rng_state()
    for attr in ("dropout_p", "lstm_dropout_p"):
        dec.dropout_p = dec.lstm_dropout_p = 0.0
        setattr(dec, attr, 0.5)
        dec.ss_prob = 0.25
        with pytest.raises(NotImplementedError, match=r"(?s)%s.*ss_prob" % attr):
            dec(*DEC_ARGS)
        dec.ss_prob = 0
        with pytest.raises(NotImplementedError, match=r"(?s)%s.*rollout" % attr):
            dec.rollout(DEC_ARGS[0])
    model.decoder.dropout_p = 0.5
    with pytest.raises(NotImplementedError, match=r"(?s)dropout_p.*rollout"):
        model.scst_forward(torch.zeros(2, 3, 32, 32), [0, 1], None)
    m.dropout_p, m.ss_prob = 0.5, 0.25
    with pytest.raises(NotImplementedError, match=r"(?s)dropout_p.*ss_prob"):
        m.decode(*ATT_ARGS)
    with pytest.raises(NotImplementedError, match=r"(?s)dropout_p.*ss_prob"):
        m(torch.zeros(2, 3, 16, 16), ATT_ARGS[2], ATT_ARGS[3])
    m.ss_prob = 0
    with pytest.raises(NotImplementedError, match=r"(?s)dropout_p.*rollout"):
        m.rollout(ATT_ARGS[0], ATT_ARGS[1])
    with pytest.raises(NotImplementedError, match=r"(?s)dropout_p.*rollout"):
        m.scst_forward(torch.zeros(2, 3, 16, 16), [0, 1], None)
    assert torch.equal(torch.get_rng_state(), state)
    # lstm_dropout_p has nothing to act on with one layer: it is ignored, scheduled sampling stays available
    one.lstm_dropout_p, one.ss_prob = 0.5, 0.25
    assert one.dropout_plan(sampling=True) is None
    # eval mode never drops, so nothing is refused there either
    dec.eval()
    dec.dropout_p, dec.ss_prob = 0.5, 0.25
    assert dec.dropout_plan(sampling=True) is None
    m.eval()
    assert m.dropout_plan(sampling=True) is None
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [0x0123456789ABCDEF, 7])
def test_reference_mask_keeps_one_minus_p(p, seed):
    n = 1 << 16
    kept = DR.keep(seed, 0, 0, 1, n, p).mean()
    assert abs(kept - (1 - p)) < 4 * math.sqrt(p * (1 - p) / n), kept


def test_sites_and_ranks_have_masks_of_their_own_and_p_zero_keeps_everything():
    seed = 0xFEDCBA9876543210
    base = DR.keep(seed, 0, 1, 8, 512, 0.5)
    for other in (DR.keep(seed, 0, 2, 8, 512, 0.5), DR.keep(seed, 1, 1, 8, 512, 0.5), DR.keep(seed + 1, 0, 1, 8, 512, 0.5)):
        agree = (base == other).mean()
        assert 0.4 < agree < 0.6, agree                 # independent fair coins agree half the time (4096 of them: 0.5 +- 0.03 is 4 sd)
    assert DR.keep(seed, 0, 1, 8, 512, 0.0).all() and DR.scale(0.0) == np.float32(1) and DR.threshold(0.0) == 0
    x = np.random.default_rng(0).standard_normal((8, 512)).astype(np.float32)
    assert np.array_equal(DR.apply(x, 0.0, seed, 0, 1).view(np.uint32), x.view(np.uint32))
    assert DR.threshold(2.0 ** -24) == 1 and DR.threshold(0.5) == 1 << 23 and DR.scale(0.5) == np.float32(2)
    top = float(np.nextafter(np.float32(1), np.float32(0)))
    assert DR.threshold(top) == (1 << 24) - 1 and DR.scale(top) == np.float32(2.0 ** 24)
    # the counter's third word carries the high bit no token draw sets (their word is the step index): rebuilt here from Philox
    import ss_reference as R
    k0, k1 = R.seed_key(seed)
    w = R.philox4x32_10(np.uint32(3 >> 2), np.uint32(5), np.uint32(0x80000000 | 1), np.uint32(0), k0, k1)[3]
    assert bool(DR.keep(seed, 0, 1, 6, 4, 0.5)[5, 3]) == bool((int(w) >> 8) >= (1 << 23))


def test_references_with_all_ones_masks_are_the_oracles():
    """the two float64 references of the GPU tests, fed masks of ones, are the project's oracles (which the goldens pin)"""
    from oracle import attend as OA
    from oracle import decoder as OD
    from oracle import train_step as OT
    g = torch.Generator().manual_seed(5)
    E, H, V, Lh = 12, 20, 37, 2
    params = OD.init_decoder_params(E, H, V, Lh, generator=g)
    lengths = [7, 5, 5, 3, 2]
    caps = torch.randint(4, V, (5, 7), generator=g)
    feats = torch.randn(5, E, generator=g)
    loss, grads, d_feat, logits = OT.decoder_loss_and_grads(params, feats, caps, lengths, Lh)
    targets, l1 = OT.pack_targets(caps, lengths)
    N = sum(l1)
    ref = DR.decoder_loss_and_grads(params, feats, caps[:, :-1], l1, targets, Lh, {1: torch.ones(N, H, dtype=torch.float64),
                                                                                 2: torch.ones(N, H, dtype=torch.float64)})
    assert abs(ref["loss"].item() - loss.item()) < 1e-5
    np.testing.assert_allclose(ref["logits"].numpy(), logits.numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(ref["d_features"].numpy(), d_feat.numpy(), rtol=1e-3, atol=1e-7)
    for k in params:
        np.testing.assert_allclose(ref["grads"][k].numpy(), grads[k].numpy(), rtol=1e-3, atol=1e-7, err_msg=k)
    hidden, context, vocab, embed, P = 20, 8, 29, 12, 6
    ap = {k: v.double() for k, v in OA.init_attend_params(hidden, context, vocab, embed, generator=g, feat=context).items()}
    af = torch.randn(4, P, context, generator=g).double()
    acaps = torch.randint(0, vocab, (4, 6), generator=g)
    al = [6, 4, 4, 2]
    loss64, g64, logits64 = OA.attend_loss_and_grads(ap, af, acaps, al)
    at = OD.pack_time_major(acaps[:, 1:], [l - 1 for l in al])
    aref = DR.attend_loss_and_grads(ap, af, acaps[:, :-1], [l - 1 for l in al], at, torch.ones(at.numel(), embed, dtype=torch.float64))
    assert abs(aref["loss"].item() - loss64.item()) < 1e-12
    for k in ap:
        np.testing.assert_allclose(aref["grads"][k].numpy(), g64[k].numpy(), rtol=1e-9, atol=1e-12, err_msg=k)
