"""GPU: consensus reranking on the device (consensus.py, csrc/sat_cider.hip) against the utilities recorded from the reference's
own `CiderScorer` (tests/golden/consensus/G13_consensus.npz) and, on random corpora, against the pure-Python restatement
(tests/consensus_reference.py).

The bound is test_gpu_cider.py's: 1e-9 absolute on values <= 10, compared in f64.  A pairwise score is fewer than 10^3 f64
operations of <= 2 ulp and a utility adds K - 1 <= 63 of them, i.e. an expected rounding of ~1e-10 at the most.  Every case prints
its maximum error."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cider_reference as R  # noqa: E402
import consensus_reference as CR  # noqa: E402
from test_consensus_host import load_case  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
TOL = 1e-9
NEAR_TIE = 1e-8
END = 2


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "consensus", "G13_consensus.npz"))


def cand_tensor(cands, T, terminate=True, junk=7):
    """cands [B][K] id lists as an int64 [B, K, T] device tensor: each row its tokens, then END (when it fits and `terminate`),
    then junk ids"""
    B, K = len(cands), len(cands[0])
    ids = torch.full((B, K, T), junk, dtype=torch.int64)
    for b, image in enumerate(cands):
        for i, c in enumerate(image):
            ids[b, i, :len(c)] = torch.tensor(c, dtype=torch.int64)
            if terminate and len(c) < T:
                ids[b, i, len(c)] = END
    return ids.cuda()


def lengths(cands):
    return torch.tensor([[len(c) for c in image] for image in cands], dtype=torch.int32).cuda()


def bits(t):
    return t.contiguous().view(torch.int64)


def compare(got, want, what):
    """got: (best, utility[, pair]) device tensors; want: the restatement's (utility, pair, best).  Returns the images whose pick
    was compared by utility because the restatement's two best utilities are closer than NEAR_TIE."""
    best, utility = got[0].cpu().numpy(), got[1].cpu().numpy()
    wu, wp, wb = np.asarray(want[0], dtype=np.float64), np.asarray(want[1], dtype=np.float64), want[2]
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float64 and utility.shape == wu.shape and best.shape == (len(wb),)
    err = np.abs(utility - wu).max()
    perr = 0.0
    if len(got) > 2:
        pair = got[2].cpu().numpy()
        assert got[2].dtype == torch.float64 and pair.shape == wp.shape
        perr = np.abs(pair - wp).max()
        diag = np.diagonal(pair, axis1=1, axis2=2)
        assert not diag.any() and not np.signbit(diag).any()                    # exactly +0.0
    near = []
    for b, u in enumerate(wu):
        top = np.sort(u)[::-1]
        if len(top) > 1 and top[0] - top[1] < NEAR_TIE:
            near.append(b)
            assert abs(utility[b][best[b]] - top[0]) <= TOL
        else:
            assert best[b] == wb[b], (what, b)
    print("%s: max |utility - want| = %.3g, max |pair - want| = %.3g, %d of %d picks compared by utility"
          % (what, err, perr, len(near), len(wu)))
    assert err <= TOL and perr <= TOL
    return near


@pytest.mark.parametrize("c", ["small", "one"])
def test_golden(golden, c):
    refs, cands = load_case(golden, c)
    rr = sat.ConsensusReranker(sat.CiderScorer(refs), end_id=END)
    T = max(len(x) for image in cands for x in image)
    ids = cand_tensor(cands, T, terminate=False)            # the small corpus's ids include 2: the lengths come through `kept`
    best, utility = rr.rerank(ids, kept=lengths(cands))
    want = golden[c + "_utility"]
    err = np.abs(utility.cpu().numpy() - want).max()
    print("golden %s: max |utility - reference| = %.3g" % (c, err))
    assert err <= TOL
    assert best.cpu().tolist() == [int(i) for i in want.argmax(1)]               # the first argmax: image 0 of `small` is a tie
    if c == "small":
        assert utility[2, 0].item() > 1.0 and utility[2, 2].item() > 1.0        # n-grams the corpus lacks still match each other
        assert torch.equal(bits(utility[0, 1]), bits(utility[0, 3]))
    else:
        assert not utility.cpu().numpy().any()


@pytest.fixture(scope="module")
def corpus():
    """(refs, df, log_images, device scorer): 30 images of 3 references over ids 3..12; 13..15 are ids the corpus lacks"""
    rng = np.random.Generator(np.random.PCG64(2025))
    refs = [[[int(t) for t in rng.integers(3, 13, rng.integers(1, 13))] for _ in range(3)] for _ in range(30)]
    df, li = CR.corpus_df(refs)
    return refs, df, li, sat.CiderScorer(refs)


def draw_cands(rng, B, K, T):
    """K variations of one base caption per image (so that n-grams of every order are shared), ids 3..15, lengths 0..T with 0, 1
    and T present where K allows; no two candidates of an image are equal unless T == 1"""
    out = []
    for b in range(B):
        base = [int(t) for t in rng.integers(3, 16, T)]
        image = []
        while len(image) < K:
            i = len(image)
            n = (T, 0, 1)[i] if b == 0 and i < 3 and K >= 4 else int(rng.integers(0, T + 1))
            c = list(base[:n])
            for p in range(len(c)):
                if rng.random() < 0.2:
                    c[p] = int(rng.integers(3, 16))
            if T > 1 and c in image:
                continue
            image.append(c)
        out.append(image)
    return out


SHAPES = [(1, 1, 20), (1, 2, 1), (3, 5, 20), (2, 8, 64), (1, 33, 20), (1, 64, 20), (64, 5, 20)]


def test_random_corpus_vs_restatement(corpus):
    """one candidate, one token, the row limit, K past 32 and at the limit, a multi-workgroup grid.  (1, 2, 1) is a tie by
    construction (one-token candidates score each other symmetrically); over the whole sweep at most 5 % of the images may be
    compared by utility instead of by index"""
    refs, df, li, scorer = corpus
    rr = sat.ConsensusReranker(scorer, end_id=END)
    near = images = 0
    for B, K, T in SHAPES:
        rng = np.random.Generator(np.random.PCG64(1000 * B + 10 * K + T))
        cands = draw_cands(rng, B, K, T)
        want = CR.batch(cands, df, li)
        got = rr.rerank(cand_tensor(cands, T), return_pairwise=True)
        near += len(compare(got, want, "B %d K %d T %d" % (B, K, T)))
        images += B
        if K > 1 and T > 1:
            assert max(max(u) for u in want[0]) > 0.5                           # not all zeros
    assert near <= 0.05 * images, (near, images)


def test_weighted(corpus):
    refs, df, li, scorer = corpus
    rr = sat.ConsensusReranker(scorer, end_id=END)
    rng = np.random.Generator(np.random.PCG64(31))
    cands = draw_cands(rng, 3, 5, 20)
    w = rng.random((3, 5))
    w[:, 1] = 0.0                                           # a column of zeros
    w[2] = [0.0, 0.0, 3.0, 0.0, 0.0]                        # image 2: all weights but candidate 2's are zero
    ids = cand_tensor(cands, 20)
    want = CR.batch(cands, df, li, weights=w.tolist())
    got = rr.rerank(ids, weights=torch.from_numpy(w).cuda(), return_pairwise=True)
    compare(got, want, "weighted")
    u, pair = got[1].cpu().numpy(), got[2].cpu().numpy()
    assert u[2][2] == 0.0 and not np.signbit(u[2][2])       # nothing but itself has weight: den == 0
    for i in (0, 1, 3, 4):
        assert abs(u[2][i] - pair[2][i][2]) <= TOL
    uni = rr.rerank(ids, return_pairwise=True)
    assert torch.equal(bits(uni[2]), bits(got[2]))          # the pairwise matrix does not depend on the weights
    ones = rr.rerank(ids, weights=torch.ones(3, 5, device="cuda"))               # f32 weights; 1 * v and K - 1 ones are exact
    assert torch.equal(bits(ones[1]), bits(uni[1])) and torch.equal(ones[0], uni[0])
    w32 = torch.from_numpy(w.astype(np.float32)).cuda()
    a, b = rr.rerank(ids, weights=w32), rr.rerank(ids, weights=w32.double())
    assert torch.equal(bits(a[1]), bits(b[1]))


def test_weighted_with_one_candidate(corpus):
    rr = sat.ConsensusReranker(corpus[3], end_id=END)
    ids = cand_tensor([[[3, 4, 5, 6]], [[7, 8]]], 20)
    for weights in (None, torch.tensor([[2.0], [0.0]], dtype=torch.float64).cuda()):
        best, utility, pair = rr.rerank(ids, weights=weights, return_pairwise=True)
        assert best.cpu().tolist() == [0, 0] and not utility.cpu().numpy().any() and not pair.cpu().numpy().any()
        assert tuple(utility.shape) == (2, 1) and tuple(pair.shape) == (2, 1, 1)
    one = rr.rerank(ids[0])                                 # [K, T]: one image
    assert tuple(one[0].shape) == (1,) and tuple(one[1].shape) == (1, 1)


def test_lengths_from_end_id_or_from_kept(corpus):
    """a row that starts with END is empty, a row without END has T tokens; both ways of giving the lengths give the same bits"""
    refs, df, li, scorer = corpus
    rr = sat.ConsensusReranker(scorer, end_id=END)
    rng = np.random.Generator(np.random.PCG64(41))
    cands = draw_cands(rng, 4, 6, 20)
    ids = cand_tensor(cands, 20)
    assert (ids[:, :, 0] == END).any() and (ids != END).all(dim=2).any()
    kept = sat.kept_tokens(ids.view(24, 20), END)
    assert kept.cpu().tolist() == [len(c) for image in cands for c in image]
    a = rr.rerank(ids, return_pairwise=True)
    compare(a, CR.batch(cands, df, li), "end_id")
    for k in (kept, kept.view(4, 6)):
        b = rr.rerank(ids, kept=k, return_pairwise=True)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_ids_that_are_no_tokens_match_nothing(corpus):
    refs, df, li, scorer = corpus
    rr = sat.ConsensusReranker(scorer, end_id=END)
    big, neg = 2 ** 31, -4
    cands = [[[big + 5] * 3, [big + 5] * 3, [neg, neg]],                        # equal rows of non-tokens: nothing matches
             [[5, big, 6, 7], [5, big, 6, 7], [5, 6, 7, neg]],                  # the tokens around them still do
             [[2 ** 31 - 1, 4, 4], [2 ** 31 - 1, 4], [2 ** 40, 4, 4]]]          # 2^31 - 1 is a token
    ids = cand_tensor(cands, 6, terminate=False)
    want = CR.batch(cands, df, li)
    got = rr.rerank(ids, kept=lengths(cands), return_pairwise=True)
    compare(got, want, "non-tokens")
    u = got[1].cpu().numpy()
    assert not u[0].any() and u[1].min() > 0.1 and u[2][0] > 0.1
    assert got[2][1, 0, 1].item() < 9.0                     # equal rows, but the non-token breaks every n-gram through it


def test_a_strided_view_gives_the_bits_of_its_contiguous_copy(corpus):
    rr = sat.ConsensusReranker(corpus[3], end_id=END)
    rng = np.random.Generator(np.random.PCG64(51))
    buf = torch.from_numpy(rng.integers(2, 16, (3, 9, 31))).cuda()
    view = buf[:, :6, :20]
    assert not view.is_contiguous()
    a, b = rr.rerank(view, return_pairwise=True), rr.rerank(view.contiguous(), return_pairwise=True)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    one = rr.rerank(buf[1, 2:8, 5:25], return_pairwise=True)                     # [K, T] out of the middle
    again = rr.rerank(buf[1:2, 2:8, 5:25].contiguous(), return_pairwise=True)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(one, again)) and a[1].cpu().numpy().max() > 0


def test_same_bits_twice_and_for_an_image_alone(corpus):
    rr = sat.ConsensusReranker(corpus[3], end_id=END)
    cands = draw_cands(np.random.Generator(np.random.PCG64(61)), 8, 7, 20)
    ids = cand_tensor(cands, 20)
    w = torch.from_numpy(np.random.Generator(np.random.PCG64(62)).random((8, 7))).cuda()
    for weights in (None, w):
        a = rr.rerank(ids, weights=weights, return_pairwise=True)
        b = rr.rerank(ids, weights=weights, return_pairwise=True)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
        for img in (0, 5, 7):
            alone = rr.rerank(ids[img:img + 1], weights=None if weights is None else weights[img:img + 1], return_pairwise=True)
            assert all(torch.equal(bits(x), bits(y[img:img + 1])) for x, y in zip(alone, a))


def test_limits_and_a_short_workspace_return_errors_and_enqueue_nothing(corpus):
    scorer = corpus[3]
    lib = L.load()
    ids = torch.full((1, 65, 65), 5, dtype=torch.int64, device="cuda")
    utility = torch.full((65,), -7.0, dtype=torch.float64, device="cuda")
    best = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(lib.sat_consensus_ws_bytes(1, 65), dtype=torch.uint8, device="cuda")

    def call(K, T, ws_bytes):
        return lib.sat_consensus_rerank(C.byref(scorer._corpus), ids.data_ptr(), 65 * 65, 65, 1, K, T, None, END, 6.0, None,
                                        utility.data_ptr(), best.data_ptr(), None, ws.data_ptr(), ws_bytes, L.stream())
    assert ws.data_ptr() % 8 == 0
    assert call(65, 20, ws.numel()) == L.SAT_ERR_UNSUPPORTED
    assert call(5, 65, ws.numel()) == L.SAT_ERR_UNSUPPORTED
    assert call(5, 20, lib.sat_consensus_ws_bytes(1, 5) - 1) == L.SAT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (utility == -7.0).all() and best.item() == -7 and not ws.any()       # nothing ran
    assert call(5, 20, lib.sat_consensus_ws_bytes(1, 5)) == L.SAT_OK
    torch.cuda.synchronize()
    assert (utility[:5] != -7.0).all() and (utility[5:] == -7.0).all() and best.item() == 0


def want_pick(rr, df, li):
    """the restatement on the reranker's last candidates, read back"""
    rows = [[R.truncate(c, END) for c in image] for image in rr.last_ids.cpu().tolist()]
    assert [[len(c) for c in image] for image in rows] == rr.last_kept.cpu().tolist()
    want = CR.batch(rows, df, li)
    print("utilities of image 0:", ["%.4f" % u for u in want[0][0]], "picks", want[2])
    assert max(max(u) for u in want[0]) > 0.0               # the candidates share something: the comparison is not of zeros
    return want


def test_end_to_end_on_a_tiny_model():
    from oracle import decoder as OD
    from oracle import encoder as OE
    tiny = dict(layers=(1, 1, 1, 1), width=8)
    E, H, V, Lh, B, T = 32, 64, 200, 1, 4, 10
    gen = torch.Generator().manual_seed(1)
    ep, eb = OE.init_encoder_params(E, tiny, generator=gen, randomize_bn=True)
    dp = OD.init_decoder_params(E, H, V, Lh, generator=gen)
    model = sat.ShowAndTell(E, H, V, Lh, arch=tiny, compute_dtype="f32")
    model.encoder.load_state_dict({**ep, **eb})
    model.decoder.load_state_dict(dp)
    model.cuda().eval()
    images = torch.randn(B, 3, 64, 64, generator=gen).cuda()
    caps = torch.randint(4, V, (B, T), generator=gen)
    caps[:, 0], caps[:, -1] = 1, 2
    caps = caps.cuda()
    rng = np.random.Generator(np.random.PCG64(71))
    refs = [[[int(t) for t in rng.integers(3, V, rng.integers(3, 12))] for _ in range(2)] for _ in range(25)]
    df, li = CR.corpus_df(refs)
    rr = sat.ConsensusReranker(sat.CiderScorer(refs), end_id=END)

    picked = rr.decode(model, images, beam_size=4, num_beam_groups=2, diversity_penalty=0.5)
    assert tuple(rr.last_ids.shape) == (B, 4, 20) and tuple(rr.last_scores.shape) == (B, 4) and tuple(picked.shape) == (B, 20)
    compare((rr.last_best, rr.last_utility), want_pick(rr, df, li), "decode, 2 groups of 2")
    chosen = rr.last_best.cpu().tolist()
    assert picked.cpu().tolist() == [rr.last_ids[b, chosen[b]].cpu().tolist() for b in range(B)]
    weighted = rr.decode(model, images, beam_size=4, weights="scores")
    rows = [[R.truncate(c, END) for c in image] for image in rr.last_ids.cpu().tolist()]
    w = torch.softmax(rr.last_scores.double(), 1).cpu().tolist()
    compare((rr.last_best, rr.last_utility), CR.batch(rows, df, li, weights=w), 'decode, weights="scores"')
    assert tuple(weighted.shape) == (B, 20)

    picked = rr.decode_samples(model, images, num_samples=6, seed=1234, temperature=0.7)
    assert tuple(rr.last_ids.shape) == (B, 6, 20) and rr.last_scores is None and tuple(picked.shape) == (B, 20)
    compare((rr.last_best, rr.last_utility), want_pick(rr, df, li), "decode_samples, 6 draws")
    chosen = rr.last_best.cpu().tolist()
    assert picked.cpu().tolist() == [rr.last_ids[b, chosen[b]].cpu().tolist() for b in range(B)]

    lens = [T] * B
    plain = sat.validation_step(model, images, caps, lens, end_id=END, beam_size=4)
    assert sorted(plain) == ["ids", "kept", "loss"]
    assert torch.equal(plain["ids"], model.sample_beam(images, beam_size=4, end_id=END))       # what it returns today
    out = sat.validation_step(model, images, caps, lens, end_id=END, beam_size=4, consensus=rr)
    assert sorted(out) == ["consensus_best", "consensus_utility", "ids", "kept", "loss"]
    compare((out["consensus_best"], out["consensus_utility"]), want_pick(rr, df, li), "validation_step")
    assert torch.equal(rr.last_ids[:, 0], plain["ids"]) and torch.equal(out["loss"], plain["loss"])
    assert torch.equal(out["ids"], rr.select(rr.last_ids, out["consensus_best"]))
    assert torch.equal(out["ids"], rr.decode(model, images, beam_size=4))
    assert torch.equal(out["kept"], sat.kept_tokens(out["ids"], END))
