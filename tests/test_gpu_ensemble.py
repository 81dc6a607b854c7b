"""GPU: the ensemble decode -- sat_ensemble_logprobs (ensemble_logprobs_kernel), sat_beam_decode_ensemble and `sat.Ensemble` --
against the plain references of tests/ensemble_reference.py.

Combine kernel.  Inputs are the planted rows of the beam step tests (background in [-1, 1), plants 0.25 apart from 2.0 up), one
matrix per member; the result is compared with the f64 combine at the step tests' ATOL = 1e-5 on the same input construction, the
measured maximum printed.  Both row paths run: ldl == ldo == pad4(V) on 16-byte aligned bases takes the 16-byte path, an odd ldl
or ldo the scalar path.  Input pad columns hold NaN (nobody reads them), output pad columns +inf (nobody writes them).

Combine into the selection.  "Consensus" cases: every member alone prefers its own column, the ensemble the shared runner-up;
asserted on the f64 reference before the device runs, with the f64 keys more than MARGIN = 1e-3 apart, so parents and tokens are
compared exactly and scores to 1e-5.

Whole decodes.  The cases of tests/ensemble_reference.py, whose seeds are searched against the CPU restatement only; ids are compared
exactly and scores to 1e-4 on the images whose smallest key gap exceeds 2e-4.  tests/test_ensemble_host.py asserts, without a GPU,
that this leaves out at most a quarter of the images of every case."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import beam_constraints_reference as BC
import beam_groups_reference as BG
import beam_reference as R
import ensemble_reference as ER

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib
Ensemble, SatDecoderModel = sat.Ensemble, L.SatDecoderModel      # (a tree without the feature fails here)
ARG, UNSUPPORTED, WORKSPACE = 1001, 1003, 1002
MARGIN, ATOL = 1e-3, 1e-5
DECODE_ATOL = 1e-4
END = ER.END
LAM = 0.6
pad4 = ER.pad4


def device_combine(xs, ldl, ldo, weights, mode, expect=0, M=None, offset=0, null=None):
    """sat_ensemble_logprobs on the device.  xs: M arrays [R, V]; the input pad columns are NaN, `out` is filled with +inf.
    offset: floats by which every base is shifted off its 16-byte alignment.  -> out [R, ldo] (numpy), pad columns included"""
    lib = L.load()
    R_, V = xs[0].shape
    bufs = []
    for x in xs:
        buf = np.full((R_ * max(ldl, V) + offset,), np.nan, dtype=np.float32)
        if ldl >= V:                                               # (a smaller ldl is refused: the buffer is never read)
            buf[offset:].reshape(R_, ldl)[:, :V] = x
        bufs.append(torch.from_numpy(buf).cuda())
    out = torch.full((R_ * max(ldo, V) + offset,), float("inf"), device="cuda")
    M = len(xs) if M is None else M
    ptrs = (C.c_void_p * max(len(xs), 1))(*[b.data_ptr() + 4 * offset for b in bufs])
    if null == "member":
        ptrs[len(xs) - 1] = None
    w = None if weights is None else (C.c_float * len(weights))(*weights)
    rc = lib.sat_ensemble_logprobs(None if null == "table" else ptrs, M, ldl, w, mode, R_, V,
                                   None if null == "out" else out.data_ptr() + 4 * offset, ldo, L.stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    if expect:
        assert torch.isposinf(out).all()                           # an error leaves `out` untouched
        return None
    got = out.cpu().numpy()[offset:].reshape(R_, ldo)
    assert np.isposinf(got[:, V:]).all()                           # columns V .. ldo-1 are not written
    return got


def check_combine(got, ref, tag):
    V = ref.shape[1]
    fin = np.isfinite(ref)
    assert np.array_equal(np.isneginf(got[:, :V]), np.isneginf(ref)) and not np.isnan(got[:, :V]).any(), tag
    return float(np.abs(got[:, :V][fin].astype(np.float64) - ref[fin]).max())


def lds(V):
    return sorted({V, pad4(V)})


# ---- the combine kernel against f64 ----
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("V", [3, 203, 1000, 12292])
def test_combine_against_f64(V, M):
    worst = 0.0
    for R_ in (1, 10, 40):
        xs = [ER.planted_rows(V, R_, 100 * m + R_) for m in range(M)]
        for weights in (None, [1.0 + 0.75 * m for m in range(M)]):
            for mode in (0, 1):
                ref = ER.combine_ref(xs, weights, mode)
                for ldl in lds(V):
                    for ldo in lds(V):
                        err = check_combine(device_combine(xs, ldl, ldo, weights, mode), ref, (V, M, R_, mode, ldl, ldo))
                        worst = max(worst, err)
                        assert err <= ATOL, (V, M, R_, weights, mode, ldl, ldo, err)
    print("combine V %d M %d: max error %.3g (atol %.0e)" % (V, M, worst, ATOL))


@pytest.mark.parametrize("V", [203, 1000])
def test_alignment_selects_a_path_and_never_a_value(V):
    """the 16-byte path (aligned bases, ldl % 4 == 0) and the scalar path (bases one float off; odd leading dimensions) give the
    same bits"""
    xs = [ER.planted_rows(V, 10, 7 + m) for m in range(3)]
    for mode in (0, 1):
        a = device_combine(xs, pad4(V), pad4(V), [1.0, 2.0, 3.0], mode)[:, :V]
        b = device_combine(xs, pad4(V), pad4(V), [1.0, 2.0, 3.0], mode, offset=1)[:, :V]
        c = device_combine(xs, V + 1, V + 3, [1.0, 2.0, 3.0], mode)[:, :V]
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), c.view(np.int32))


def test_one_member_in_prob_mode_is_log_softmax_and_the_step_kernels_subtract_nothing():
    x = ER.planted_rows(1000, 10, 5)
    out = device_combine([x], 1000, 1000, None, 0)
    assert np.abs(out - R.log_softmax64(x)).max() <= ATOL
    assert np.abs(ER.lse64(out)).max() <= ATOL                     # in mode 0 the combined row is normalised: its lse is 0


@pytest.mark.parametrize("V", [11, 203])
def test_minus_inf_columns_follow_the_rule_of_each_mode(V):
    xs = [ER.planted_rows(V, 10, 30 + m) for m in range(3)]
    xs[1][:, 4] = -np.inf                                           # one member only
    xs[2][3, 0] = -np.inf
    for x in xs:
        x[:, 7] = -np.inf                                           # every member
        x[5, V - 1] = -np.inf                                       # ... in the V % 4 tail
    for mode in (0, 1):
        ref = ER.combine_ref(xs, [1.0, 2.0, 4.0], mode)
        assert np.isneginf(ref[:, 7]).all() and np.isneginf(ref[:, 4]).all() == (mode == 1)
        for ld in lds(V):
            assert check_combine(device_combine(xs, ld, ld, [1.0, 2.0, 4.0], mode), ref, (V, mode, ld)) <= ATOL


def test_combine_argument_errors_leave_out_untouched():
    xs = [ER.planted_rows(12, 4, m) for m in range(2)]
    device_combine(xs, 12, 12, None, 0)
    for kw in (dict(null="table"), dict(null="member"), dict(null="out"), dict(M=0), dict(M=9), dict(M=-1)):
        device_combine(xs, 12, 12, None, 0, expect=ARG, **kw)
    for mode in (-1, 2):
        device_combine(xs, 12, 12, None, mode, expect=ARG)
    device_combine(xs, 11, 12, None, 0, expect=ARG)                 # ldl < V
    device_combine(xs, 12, 11, None, 0, expect=ARG)                 # ldo < V
    for bad in ([1.0, 0.0], [1.0, -1.0], [float("nan"), 1.0], [1.0, float("inf")]):
        device_combine(xs, 12, 12, bad, 0, expect=ARG)
    lib = L.load()
    buf = torch.full((4, 12), float("inf"), device="cuda")
    ptrs = (C.c_void_p * 2)(buf.data_ptr(), buf.data_ptr())
    for R_, V in ((0, 12), (4, 0), (-1, 12)):
        assert lib.sat_ensemble_logprobs(ptrs, 2, 12, None, 0, R_, V, buf.data_ptr(), 12, L.stream()) == ARG
    assert lib.sat_ensemble_logprobs(ptrs, 2, 12, None, 0, 4, 12, buf.data_ptr(), 12, L.stream()) == ARG      # out aliases an input
    torch.cuda.synchronize()
    assert torch.isposinf(buf).all()


# ---- the combine in front of the selection kernels ----
def gap_of(cand, K):
    """the smallest distance between consecutive finite candidates among the best K + 1, per image"""
    gaps = []
    for row in cand:
        top = -np.sort(-row)[:K + 1]
        top = top[np.isfinite(top)]
        gaps.append((top[:-1] - top[1:]).min() if top.size > 1 else np.inf)
    return np.array(gaps)


def consensus_case(M, B, K, V, mode, G):
    """the first seed at which the f64 keys of every image lie more than MARGIN apart"""
    for seed in range(200):
        rng = np.random.default_rng(seed)
        xs, own, shared = ER.consensus_rows(M, B * K, V, rng, extra=K)
        scores = ER.bases(B, K)
        out = ER.combine_ref(xs, None, mode)
        if G > 1:
            ref = BG.step_ref(out, scores, None, -1, K, G, LAM)
            gap = ref["gap"]
        else:
            ref = R.beam_step_ref(out, scores, None, -1, K)
            gap = gap_of(ref["cand"], K)
        if (gap > MARGIN).all():
            return xs, scores, ref, gap
    raise AssertionError("no well-formed consensus case below seed 200")


def device_combine_and_step(xs, scores, K, mode, G):
    lib = L.load()
    R_, V = xs[0].shape
    B, ldl = R_ // K, pad4(V)
    bufs = []
    for x in xs:
        buf = np.zeros((R_, ldl), dtype=np.float32)
        buf[:, :V] = x
        bufs.append(torch.from_numpy(buf).cuda())
    comb = torch.zeros(R_, ldl, device="cuda")
    ptrs = (C.c_void_p * len(xs))(*[b.data_ptr() for b in bufs])
    L.check(lib.sat_ensemble_logprobs(ptrs, len(xs), ldl, None, mode, R_, V, comb.data_ptr(), ldl, L.stream()), "sat_ensemble_logprobs")
    sc = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)).cuda()
    parent = torch.full((R_,), -7, dtype=torch.int32, device="cuda")
    token = torch.full((R_,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((R_,), float("nan"), device="cuda")
    ws = torch.empty(max(lib.sat_beam_step_groups_ws_bytes(B, K, V, 20), 64), dtype=torch.uint8, device="cuda")
    if G > 1:
        L.check(lib.sat_beam_step_groups(comb.data_ptr(), ldl, sc.data_ptr(), None, -1, B, K, V, None, None, None, 0, 20, G, LAM,
                                         parent.data_ptr(), token.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()),
                "sat_beam_step_groups")
    else:
        L.check(lib.sat_beam_step(comb.data_ptr(), ldl, sc.data_ptr(), None, -1, B, K, V, parent.data_ptr(), token.data_ptr(),
                                  out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "sat_beam_step")
    torch.cuda.synchronize()
    return parent.cpu().numpy().astype(np.int64).reshape(B, K), token.cpu().numpy().reshape(B, K), out.cpu().numpy().reshape(B, K)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("V", [203, 1000])
def test_consensus_through_the_selection_kernels(V, mode, G):
    """sat_ensemble_logprobs into sat_beam_step (G 1) and into sat_beam_step_groups with (K, G) = (4, 2)"""
    M, B, K = 3, 3, 4
    xs, scores, ref, gap = consensus_case(M, B, K, V, mode, G)
    # before the device runs: in every image the ensemble's winners are not those of any member alone
    for x in xs:
        own = BG.step_ref(x, scores, None, -1, K, G, LAM) if G > 1 else R.beam_step_ref(x, scores, None, -1, K)
        for b in range(B):
            assert (own["parent"][b].tolist(), own["token"][b].tolist()) != (ref["parent"][b].tolist(), ref["token"][b].tolist())
    parent, token, out = device_combine_and_step(xs, scores, K, mode, G)
    assert parent.tolist() == ref["parent"].tolist() and token.tolist() == ref["token"].tolist()
    err = np.abs(out.astype(np.float64) - ref["scores"]).max()
    print("consensus V %d mode %d G %d: score error %.3g (atol %.0e), smallest key gap %.3g" % (V, mode, G, err, ATOL, gap.min()))
    assert err <= ATOL


# ---- sat_beam_decode_ensemble and Ensemble.sample_beam_features ----
def decoder_of(p, Lh):
    V, E = p["embed.weight"].shape
    dec = sat.DecoderRNN(E, p["lstm.weight_hh_l0"].shape[1], V, Lh)
    dec.load_state_dict(p)
    return dec.cuda().eval()


@functools.lru_cache(maxsize=None)
def decoder_case(kind):
    w = ER.decoder_case(kind)
    made = {}
    decs = []
    for p, Lh in w["members"]:                                      # ("copies": the same object three times)
        if id(p) not in made:
            made[id(p)] = decoder_of(p, Lh)
        decs.append(made[id(p)])
    w["decs"], w["cuda"] = decs, [f.cuda() for f in w["feats"]]
    w["ens"] = sat.Ensemble(decs, None, "logprob" if w["mode"] else "prob")
    return w


def search_order(ids, scores, order):
    """the public (re-ranked) result taken back to search order: slot order[b, r] held what is now at rank r"""
    o = order.long()
    ids_s, sc_s = torch.empty_like(ids), torch.empty_like(scores)
    ids_s.scatter_(1, o[:, :, None].expand_as(ids), ids)
    sc_s.scatter_(1, o, scores)
    return ids_s, sc_s


def check_decode(ids, scores, ref, tag):
    keep = (ref["gap"] > ER.GAP).numpy()
    assert keep.sum() * 4 >= 3 * len(keep)                          # (tests/test_ensemble_host.py asserts it on the CPU)
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    assert ids.shape == tuple(ref["ids"].shape)
    assert np.array_equal(ids[keep], ref["ids"].numpy()[keep]), tag
    want = ref["scores"].numpy()[keep]
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(scores[keep]), fin)
    err = np.abs(scores[keep][fin] - want[fin]).max()
    print("%s: %d of %d images left out, score error %.3g (atol %.0e)" % (tag, int((~keep).sum()), len(keep), err, DECODE_ATOL))
    assert err <= DECODE_ATOL
    return keep


@pytest.mark.parametrize("kind", ["plain", "logprob"])
def test_two_members_of_different_shape_match_the_restatement(kind):
    """(E 32, H 64, 1 layer) and (E 48, H 96, 2 layers), V 203, B 5, K 4, with end_id"""
    w = decoder_case(kind)
    ens = w["ens"]
    ids, scores = ens.sample_beam_features(w["cuda"], w["K"], END, return_all=True)
    assert ens.last_beam_order is None and ens.last_beam_norm_scores is None and ens.last_beam_groups is None
    check_decode(ids, scores, w["ref"], kind)
    assert torch.equal(ens.sample_beam_features(w["cuda"], w["K"], END), ids[:, 0])
    for dec, f in zip(w["decs"], w["cuda"]):                        # no member alone decodes what the ensemble decodes
        assert (dec.sample_beam(f, w["K"], END, return_all=True)[0] != ids).any()


@pytest.mark.parametrize("kind", ["wide", "wide_x3"])
def test_wide_members_match_the_restatement(kind):
    """B 32, so R = 128: a one-layer member takes the wide step (split-K gate GEMM over [x | h]).  "wide": beside a narrow two-layer
    member, V 203 (exact-f32 projection); "wide_x3": two one-layer members, V 1000 (the projection from the three-way split)"""
    w = decoder_case(kind)
    ids, scores = w["ens"].sample_beam_features(w["cuda"], w["K"], END, return_all=True)
    check_decode(ids, scores, w["ref"], kind)
    for dec, f in zip(w["decs"], w["cuda"]):
        assert (dec.sample_beam(f, w["K"], END, return_all=True)[0] != ids).any()


def test_three_copies_in_prob_mode_decode_as_the_model_itself():
    w = decoder_case("copies")
    ids, scores = w["ens"].sample_beam_features(w["cuda"], w["K"], END, return_all=True)
    keep = check_decode(ids, scores, w["ref"], "copies")
    p, Lh = w["members"][0]
    own_ref = BC.decoder_beam(p, w["feats"][0], w["K"], Lh, END, BC.Constraints())
    keep = torch.from_numpy(keep & (own_ref["gap"] > ER.GAP).numpy()).cuda()
    assert int(keep.sum()) * 4 >= 3 * ER.B_DEC
    own_ids, own_scores = w["decs"][0].sample_beam(w["cuda"][0], w["K"], END, return_all=True)
    assert torch.equal(ids[keep], own_ids[keep])
    assert (scores[keep] - own_scores[keep]).abs().max().item() <= DECODE_ATOL


def test_constrained_decode_matches_the_restatement_in_search_order():
    """no_repeat_ngram_size 2, min_length 3, length_penalty 0.7"""
    w = decoder_case("constrained")
    ens = w["ens"]
    ids, scores = ens.sample_beam_features(w["cuda"], w["K"], END, return_all=True, **w["kw"])
    order, norm = ens.last_beam_order, ens.last_beam_norm_scores
    assert order is not None and ens.last_beam_groups is None and (norm[:, :-1] >= norm[:, 1:]).all()
    ids_s, sc_s = search_order(ids, scores, order)
    keep = check_decode(ids_s, sc_s, w["ref"], "constrained")
    rr = BC.rerank_ref(ids_s.cpu().numpy(), sc_s.cpu().numpy(), END, 0.7)
    assert np.abs(norm.cpu().numpy() - rr["norm"]).max() <= DECODE_ATOL
    assert BC.check_properties(ids.cpu().numpy()[keep], END, w["c"]) == int(keep.sum()) * w["K"]


def test_grouped_decode_matches_the_restatement_in_search_order():
    """num_beam_groups 2, diversity_penalty 0.6"""
    w = decoder_case("grouped")
    ens = w["ens"]
    ids, scores = ens.sample_beam_features(w["cuda"], w["K"], END, return_all=True, **w["kw"])
    order = ens.last_beam_order
    assert torch.equal(ens.last_beam_groups, order // 2) and torch.equal(ens.last_beam_norm_scores, scores)
    ids_s, sc_s = search_order(ids, scores, order)
    check_decode(ids_s, sc_s, w["ref"], "grouped")
    ens.sample_beam_features(w["cuda"], w["K"], END)                # a plain call clears the records
    assert ens.last_beam_order is None and ens.last_beam_groups is None


def test_beam_width_one_is_the_greedy_restatement():
    w = decoder_case("greedy")
    ids = w["ens"].sample_beam_features(w["cuda"], 1, END)
    keep = (w["ref"]["gap"] > ER.GAP).numpy()
    assert keep.sum() * 4 >= 3 * len(keep)
    assert tuple(ids.shape) == (ER.B_DEC, 20) and np.array_equal(ids.cpu().numpy()[keep], w["ref"]["ids"].numpy()[keep][:, 0])


def test_one_member_returns_the_members_bits():
    w = decoder_case("plain")
    dec, f = w["decs"][1], w["cuda"][1]
    one = sat.Ensemble([dec], [3.0], "logprob")
    for kw in ({}, dict(no_repeat_ngram_size=2, length_penalty=0.7), dict(num_beam_groups=2, diversity_penalty=0.6)):
        a = one.sample_beam_features([f], 4, END, return_all=True, **kw)
        order = one.last_beam_order
        b = dec.sample_beam(f, 4, END, return_all=True, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert (order is None) == (not kw) and (order is None or torch.equal(order, dec.last_beam_order))


def test_show_and_tell_members_run_their_own_encoders():
    arch = dict(layers=(1, 1, 1, 1), width=8)
    w = decoder_case("plain")
    models = []
    for (p, Lh), dec in zip(w["members"], w["decs"]):
        m = sat.ShowAndTell(dec.embed_size, dec.hidden_size, ER.V_DEC, Lh, arch=arch, compute_dtype="f32").cuda().eval()
        m.decoder.load_state_dict(p)
        models.append(m)
    images = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    ens = sat.Ensemble(models, [2.0, 1.0])
    ids, scores = ens.sample_beam(images, 4, END, return_all=True)
    feats = [m.encoder(images) for m in models]
    want = sat.Ensemble(w["decs"], [2.0, 1.0]).sample_beam_features(feats, 4, END, return_all=True)
    assert torch.equal(ids, want[0]) and torch.equal(scores, want[1])
    greedy = ens.sample(images)
    assert tuple(greedy.shape) == (3, 20) and torch.equal(greedy, ens.sample_beam(images, 1))
    one = sat.Ensemble(models[:1])
    assert torch.equal(one.sample_beam(images, 4, END), models[0].sample_beam(images, 4, END))


def test_decode_argument_errors_come_before_anything_is_enqueued():
    lib = L.load()
    w = decoder_case("plain")
    decs, feats = w["decs"], w["cuda"]
    B, K, V = ER.B_DEC, 4, ER.V_DEC
    lstm = [d._lstm_ptrs() for d in decs]

    def structs(n=2, **over):
        arr = (L.SatDecoderModel * max(n, 1))()
        for j in range(min(n, 2)):
            d = decs[j]
            f = dict(features=feats[j].data_ptr(), embed=d.embed.weight.data_ptr(), lstm_w=C.cast(lstm[j], C.POINTER(C.c_void_p)),
                     num_layers=d.num_layers, lin_w=d.linear.weight.data_ptr(), lin_b=d.linear.bias.data_ptr(), E=d.embed_size,
                     H=d.hidden_size)
            if j == 1:
                f.update(over)
            arr[j] = L.SatDecoderModel(**f)
        return arr

    good = structs()
    wsb = lib.sat_beam_decode_ensemble_ws_bytes(good, 2, B, K, V, 20)
    assert wsb > 0
    ws, ws_ptr = L.workspace256(wsb, "cuda")
    ids = torch.full((B, K, 20), -7, dtype=torch.int64, device="cuda")

    def call(models, M=2, weights=None, mode=0, K_=K, G=1, lam=0.0, ws_bytes=wsb):
        wa = None if weights is None else (C.c_float * len(weights))(*weights)
        return lib.sat_beam_decode_ensemble(models, M, wa, mode, B, K_, V, 20, END, None, G, lam, ids.data_ptr(), None, None, None,
                                            ws_ptr, ws_bytes, L.stream())

    assert call(good, M=0) == ARG and call(good, M=9) == ARG and call(None) == ARG
    assert call(good, mode=2) == ARG and call(good, weights=[1.0, 0.0]) == ARG and call(good, weights=[1.0, float("nan")]) == ARG
    for field in ("features", "embed", "lin_w", "lin_b"):
        assert call(structs(**{field: None})) == ARG
    assert call(structs(lstm_w=C.POINTER(C.c_void_p)())) == ARG
    nine = (C.c_void_p * 36)(*([lstm[1][0]] * 36))                  # (an honest table for nine layers: the check reads 4 per layer)
    assert call(structs(E=50)) == UNSUPPORTED
    assert call(structs(num_layers=9, lstm_w=C.cast(nine, C.POINTER(C.c_void_p)))) == UNSUPPORTED
    assert call(good, G=3) == ARG and call(good, G=2, lam=-1.0) == ARG and call(good, K_=9) == ARG
    assert call(good, ws_bytes=wsb - 1) == WORKSPACE
    assert lib.sat_beam_decode_ensemble_ws_bytes(structs(E=50), 2, B, K, V, 20) == 0
    torch.cuda.synchronize()
    assert (ids == -7).all()
    assert call(good) == 0
    torch.cuda.synchronize()
    assert torch.equal(ids, sat.Ensemble(decs).sample_beam_features(feats, K, END, return_all=True)[0])


# ---- Show-Attend-Tell ----
@functools.lru_cache(maxsize=None)
def attend_case(constrained):
    w = ER.attend_case(constrained)
    hidden, context, vocab, embed, B, P, feat = w["dims"]
    models = []
    for p in w["ps"]:
        m = sat.ShowAttendTellModel(hidden, context, vocab, embed, None, feature_size=(P, feat), compute_dtype="f32", vgg_cfg=[8, "M", feat])
        m.load_state_dict(p, strict=False)
        models.append(m.cuda().eval())
    w["models"], w["cuda"] = models, [f.cuda() for f in w["feats"]]
    return w


def test_attend_members_in_lock_step_match_the_restatement():
    w = attend_case(False)
    ens = sat.Ensemble(w["models"])
    ids, scores = ens.sample_beam_features(w["cuda"], 4, END, return_all=True)
    check_decode(ids, scores, w["ref"], "attend")
    assert ens.last_beam_order is None
    for m, f in zip(w["models"], w["cuda"]):
        assert (m.sample_beam_features(f, 4, None, END, return_all=True)[0] != ids).any()
    one = sat.Ensemble(w["models"][:1])
    a, b = one.sample_beam_features(w["cuda"][:1], 4, END, return_all=True), w["models"][0].sample_beam_features(w["cuda"][0], 4, None, END,
                                                                                                                   return_all=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_attend_constrained_ensemble_matches_the_restatement():
    """no_repeat_ngram_size 2, min_length 3"""
    w = attend_case(True)
    ens = sat.Ensemble(w["models"])
    ids, scores = ens.sample_beam_features(w["cuda"], 4, END, return_all=True, **w["kw"])
    ids_s, sc_s = search_order(ids, scores, ens.last_beam_order)
    keep = check_decode(ids_s, sc_s, w["ref"], "attend constrained")
    assert BC.check_properties(ids.cpu().numpy()[keep], END, w["c"]) == int(keep.sum()) * 4
