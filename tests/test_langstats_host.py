"""CPU: the host side of BLEU-1..4 and ROUGE-L on the device (langstats.py, csrc/sat_langstats.hip).  The pure-Python restatement
(tests/bleu_rouge_reference.py) matches what was recorded from the reference's own `BleuScorer` and `Rouge`
(tests/golden/make_goldens_bleu_rouge.py): integers equal, floats within 1e-12; the fixture holds the edge cases it is for and
regenerates; the three symbols are declared, bound and exported by both builds of the library and reject bad arguments without
a launch; `BleuScorer`, `RougeLScorer`, `MixedReward` and `validation_step` validate before they touch the GPU."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bleu_rouge_reference as R  # noqa: E402
from test_cider_host import load_corpus  # noqa: E402

sat = importlib.import_module("show-and-tell_amd")
langstats = importlib.import_module("show-and-tell_amd.langstats")
L = sat._lib
NAMES = ("sat_bleu_comps", "sat_bleu_finalize", "sat_rouge_l_score")
CORPORA = ("small", "wide", "one", "edges")
# every value is <= 1 and fewer than 40 f64 operations from integers; the restatement does the reference's operations in the
# reference's order with the same `math` library, so in practice it does not differ at all
TOL = 1e-12


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "langstats", "G12_bleu_rouge.npz"))


@pytest.mark.parametrize("c", CORPORA)
def test_restatement_matches_the_reference(golden, c):
    refs, hyps = load_corpus(golden, c)
    idx = range(len(refs))
    comps, sentence, totals, corpus = R.bleu(hyps, refs, idx)
    assert np.array_equal(np.asarray(comps, dtype=np.int64), golden[c + "_comps"])
    assert totals == golden[c + "_comps"].sum(axis=0).tolist()
    e_s = np.abs(np.asarray(sentence).T - golden[c + "_bleu_list"]).max()
    e_c = np.abs(np.asarray(corpus) - golden[c + "_bleus"]).max()
    lcs = [l for h, i in zip(hyps, idx) for l in R.rouge_l_one(h, refs[i])[1]]
    assert lcs == golden[c + "_lcs"].tolist()
    mean, scores = R.rouge_l(hyps, refs, idx)
    e_r = np.abs(np.asarray(scores) - golden[c + "_rouge_scores"]).max()
    e_m = abs(mean - float(golden[c + "_rouge_mean"]))
    print(c, "max |restatement - reference|: bleu_list %.3g, bleus %.3g, rouge %.3g, rouge mean %.3g" % (e_s, e_c, e_r, e_m))
    assert max(e_s, e_c, e_r, e_m) <= TOL


def _clip_sources(hyp, refs):
    """order -> set of the references that alone hold the maximum count of some n-gram of that order that the row has too"""
    out = {}
    for g, c in R.precook(hyp)[1].items():
        counts = [R.precook(r)[1].get(g, 0) for r in refs]
        if max(counts) > 0 and counts.count(max(counts)) == 1:
            out.setdefault(len(g), set()).add(counts.index(max(counts)))
    return out


def _longest_common_run(a, b):
    return max([k for k in range(1, len(a) + 1) for i in range(len(a) - k + 1)
                if any(a[i:i + k] == b[j:j + k] for j in range(len(b) - k + 1))] or [0])


def test_fixture_has_the_cases_it_is_for(golden):
    refs, hyps = load_corpus(golden, "edges")
    comps, rouge = golden["edges_comps"], golden["edges_rouge_scores"]
    has = dict.fromkeys(("tie", "orders", "longer", "shorter", "equal", "empty_hyp", "empty_both", "empty_ref", "hyp64", "ref128",
                         "absent", "gapped"), False)
    for i, (image, h) in enumerate(zip(refs, hyps)):
        lens = [len(r) for r in image]
        near = sorted(lens, key=lambda l: (abs(l - len(h)), l))
        if len(near) > 1 and abs(near[0] - len(h)) == abs(near[1] - len(h)) and near[0] < near[1]:
            has["tie"] |= comps[i, 1] == near[0] and lens.index(near[0]) > lens.index(near[1])     # the shorter one, listed second
        src = _clip_sources(h, image)
        has["orders"] |= any(x != y for a in src for b in src if a < b for x in src[a] for y in src[b]) and len(image) == 2
        has["longer"] |= len(h) > max(lens)
        has["shorter"] |= 0 < len(h) < min(lens)
        has["equal"] |= len(h) > 0 and h in image and rouge[i] == 1.0
        has["empty_hyp"] |= h == [] and [] not in image and rouge[i] == 0.0 and not golden["edges_bleu_list"][:, i].any()
        has["empty_both"] |= h == [] and [] in image and rouge[i] == 1.0
        has["empty_ref"] |= h != [] and [] in image and 0.0 < rouge[i] < 1.0
        has["hyp64"] |= len(h) == 64
        has["ref128"] |= max(lens) == 128 and len(h) > 0
        has["absent"] |= len(h) > 0 and not set(h) & {t for r in image for t in r} and rouge[i] == 0.0 and not comps[i, 6:].any()
        has["gapped"] |= any(R.lcs(r, h) > max(_longest_common_run(h, r), 1) for r in image)
    assert all(has.values()), has
    assert max(len(h) for h in hyps) == 64 and max(len(r) for image in refs for r in image) == 128
    assert comps[:, 0].tolist() == [len(h) for h in hyps]


def _reference_tree():
    from oracle.build_ref import reference_checkout
    path = reference_checkout()
    try:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            import lib2to3  # noqa: F401
    except ImportError:
        return False
    return bool(path) and all(os.path.exists(os.path.join(path, "pycocoevalcap", *p))
                              for p in (("bleu", "bleu_scorer.py"), ("rouge", "rouge.py")))


@pytest.mark.skipif(not _reference_tree(), reason="the reference checkout or lib2to3 is not on this machine")
def test_fixture_regenerates_from_the_reference(golden, golden_dir, tmp_path):
    subprocess.check_call([sys.executable, os.path.join(golden_dir, "make_goldens_bleu_rouge.py"), str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    new = np.load(os.path.join(str(tmp_path), "G12_bleu_rouge.npz"))
    assert sorted(new.files) == sorted(golden.files)
    for k in golden.files:
        assert new[k].dtype == golden[k].dtype and np.array_equal(new[k], golden[k]), k


def test_symbols_are_declared_bound_and_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    hooks = L.open_library(os.path.join(ROOT, "tests", "_build", "libsat_hip_testhooks.so"))
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr)
        assert name in L.SIGNATURES and name in L.ADDED_WITHIN_ABI
        for lib in (L.load(), hooks):
            assert hasattr(lib, name)
    assert "typedef struct sat_ref_corpus {" in hdr and C.sizeof(L.SatRefCorpus) == 48
    assert L.load().sat_version() == hooks.sat_version() == L.ABI_VERSION == 18
    assert sat.BleuScorer is langstats.BleuScorer and sat.RougeLScorer is langstats.RougeLScorer
    assert sat.MixedReward is langstats.MixedReward


P = 0x1000          # a non-null pointer that is never dereferenced: every call below is rejected before anything is enqueued


def corpus(**kw):
    a = dict(ref_tokens=P, ref_offsets=P, image_offsets=P, n_tokens=9, n_refs=3, n_images=2, max_ref_tokens=5)
    a.update(kw)
    return L.SatRefCorpus(**a)


def bleu_call(c=None, **kw):
    a = dict(ids=P, stride=20, B=4, T=20, kept=None, end_id=2, image_index=P, comps=P, sentence=P, mean=None, totals=None)
    a.update(kw)
    c = corpus() if c is None else c
    return L.load().sat_bleu_comps(C.byref(c) if c else None, a["ids"], a["stride"], a["B"], a["T"], a["kept"], a["end_id"],
                                   a["image_index"], a["comps"], a["sentence"], a["mean"], a["totals"], None)


def rouge_call(c=None, **kw):
    a = dict(ids=P, stride=20, B=4, T=20, kept=None, end_id=2, image_index=P, beta=1.2, scores=P, mean=P)
    a.update(kw)
    c = corpus() if c is None else c
    return L.load().sat_rouge_l_score(C.byref(c) if c else None, a["ids"], a["stride"], a["B"], a["T"], a["kept"], a["end_id"],
                                      a["image_index"], a["beta"], a["scores"], a["mean"], None)


def _id(d):
    return "%s=%s" % next(iter(d.items()))


BAD_CORPUS = [dict(ref_tokens=None), dict(ref_offsets=None), dict(image_offsets=None), dict(n_tokens=0), dict(n_tokens=-1),
              dict(n_refs=0), dict(n_refs=-1), dict(n_images=0), dict(n_images=-2), dict(max_ref_tokens=0), dict(max_ref_tokens=-1)]
BAD_ROWS = [dict(ids=None), dict(image_index=None), dict(B=0), dict(B=-3), dict(T=0), dict(T=-1), dict(stride=19)]


@pytest.mark.parametrize("bad", BAD_CORPUS, ids=_id)
def test_corpus_argument_errors_without_a_launch(bad):
    assert bleu_call(corpus(**bad)) == 1001
    assert rouge_call(corpus(**bad)) == 1001


@pytest.mark.parametrize("bad", BAD_ROWS + [dict(comps=None), dict(sentence=None)], ids=_id)
def test_bleu_argument_errors_without_a_launch(bad):
    assert bleu_call(**bad) == 1001


@pytest.mark.parametrize("bad", BAD_ROWS + [dict(scores=None), dict(mean=None), dict(beta=0.0), dict(beta=-1.2),
                                            dict(beta=float("nan")), dict(beta=float("inf"))], ids=_id)
def test_rouge_argument_errors_without_a_launch(bad):
    assert rouge_call(**bad) == 1001


def test_null_corpus_and_finalize_pointers_are_argument_errors():
    assert bleu_call(False) == 1001 and rouge_call(False) == 1001
    assert L.load().sat_bleu_finalize(None, P, None) == 1001
    assert L.load().sat_bleu_finalize(P, None, None) == 1001


def test_sizes_past_the_kernels_limits_are_unsupported_without_a_launch():
    assert bleu_call(T=65, stride=65) == 1003 and rouge_call(T=65, stride=65) == 1003
    assert bleu_call(corpus(max_ref_tokens=129)) == 1003 and rouge_call(corpus(max_ref_tokens=129)) == 1003


def test_scorers_validate_on_the_host_before_any_gpu_work():
    ok = [[[1, 2, 3]], [[4, 5], []]]
    for n in (1, 3, 5):
        with pytest.raises(ValueError, match="n = 4"):
            sat.BleuScorer(ok, n=n)
    for beta in (0.0, -1.2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            sat.RougeLScorer(ok, beta=beta)
    for cls in (sat.BleuScorer, sat.RougeLScorer):
        for bad in ([], [[[1]], []], [[[1, -1]]], [[[2 ** 31]]], [[list(range(129))]], [[[]], [[]]]):
            with pytest.raises(ValueError):
                cls(bad)
        for bad in ([[[1.5]]], [[["a"]]], [[[True]]]):
            with pytest.raises(TypeError):
                cls(bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(ok, device="cpu")                                              # everything in order, but not on the GPU
        with pytest.raises(TypeError, match="from_scorer"):
            cls.from_scorer(object())
    with pytest.raises(ValueError, match="n = 4"):
        sat.BleuScorer.from_scorer(object(), n=2)
    with pytest.raises(ValueError, match="beta"):
        sat.RougeLScorer.from_scorer(object(), beta=0.0)


@pytest.mark.parametrize("cls", ["BleuScorer", "RougeLScorer"])
def test_score_validates_its_arguments_on_the_host(cls):
    s = object.__new__(getattr(sat, cls))           # the host checks need no corpus on a device
    s.n_images = 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.score(torch.zeros(2, 20, dtype=torch.int64), [0, 1])
    for bad in ([0, 3], [-1, 0], [[0, 1]], [0.0, 1.0]):
        with pytest.raises((ValueError, TypeError)):
            s._image_index(bad, 2)
    if cls == "BleuScorer":
        for order in (0, 5, 2.0, True, None):
            with pytest.raises(ValueError, match="order"):
                s.score(torch.zeros(2, 20, dtype=torch.int64), [0, 1], order=order)
        s.totals = None
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            s.update(torch.zeros(2, 20, dtype=torch.int64), [0, 1])


def test_mixed_reward_validates_its_members():
    class Scorer:
        def score(self, ids, image_index, end_id=2, kept=None):
            return None, torch.tensor([1.0, 2.0], dtype=torch.float64) * end_id

    class Single(Scorer):
        def score(self, ids, image_index, end_id=2, kept=None):
            return None, torch.tensor([1.0, 2.0])

    with pytest.raises(ValueError):
        sat.MixedReward([])
    for bad in ([Scorer()], [(Scorer(),)], [(Scorer(), 1.0, 2.0)], [(object(), 1.0)], [(Scorer(), "1")], [(Scorer(), True)]):
        with pytest.raises(TypeError):
            sat.MixedReward(bad)
    for w in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sat.MixedReward([(Scorer(), w)])
    with pytest.raises(TypeError, match="f64"):
        sat.MixedReward([(Single(), 1.0)]).score(None, None)
    mix = sat.MixedReward([(Scorer(), 1.0), (Scorer(), 0.5)])          # the sum itself is plain tensor arithmetic
    mean, scores = mix.score(None, None, end_id=3)
    assert scores.tolist() == [4.5, 9.0] and mean.tolist() == [6.75] and mean.dtype == torch.float64 and len(mix.last_scores) == 2


def test_validation_step_rejects_bleu_or_rouge_without_image_index():
    b, r = object.__new__(sat.BleuScorer), object.__new__(sat.RougeLScorer)
    for kw in (dict(bleu=b), dict(rouge=r), dict(bleu=b, rouge=r), dict(bleu=b, scorer=object())):
        with pytest.raises(ValueError, match="image_index"):
            sat.validation_step(None, None, None, None, **kw)
    with pytest.raises(ValueError, match="scorer and image_index go together"):       # as before
        sat.validation_step(None, None, None, None, image_index=[0])
    with pytest.raises(ValueError, match="scorer and image_index go together"):
        sat.validation_step(None, None, None, None, scorer=object())
