"""GPU: whole beam decodes against recorded BITS -- sat_beam_decode, sat_beam_decode_ex, sat_beam_decode_groups and
sat_beam_decode_ensemble through `DecoderRNN.sample_beam` and `Ensemble.sample_beam_features`, every case of
tests/golden/make_goldens_beam_bits.py (narrow with one and two layers, K = 1 over an odd number of steps, two layers at 128 rows,
the wide step with the exact-f32 and with the x3 projection; plain, constrained and grouped; every ensemble kind of
tests/ensemble_reference.py).

The fixture tests/golden/beam/G14_beam_decode_bits.npz was recorded from the tree in front of the one that gave the single-model and
the ensemble decode ONE member step and ONE search loop (two runs, byte-identical), so the comparison is `torch.equal` on ids,
scores, last_beam_norm_scores and last_beam_order of every image of every case: no tolerance, no tie filter, nothing left out.
What it pins is the launch sequence and the arithmetic of the decode loops -- the tests against the f64 / CPU restatements
(test_gpu_beam_constraints.py, test_gpu_beam_groups.py, test_gpu_ensemble.py) say that those bits are RIGHT.

The fixture is tied to gfx950 and to the ROCm build it was recorded with: a compiler that contracts or orders a sum differently
changes low bits of the scores.  A failure after a toolchain change alone means: regenerate it with the script, from a tree whose
other beam tests pass."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_goldens_beam_bits as MG  # noqa: E402

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(HERE, "golden", "beam", MG.NAME))
    return {k: z[k] for k in z.files}


def check(got, prefix):
    want = {k: v for k, v in golden().items() if k.startswith(prefix + "__")}
    assert want and sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(want[k])), k


def test_the_fixture_holds_every_case_and_nothing_else():
    keys = set()
    for name, spec in MG.SINGLE.items():
        for mode in spec[-1]:
            ranked = mode != "plain"
            keys |= {"%s__%s__%s" % (name, mode, a) for a in ("ids", "scores") + (("norm", "order") if ranked else ())}
    for kind in MG.ENSEMBLE:
        ranked = kind in ("constrained", "grouped")
        keys |= {"ens_%s__call__%s" % (kind, a) for a in ("ids", "scores") + (("norm", "order") if ranked else ())}
    assert keys == set(golden())
    assert os.path.getsize(os.path.join(HERE, "golden", "beam", MG.NAME)) < 300 * 1024


@pytest.mark.parametrize("name", list(MG.SINGLE))
def test_single_model_decode_returns_the_recorded_bits(name):
    check(MG.decode_single(sat, name), name)


@pytest.mark.parametrize("kind", MG.ENSEMBLE)
def test_ensemble_decode_returns_the_recorded_bits(kind):
    check(MG.decode_ensemble(sat, kind), "ens_" + kind)
