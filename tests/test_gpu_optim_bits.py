"""GPU: what `TrainStep` and `FusedClampAdam` leave in their flat buffers against recorded BITS -- every case of
tests/golden/make_goldens_optim_bits.py (plain, clamp off, global norm, measured norm, weight decay, averaged weights with and
without warm-up, a dropped update for a NaN, for a fault word set by hand, accumulation, parameters without gradient, state dict
round trips).

The fixture tests/golden/optim/G15_flat_adam_bits.npz was recorded from the tree in front of the one that moved the update
sequence, the averaging and the state dicts of both classes into `optim.FlatAdam` (two runs, byte-identical), so the comparison is
`torch.equal` on every recorded array: no tolerance, nothing left out.  The FusedClampAdam buffers are recorded as they are; the
TrainStep buffers (about 20 000 floats each, 48 of them) as SHA-256 digests, one over the whole buffer and one per parameter
slice, which any changed bit changes.  What the fixture pins is the launch sequence and its arguments -- the tests against the f64
restatements (test_gpu_optim.py, test_gpu_ema.py, test_gpu_grad_accum.py) say that those bits are RIGHT.

The fixture is tied to gfx950 and to the ROCm build it was recorded with.  A failure after a toolchain change alone means:
regenerate it with the script, from a tree whose other optimizer tests pass."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_goldens_optim_bits as MG  # noqa: E402

pytestmark = pytest.mark.gpu

sat = importlib.import_module("show-and-tell_amd")
PATH = os.path.join(HERE, "golden", "optim", MG.NAME)


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(PATH)
    return {k: z[k] for k in z.files}


def check(got, name):
    want = {k: v for k, v in golden().items() if k.startswith(name + "__")}
    assert want and sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        same = torch.equal(torch.from_numpy(got[k]), torch.from_numpy(want[k]))
        rows = [] if same or got[k].dtype != np.uint8 else [i for i in range(len(want[k])) if (got[k][i] != want[k][i]).any()]
        assert same, "%s differs%s" % (k, " (digest rows %s: 0 = whole buffer, then sorted(flat.slices))" % rows if rows else "")


def test_the_fixture_holds_every_case_and_nothing_else():
    cases = list(MG.TS_CASES) + list(MG.FCA_CASES)
    assert len(cases) == 21
    assert {"%s__%s" % (name, f) for name in cases for f in MG.fields(name)} == set(golden())
    assert os.path.getsize(PATH) < 300 * 1024


@pytest.mark.parametrize("name", list(MG.TS_CASES))
def test_train_step_leaves_the_recorded_bits(name):
    check(MG.run_train_step(sat, name), name)


@pytest.mark.parametrize("name", list(MG.FCA_CASES))
def test_fused_clamp_adam_leaves_the_recorded_bits(name):
    check(MG.run_fused_clamp_adam(sat, name), name)
