"""GPU (program construction allocates device buffers): the committed tuning table (show-and-tell_amd/tune/gfx950.json) names,
for every conv of the BASELINE programs, a variant that op RUNS.  A variant the op cannot run is replaced silently at launch,
and `OpProgram.signatures()` -- what keeps grouped and ungrouped programs of one model on the same bits -- records the variant
the op names: so every conv op of every program is asked of the library (`sat_conv_resolved_variant`), and the recorded
signatures must be those of the resolved variants."""
import importlib

import pytest
import torch

from conv_cases import resolved

pytestmark = pytest.mark.gpu
sat = importlib.import_module("show-and-tell_amd")
L, T = sat._lib, sat.tune


@pytest.fixture()
def table(monkeypatch):
    assert torch.cuda.is_available(), "needs the MI355X"
    for k in ("SAT_AUTOTUNE", "SAT_TUNE_FILE", "SAT_TUNE_TABLE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(T, "_committed", None)
    tab = T.committed()
    assert len(tab) > 0
    return tab


def _check(prog, table, want_of=None):
    """-> number of conv ops whose variant came from the table; every named variant must be the one that runs"""
    lib, wrong, from_table, sigs = L.load(), [], 0, {}
    for i in range(prog.n_ops):
        o = prog.ops[i]
        if o.kind != L.OP_CONV or o.dtype != L.SAT_BF16:
            continue
        assert int(o.variant) > 0, "conv op %d has no variant" % i
        key = T.tune_key(o, want_of(o) if want_of else None)
        got = resolved(lib, o)
        if got != int(o.variant):
            wrong.append((key, int(o.variant), got, key in table))
        from_table += key in table and table[key] == int(o.variant)
        sigs[T.layer_key(o)] = int(lib.sat_conv_variant_signature(got) if (o.stat_partial or o.stat_acc) else lib.sat_conv_variant_family(got))
    assert not wrong, "(key, named, runs, from the table): %s" % wrong
    if hasattr(prog, "signatures"):
        assert prog.signatures() == sigs
    return from_table


def _encoder_programs(enc, images):
    enc._program(images)                   # the grouped lead first, then the ungrouped program within its signatures
    progs = list(enc._programs.values())
    assert sorted(p.groups for p in progs) == [1, enc.lookahead_groups]
    return progs


@pytest.mark.parametrize("defer", ["0", "1"])
@pytest.mark.parametrize("training", [True, False])
def test_resnet152_batch64_programs_run_the_variants_the_table_names(table, monkeypatch, training, defer):
    """BASELINE config 2: ResNet-152, batch 64, 224 x 224 -- the ungrouped program and the two-batch grouped one"""
    monkeypatch.setenv("SAT_DEFER_BN3", defer)
    with torch.no_grad():
        model = sat.ShowAndTell(256, 512, 10000, 1, compute_dtype="bf16").cuda().train(training)
        images = torch.randn(64, 3, 224, 224, device="cuda")
        n = 0
        for prog in _encoder_programs(model.encoder, images):
            n += _check(prog, table, lambda o, p=prog: p._want_sigs.get(T.layer_key(o)))
    print("resnet152 training=%s defer=%s: %d conv ops took their variant from the table" % (training, defer, n))
    assert n > 0


@pytest.mark.parametrize("training", [True, False])
def test_inception_v3_programs_run_the_variants_the_table_names(table, training):
    """Inception-v3 at 299 x 299, batch 64: groups 1 and 3"""
    with torch.no_grad():
        model = sat.ShowAndTell(512, 1024, 10000, 2, arch="inception_v3", compute_dtype="bf16").cuda().train(training)
        assert model.encoder.lookahead_groups == 3
        images = torch.randn(64, 3, 299, 299, device="cuda")
        n = 0
        for prog in _encoder_programs(model.encoder, images):
            n += _check(prog, table, lambda o, p=prog: p._want_sigs.get(T.layer_key(o)))
    print("inception_v3 training=%s: %d conv ops took their variant from the table" % (training, n))
    assert n > 0


def test_vgg16_program_runs_the_variants_the_table_names(table):
    """VGG16 features[:-3], batch 64, 224 x 224 (Show-Attend-Tell)"""
    with torch.no_grad():
        model = sat.ShowAttendTellModel(1024, 512, 10000, 512, None, compute_dtype="bf16").cuda()
        n = _check(model._program_for(torch.randn(64, 3, 224, 224, device="cuda")), table)
    print("vgg16: %d conv ops took their variant from the table" % n)
    assert n > 0
