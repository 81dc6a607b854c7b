"""CPU: the conv variant case table (tests/conv_cases.py) is complete and every row runs the kernel it names, asked of the
library's own selection code (`sat_conv_resolved_variant`: host only, the same prepare_args / variant_ok / heuristic_variant as
the launch) on ops with dummy pointers -- so the table is verified before any GPU time is spent.  Plus the fall-backs a test
can walk into without noticing, as negative rows, and the committed tuning table's stamp."""
import ctypes as C
import json

import pytest

import conv_cases as cc

L = cc.L


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_case_table_covers_every_variant_in_every_admitted_mode(lib):
    assert lib.sat_conv_num_variants() == 41 == len({v for v, _, _ in cc.CASES})
    cc.check_complete()
    assert len(set(cc.CASES)) == len(cc.CASES)
    assert all(g in cc.GEOS for _, _, g in cc.CASES) and {g for _, _, g in cc.CASES} == set(cc.GEOS)
    # a deleted row, a variant without rows and a row outside the family table are all noticed
    only = [r for r in cc.CASES if (r[0], r[1]) == (24, "atomic")]
    with pytest.raises(AssertionError, match=r"no row for \(variant, mode\): \[\(24, 'atomic'\)\]"):
        cc.check_complete([r for r in cc.CASES if r not in only])
    with pytest.raises(AssertionError, match="no row"):
        cc.check_complete([r for r in cc.CASES if r[0] != 41])
    with pytest.raises(AssertionError, match="does not admit"):
        cc.check_complete(cc.CASES + [(24, "slab", "r3x3")])


def test_every_row_resolves_to_the_variant_it_names(lib):
    assert not cc.GPU_ONLY_ROWS                      # no predicate reads a device property: every row is checked here
    wrong = [(cc.case_id(r), cc.resolved(lib, cc.host_op(lib, *r))) for r in cc.CASES if cc.resolved(lib, cc.host_op(lib, *r)) != r[0]]
    assert not wrong, wrong


def test_every_ring_variant_meets_its_tails(lib):
    """per ring variant: a ragged last row tile and column tile, a K loop shorter than the ring and one that is no multiple of its
    depth, Cin % 64 != 0, stride 2, a rectangular kernel with per-axis padding"""
    for v, (bn, depth, _, _, _, bm) in cc.RING_PARAMS.items():
        geos = [cc.GEOS[g] for vv, _, g in cc.CASES if vv == v]
        nk = [-(-g["K"] // 64) for g in geos]
        assert any(g["M"] % bm for g in geos), v
        assert any(g["Cout"] % bn and g["Cout"] % 8 == 0 and g["Cout"] > bn for g in geos), v
        assert any(n < depth for n in nk) and any(n > depth and n % depth for n in nk), v
        assert any(g["Cin"] % 64 for g in geos) and any(g["stride"] == 2 for g in geos), v
        assert any(g["KH"] != g["KW"] and g["pad"] != g["padw"] for g in geos), v
        assert any(g["ldc"] > g["Cout"] for g in geos), v
    for v in range(27, 42):                         # every other kernel: a ragged last 128-row tile
        assert any(cc.GEOS[g]["M"] % 128 for vv, _, g in cc.CASES if vv == v), v


def test_every_variant_meets_another_of_its_bit_family(lib):
    """the GPU test compares output bits inside `sat_conv_variant_family` and statistics bits inside `sat_conv_variant_signature`
    per (geometry, mode): every variant shares at least one op with another variant of its output family, and every signature
    that more than one variant has is compared on at least one op with statistics"""
    groups = {}
    for v, mode, geo in cc.CASES:
        groups.setdefault((geo, mode), []).append(v)
    fam, sig = lib.sat_conv_variant_family, lib.sat_conv_variant_signature
    for v in range(1, 42):
        assert any(v in vs and any(u != v and fam(u) == fam(v) for u in vs) for vs in groups.values()), v
        if any(u != v and sig(u) == sig(v) for u in range(1, 42)) and v not in (38, 40):      # (rs and rs8 share no geometry)
            assert any(v in vs and key[1] not in ("none",) + cc.EVAL and any(u != v and sig(u) == sig(v) for u in vs)
                       for key, vs in groups.items()), v


NEGATIVE = [
    # the statistics slabs are 128-row tiles: a 64-row-tile variant with stat_partial
    (24, "slab", "r3x3"), (25, "slab", "r3x3"), (26, "slab", "r3x3"),
    # a 128- or 256-column tile on Cout <= 64, a 256-column tile on Cout <= 128
    (1, "slab", cc._g(5, 8, 8, 320, 64)), (23, "slab", cc._g(5, 8, 8, 320, 64)), (22, "slab", cc._g(2, 9, 9, 24, 72, 3, 3, 2, 1)),
    (24, "atomic", cc._g(2, 9, 9, 64, 128)),
    # the in-LDS input transform lives in the plain unified-wave loop: wave-specialised / prefetching variants with a fused input BatchNorm
    (11, "bn_table", "r1x1_k5"), (17, "bn_derive", "r1x1_k5"), (16, "bn_table", "r1x1_k5"),
    # ... and is 1x1-only: a ring variant on a 3x3 conv with a fused input BatchNorm runs the LDS-patch kernel
    (1, "bn_table", "p_w13"),
    # special kernels outside their geometry: xp at K = 320, pr / pw on a wide image, aw8 at Cout % 256 != 0, ap at K = 512, rs64 on 32 channels
    (27, "slab", "r1x1_k5"), (30, "slab", cc._g(1, 4, 40, 64, 128, 3, 3, 1, 1)), (32, "slab", cc._g(1, 4, 40, 64, 128, 3, 3, 1, 1)),
    (34, "slab", cc._g(3, 9, 13, 512, 128)), (35, "slab", "a_k512"), (39, "slab", "rs_p1"), (31, "eval", "s_w64"), (38, "eval_res", "rs_p0"),
    # conv_ay_kernel without the second operand, and any other kernel with it
    (36, "bn_table", "a_k512"), (33, "ay_table", "a_k512"),
    # fewer statistics slabs than workgroups (rolling-window kernels own a slab per workgroup)
    (39, "slab", cc._g(3, 4, 50, 64, 64, 3, 3, 1, 1)), (41, "slab", "s_w64"),
]


@pytest.mark.parametrize("variant,mode,geo", NEGATIVE, ids=lambda x: x if isinstance(x, str) else (str(x) if isinstance(x, int) else "geo"))
def test_a_variant_the_op_cannot_run_resolves_to_another(lib, variant, mode, geo):
    o = cc.host_op(lib, variant, mode, geo)
    got = cc.resolved(lib, o)
    assert 1 <= got <= 41 and got != variant
    o.variant = 0
    assert cc.resolved(lib, o) == got                # the built-in choice
    o.variant = variant
    with pytest.raises(AssertionError, match="would run variant %d" % got):
        cc.run_named(lib, o)                         # (fails before anything is launched)


def test_out_of_range_variants_resolve_to_the_built_in_choice_and_rejected_ops_to_zero(lib):
    for mode, geo in [("slab", "r3x3"), ("bn_table", "p_w13"), ("slab", "s_w64"), ("atomic", "rs_p0"), ("eval", "a_k512")]:
        o = cc.host_op(lib, 0, mode, geo)
        want = cc.resolved(lib, o)
        assert want == lib.sat_conv_default_variant(C.byref(o), -1) and want >= 1
        for v in (42, 1000, -1, -1026):
            o.variant = v
            assert cc.resolved(lib, o) == want
    assert lib.sat_conv_resolved_variant(None) == 0
    o = cc.host_op(lib, 1, "slab", "r3x3")
    assert cc.resolved(lib, o) == 1
    for field, value in [("in0", None), ("w", 0x10008), ("kind", L.OP_BN_RELU), ("dtype", L.SAT_F32), ("Cout", 196), ("tiles_m", 3),
                         ("shift1", 0x50000), ("ldc", 64)]:
        o = cc.host_op(lib, 1, "slab", "r3x3")
        setattr(o, field, value)
        assert cc.resolved(lib, o) == 0, field
    # the query changes nothing in the op
    o = cc.host_op(lib, 24, "slab", "r3x3")
    before = bytes(o)
    cc.resolved(lib, o)
    assert bytes(o) == before


def test_both_builds_of_this_tree_export_the_query(lib):
    """`_lib.open_library` binds a symbol added within the ABI version only where a library exports it (an earlier build of the same
    ABI loads); the product library and the -DSAT_TESTHOOKS build made from THIS tree must both have it"""
    import os
    assert "sat_conv_resolved_variant" in L.ADDED_WITHIN_ABI and set(L.ADDED_WITHIN_ABI) <= set(L.SIGNATURES)
    hooks = L.open_library(os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build", "libsat_hip_testhooks.so"))
    for one in (lib, hooks):
        assert one.sat_conv_resolved_variant.argtypes is not None
        assert cc.resolved(one, cc.host_op(one, 1, "slab", "r3x3")) == 1


def test_committed_tuning_table_is_loaded_whole(lib, monkeypatch):
    """`tune.committed()` drops the whole table silently when its ABI / variant-count stamp does not match the library"""
    tune = cc.sat.tune
    monkeypatch.delenv("SAT_TUNE_TABLE", raising=False)
    monkeypatch.setattr(tune, "_committed", None)
    doc = json.load(open(tune.TABLE_PATH))
    assert doc["abi"] == L.ABI_VERSION and doc["variants"] == lib.sat_conv_num_variants()
    assert len(doc["table"]) > 0 and len(tune.committed()) == len(doc["table"])
    assert all(1 <= int(v) <= 41 for v in doc["table"].values())
